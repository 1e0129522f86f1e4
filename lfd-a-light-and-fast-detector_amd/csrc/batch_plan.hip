// csrc/batch_plan.hip -- plans a whole training batch on the device for lfd_batch_assemble_f32 (include/lfd_hip.h,
// lfd_plan_bbox_crop_batch; the host side is lfd_amd/data.py ResidentDataLoader, the contract DESIGN.md 8b, the restatement
// tests/golden/resident_plan_oracle.py).
//
// k_plan, one workgroup per sample: the eight Philox words and the decisions they fix, the sample's descriptor, its
// 2 * crop_size resize-table entries and its kept boxes in source order (a strided loop over the image's boxes with a
// ballot + LDS scan per 256 boxes, so an image with thousands of boxes keeps their order).  k_compact, one workgroup: scans
// the per-sample counts into `offsets`, copies the staged boxes into the batch's buffer and writes the status words.
//
// Bit exactness: the scale, the resized size and the table fractions are double / float expressions evaluated as
// lfd_amd/data.py writes them (this library is compiled with -ffp-contract=off; fp64 division is correctly rounded).
// Every index into a capacity is checked: nothing is written beyond desc[n], coef[n], stage[n][max_boxes_per_image],
// boxes[max_boxes], offsets[n + 1], status[4].
#include "common.h"

namespace {

constexpr int BP_THREADS = 256;
constexpr int BP_WAVES = BP_THREADS / LFD_WAVE;

struct BpArgs {
  lfd_plan_desc_t d;
  lfd_plan_bufs_t b;
};

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t* out) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// Python's random(): 53 random bits scaled by 2^-53 (exact in double)
__device__ __forceinline__ double uniform53(uint32_t a, uint32_t b) {
  return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6)) * (1.0 / 9007199254740992.0);
}

__device__ __forceinline__ int pick(uint32_t r, int n) { return (int)(((uint64_t)r * (uint64_t)(uint32_t)n) >> 32); }

// int(v) / math.ceil(v) of a double, defined for every input: beyond +-2^30 the sample is refused (LFD_PLAN_BAD_SAMPLE)
__device__ __forceinline__ int to_int(double v, bool* bad) {
  if (!(v > -1073741824.0 && v < 1073741824.0)) { *bad = true; return 0; }
  return (int)v;
}

struct Tap { int i0, i1, w0, w1; };

// data.py _fractions + _weights + column_coefs / row_coefs for one resized column / row `dst`
__device__ __forceinline__ Tap tap_of(int dst, double inv_scale, int src, bool column) {
  const float f = (float)(((double)dst + 0.5) * inv_scale - 0.5);
  const float fl = floorf(f);
  float fr = f - fl;
  long long s = (long long)fl;
  Tap t;
  if (column) {
    if (s < 0) { fr = 0.0f; s = 0; }
    if (s >= src - 1) { fr = 0.0f; s = src - 1; }
    t.i0 = (int)s;
    t.i1 = min((int)s + 1, src - 1);
  } else {
    const long long hi = src - 1;
    t.i0 = (int)min(max(s, 0LL), hi);
    t.i1 = (int)min(max(s + 1, 0LL), hi);
  }
  t.w0 = (int)rintf((1.0f - fr) * 2048.0f);
  t.w1 = (int)rintf(fr * 2048.0f);
  return t;
}

struct Box { int x, y, w, h; };

__device__ __forceinline__ Box scaled_box(const double* p, double scale, bool* bad) {
  Box s;
  s.x = to_int(p[0] * scale, bad);
  s.y = to_int(p[1] * scale, bad);
  s.w = to_int(ceil(p[2] * scale), bad);
  s.h = to_int(ceil(p[3] * scale), bad);
  return s;
}

__global__ __launch_bounds__(BP_THREADS) void k_plan(BpArgs a) {
  __shared__ int s_wave[BP_WAVES];
  __shared__ int s_bad;
  const lfd_plan_desc_t& d = a.d;
  const lfd_plan_bufs_t& b = a.b;
  const int i = blockIdx.x, tid = threadIdx.x;
  const int cs = d.crop_size, mbpi = d.max_boxes_per_image;
  if (tid == 0) s_bad = 0;
  __syncthreads();

  // ---- the sample (every lane computes the same values)
  const int idx = b.indices[i];
  bool bad = idx < 0 || idx >= d.num_images;
  int h = 1, w = 1, box0 = 0, G = 0;
  long long img_off = 0;
  if (!bad) {
    h = b.img_h[idx]; w = b.img_w[idx]; img_off = b.img_offset[idx];
    box0 = b.box_offset[idx];
    const int box1 = b.box_offset[idx + 1];
    if (h < 1 || w < 1 || h > (1 << 30) / w || img_off < 0 || img_off + (long long)h * w * d.c_src > d.arena_bytes ||
        box0 < 0 || box1 < box0 || box1 > d.total_boxes) {
      bad = true; h = w = 1; img_off = 0; box0 = 0;
    } else {
      G = box1 - box0;
    }
  }

  // ---- the draws, at fixed positions
  uint32_t r[8];
  const uint32_t k0 = (uint32_t)(d.seed & 0xffffffffull), k1 = (uint32_t)(d.seed >> 32);
  philox4x32_10((uint32_t)i, d.batch, d.epoch, 0u, k0, k1, r);
  philox4x32_10((uint32_t)i, d.batch, d.epoch, 1u, k0, k1, r + 4);
  const bool resize = uniform53(r[0], r[1]) < d.resize_prob;
  const double scale = resize ? uniform53(r[2], r[3]) * (d.resize_hi - d.resize_lo) + d.resize_lo : 1.0;
  const bool flip = uniform53(r[7], r[7]) < d.flip_prob;
  const double rh_d = rint((double)h * scale), rw_d = rint((double)w * scale);
  const bool empty = !(rh_d >= 1.0 && rw_d >= 1.0);
  const int res_h = empty ? 1 : to_int(rh_d, &bad), res_w = empty ? 1 : to_int(rw_d, &bad);

  // ---- the crop
  Box tgt = {0, 0, res_w, res_h};
  if (G > 0 && !bad && !empty) tgt = scaled_box(b.box + 4 * (long long)(box0 + pick(r[4], G)), scale, &bad);
  const int wr = cs - tgt.w, hr = cs - tgt.h;
  const int crop_x = tgt.x - (min(0, wr) + pick(r[5], abs(wr) + 1));
  const int crop_y = tgt.y - (min(0, hr) + pick(r[6], abs(hr) + 1));
  const bool blank = bad || empty;    // rendered as all zero, no boxes

  // ---- boxes: source order, the dropped ones removed
  int kept = 0;
  if (!blank) {
    for (int c0 = 0; c0 < G; c0 += BP_THREADS) {
      const int j = c0 + tid;
      bool keep = false, jbad = false;
      long long nx = 0, ny = 0, nw = 0, nh = 0;   // (64-bit: the sums of three values below 2^30 each)
      if (j < G) {
        const Box s = scaled_box(b.box + 4 * (long long)(box0 + j), scale, &jbad);
        nx = max(0LL, (long long)s.x - crop_x); ny = max(0LL, (long long)s.y - crop_y);
        nw = min((long long)cs, (long long)s.x + s.w - crop_x) - nx - 1;
        nh = min((long long)cs, (long long)s.y + s.h - crop_y) - ny - 1;
        keep = !jbad && !(nw <= 1 || nx >= cs || nh <= 1 || ny >= cs);
        if (jbad) s_bad = 1;
      }
      const unsigned long long m = __ballot(keep);
      const int lane = tid & (LFD_WAVE - 1), wv = tid / LFD_WAVE;
      if (lane == 0) s_wave[wv] = __popcll(m);
      __syncthreads();
      int before = 0, total = 0;
#pragma unroll
      for (int k = 0; k < BP_WAVES; ++k) {
        if (k < wv) before += s_wave[k];
        total += s_wave[k];
      }
      const int pos = kept + before + __popcll(m & ((1ull << lane) - 1ull));
      if (keep && pos < mbpi) {
        const long long o = (long long)i * mbpi + pos;
        reinterpret_cast<float4*>(b.stage_box)[o] = make_float4((float)(flip ? cs - nx - nw : nx), (float)ny, (float)nw, (float)nh);
        b.stage_label[o] = b.label[box0 + j];
      }
      kept += total;
      __syncthreads();
    }
  }
  __syncthreads();
  const bool coords_bad = s_bad != 0;   // a box beyond 2^30: flagged, the box itself was dropped

  // ---- the resize tables: crop_size columns (before the flip), then crop_size rows
  const double inv = 1.0 / scale;
  const long long dx0 = max(crop_x, 0), dx1 = min((long long)crop_x + cs - 1, (long long)res_w - 1);
  const long long dy0 = max(crop_y, 0), dy1 = min((long long)crop_y + cs - 1, (long long)res_h - 1);
  const bool hit = !blank && dx0 <= dx1 && dy0 <= dy1;
  int wx0 = 0, wy0 = 0, wx1 = 0, wy1 = 0;
  if (hit) {
    wx0 = tap_of((int)dx0, inv, w, true).i0; wx1 = tap_of((int)dx1, inv, w, true).i1;
    wy0 = tap_of((int)dy0, inv, h, false).i0; wy1 = tap_of((int)dy1, inv, h, false).i1;
  }
  int4* tab = reinterpret_cast<int4*>(b.coef) + (long long)i * 2 * cs;
  for (int t = tid; t < 2 * cs; t += BP_THREADS) {
    const bool column = t < cs;
    const long long dst = column ? (long long)crop_x + t : (long long)crop_y + (t - cs);
    int4 e = make_int4(0, 0, 0, 0);
    if (hit) {
      const int org = column ? wx0 : wy0;
      e = make_int4(org, org, 0, 0);
      if (dst >= 0 && dst < (column ? res_w : res_h)) {
        const Tap p = tap_of((int)dst, inv, column ? w : h, column);
        e = make_int4(p.i0, p.i1, p.w0, p.w1);
      }
    }
    tab[t] = e;
  }

  if (tid == 0) {
    lfd_batch_desc_t o;
    const int pitch = w * d.c_src;
    o.src_pitch = pitch;
    o.win_x0 = wx0; o.win_y0 = wy0;
    o.win_w = hit ? wx1 - wx0 + 1 : 1; o.win_h = hit ? wy1 - wy0 + 1 : 1;
    o.src_offset = img_off + (long long)wy0 * pitch + (long long)wx0 * d.c_src;
    o.valid_w = blank ? 0 : cs; o.valid_h = blank ? 0 : cs;
    o.flip = blank ? 0 : (flip ? 1 : 0);
    o.reserved_ = 0;
    b.desc[i] = o;
    int4 c;
    c.x = min(kept, mbpi);
    c.y = max(kept - mbpi, 0);
    c.z = (empty && !bad ? LFD_PLAN_EMPTY_RESIZE : 0) | (bad || coords_bad ? LFD_PLAN_BAD_SAMPLE : 0);
    c.w = blank ? 1 : 0;
    reinterpret_cast<int4*>(b.stage_count)[i] = c;
  }
}

__global__ __launch_bounds__(BP_THREADS) void k_compact(BpArgs a) {
  __shared__ int s_off[LFD_PLAN_MAX_BATCH + 1];
  __shared__ int s_acc[4];   // bits, dropped per image, dropped by the batch capacity, blank samples
  const lfd_plan_desc_t& d = a.d;
  const lfd_plan_bufs_t& b = a.b;
  const int tid = threadIdx.x, n = d.n, mbpi = d.max_boxes_per_image;
  if (tid < 4) s_acc[tid] = 0;
  __syncthreads();
  for (int i = tid; i < n; i += BP_THREADS) {
    const int4 c = reinterpret_cast<const int4*>(b.stage_count)[i];
    s_off[i + 1] = min(max(c.x, 0), mbpi);
    int bits = c.z;
    if (c.y > 0) { bits |= LFD_PLAN_IMAGE_OVERFLOW; atomicAdd(&s_acc[1], c.y); }
    if (bits) atomicOr(&s_acc[0], bits);
    if (c.w) atomicAdd(&s_acc[3], 1);
  }
  __syncthreads();
  if (tid == 0) {
    int run = 0, lost = 0;
    s_off[0] = 0;
    for (int i = 0; i < n; ++i) {
      const int c = s_off[i + 1], take = min(c, d.max_boxes - run);   // the batch's tail goes first
      lost += c - take;
      run += take;
      s_off[i + 1] = run;
    }
    s_acc[2] = lost;
    if (lost) s_acc[0] |= LFD_PLAN_BATCH_OVERFLOW;
  }
  __syncthreads();
  for (int i = tid; i <= n; i += BP_THREADS) b.offsets[i] = s_off[i];
  if (tid < 4) b.status[tid] = s_acc[tid];
  const int total = s_off[n];     // <= max_boxes
  for (int t = tid; t < total; t += BP_THREADS) {
    int lo = 0, hi = n - 1;       // the sample with s_off[lo] <= t < s_off[lo + 1]
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (s_off[mid] <= t) lo = mid; else hi = mid - 1;
    }
    const long long o = (long long)lo * mbpi + (t - s_off[lo]);
    reinterpret_cast<float4*>(b.boxes)[t] = reinterpret_cast<const float4*>(b.stage_box)[o];
    b.labels[t] = b.stage_label[o];
  }
}

}  // namespace

extern "C" {

int lfd_plan_bbox_crop_batch(const lfd_plan_desc_t* d, const lfd_plan_bufs_t* b, lfd_stream_t stream) {
  if (!d || !b) return LFD_ERR_INVALID_ARGUMENT;
  if (!b->img_offset || !b->img_h || !b->img_w || !b->box || !b->label || !b->box_offset || !b->indices || !b->desc ||
      !b->coef || !b->stage_box || !b->stage_label || !b->stage_count || !b->boxes || !b->labels || !b->offsets || !b->status)
    return LFD_ERR_INVALID_ARGUMENT;
  if ((reinterpret_cast<uintptr_t>(b->desc) & 7) || (reinterpret_cast<uintptr_t>(b->stage_label) & 7) ||
      (reinterpret_cast<uintptr_t>(b->labels) & 7) || (reinterpret_cast<uintptr_t>(b->box) & 7) ||
      (reinterpret_cast<uintptr_t>(b->label) & 7) || (reinterpret_cast<uintptr_t>(b->img_offset) & 7))
    return LFD_ERR_INVALID_ARGUMENT;
  if (!lfd_aligned16(b->coef) || !lfd_aligned16(b->stage_box) || !lfd_aligned16(b->stage_count) || !lfd_aligned16(b->boxes))
    return LFD_ERR_INVALID_ARGUMENT;
  if (d->n < 1 || d->crop_size < 1 || (d->c_src != 1 && d->c_src != 3) || d->max_boxes_per_image < 1 || d->max_boxes < 1 ||
      d->num_images < 1 || d->total_boxes < 0 || d->arena_bytes < 0)
    return LFD_ERR_INVALID_ARGUMENT;
  if (!(d->resize_lo - d->resize_lo == 0.0) || !(d->resize_hi - d->resize_hi == 0.0)) return LFD_ERR_INVALID_ARGUMENT;
  if (d->n > LFD_PLAN_MAX_BATCH) return LFD_ERR_UNSUPPORTED;
  if ((long long)d->n * 3 * d->crop_size * d->crop_size >= (1LL << 31)) return LFD_ERR_UNSUPPORTED;
  BpArgs a;
  a.d = *d;
  a.b = *b;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_plan, dim3((unsigned)d->n), dim3(BP_THREADS), 0, st, a);
  LFD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_compact, dim3(1), dim3(BP_THREADS), 0, st, a);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

}  // extern "C"
