// csrc/evaluate_tt100k.hip -- the TT100K protocol (accuracy / recall) on the device (include/lfd_hip.h, lfd_eval_tt100k_*; the
// host side is lfd_amd/evaluation.py TT100KEvaluator, the definition is DESIGN.md 9b).  It restates eval_annos of the
// reference's TT100K_train/official_eval.py: everything is float64 and evaluated as the definition writes it (the library
// is built with -ffp-contract=off and fp64 division is correctly rounded, so an IoU that is computed twice has the same bits).
//
// The detection store, its status words, the append kernels and the grouping are eval_store.h (boxes are {xmin, ymin, xmax,
// ymax} here, scores are scaled to 0..100); TtDets / TtRows below are what this protocol makes of one row.
// lfd_eval_tt100k_match:
//   k_es_count / k_es_scan / k_es_scatter  group the stored detections by image (histogram, one-workgroup scan, atomic scatter);
//   k_tt_order   puts each image's detections back into insertion order (rank by counting) and gathers box, score and
//                category next to each other, so the matching reads contiguous memory;
//   k_tt_match   one workgroup per (image, iou, minscore).  The reference sorts all candidate pairs by IoU descending (a stable
//                sort: ties stay in generation order, ground truth index i first, then detection index j) and matches a pair
//                when both sides are free.  That equals: repeat { take the maximum of (IoU, -i, -j) over the pairs whose two
//                sides are free; match it } until no pair is left -- at most min(G, D) rounds of a workgroup reduction.  The
//                IoU of every pair is kept in LDS when G * D <= TT_TILE; a larger image recomputes the IoU of the free pairs
//                in every round, walking ground truth after ground truth, 256 detections at a time.  The match state lives in
//                caller-owned global memory, so no per-image capacity exists.  The size bands and the counting follow in the
//                same workgroup: every band re-reads the one matching.
#include "eval_store.h"

namespace {

constexpr int TT_THREADS = ES_THREADS;
constexpr int TT_WAVES = TT_THREADS / 64;
constexpr int TT_TILE = 4096;           // IoU values kept in LDS: 32 KiB
constexpr long long TT_MATCH_GRID = 1 << 20;

struct TtArgs {
  lfd_eval_tt100k_bufs_t b;
  int I, K, G, cap, T, M, S, check_type, match_same;
  // workspace
  int* cnt;        // [I] detections per image
  int* fill;       // [I]
  int* members;    // [cap] store indices, image-major, any order inside an image
  double* sbox;    // [cap, 4] image-major, insertion order inside an image
  double* sscore;  // [cap]
  int* scat;       // [cap]
  u64* totals;     // the caller's uint64_t outputs, as the type atomicAdd takes
  u64* percat;
};

__host__ __device__ __forceinline__ EsStore tt_store(const TtArgs& a) {
  return EsStore{a.b.det_box, a.b.det_score, a.b.det_img, a.b.det_cat, a.b.state, a.b.img_mask, a.I, a.K, a.cap};
}

// ------------------------------------------------------------------ appends (the frame is eval_store.h)
struct TtDets : EsDetsDefaults {   // a bad ordinal: LFD_EVAL_ERR_IMAGE whether or not the entry fits, and nothing is written
  const int32_t* label_map;
  int num_labels;
  __device__ bool marks(int, bool) const { return true; }   // before the capacity test: an image without a detection is evaluated too
  __device__ void row(const EsStore& s, long long o, int ord, float x1, float y1, float w, float h, float score, int lab) const {
    // {xmin, ymin, xmax, ymax}: xmax = w + x in float64 from the fp32 w; the score in 0..100
    es_put(s, o, (double)x1, (double)y1, (double)w + (double)x1, (double)h + (double)y1, (double)score * 100.0, ord);
    s.det_cat[o] = es_label_category(s, label_map, num_labels, lab);
  }
};

struct TtRows {
  static constexpr int kCols = 7;   // ordinal, category, score, x, y, w, h
  __device__ void row(const EsStore& s, long long o, const double* r, int ord, bool bad) const {
    int cat = bad ? -1 : (int)r[1];   // a bad ordinal: image -1 with no category, which raises LFD_EVAL_ERR_LABEL as well
    if (cat < 0 || cat >= s.K) {
      atomicOr(&s.state[1], LFD_EVAL_ERR_LABEL);
      cat = -1;
    }
    es_put(s, o, r[3], r[4], r[5] + r[3], r[6] + r[4], r[2] * 100.0, bad ? -1 : ord);
    s.det_cat[o] = cat;
  }
};

// ------------------------------------------------------------------ grouping by image (the kernels are eval_store.h)
struct TtImageKey {
  __device__ int operator()(const EsStore& s, int d) const {
    const int img = s.det_img[d];
    return (img >= 0 && img < s.I && s.img_mask[img]) ? img : -1;
  }
};

// insertion order inside every image: position = number of the image's detections with a smaller store index
__global__ __launch_bounds__(TT_THREADS) void k_tt_order(TtArgs a) {
  __shared__ int s_ix[TT_THREADS];
  const int tid = threadIdx.x;
  for (int img = blockIdx.x; img < a.I; img += gridDim.x) {
    const int d0 = a.b.det_start[img], nd = a.b.det_start[img + 1] - d0;
    for (int ib = 0; ib < nd; ib += TT_THREADS) {
      const bool valid = ib + tid < nd;
      const int my = valid ? a.members[d0 + ib + tid] : -1;
      int r = 0;
      for (int jb = 0; jb < nd; jb += TT_THREADS) {
        __syncthreads();
        if (jb + tid < nd) s_ix[tid] = a.members[d0 + jb + tid];
        __syncthreads();
        if (valid) {
          const int lim = min(TT_THREADS, nd - jb);
          for (int jj = 0; jj < lim; ++jj) r += s_ix[jj] < my ? 1 : 0;
        }
      }
      if (valid && r < nd && my >= 0 && my < a.cap) {
        const size_t s = (size_t)d0 + r;
        a.b.det_index[s] = my;
        a.sbox[s * 4 + 0] = a.b.det_box[(size_t)my * 4 + 0];
        a.sbox[s * 4 + 1] = a.b.det_box[(size_t)my * 4 + 1];
        a.sbox[s * 4 + 2] = a.b.det_box[(size_t)my * 4 + 2];
        a.sbox[s * 4 + 3] = a.b.det_box[(size_t)my * 4 + 3];
        a.sscore[s] = a.b.det_score[my];
        a.scat[s] = a.b.det_cat[my];
      }
    }
    __syncthreads();
  }
}

// ------------------------------------------------------------------ matching
__device__ __forceinline__ double tt_area(double x1, double y1, double x2, double y2) { return fmax(0.0, (x2 - x1) * (y2 - y1)); }

// calc_iou(ground truth, detection) as the definition writes it; 0 / 0 is NaN, which no threshold lets through
__device__ __forceinline__ double tt_iou(const double* g, const double* r) {
  const double cx1 = fmax(g[0], r[0]), cy1 = fmax(g[1], r[1]);
  double cx2 = fmin(g[2], r[2]), cy2 = fmin(g[3], r[3]);
  cx2 = fmax(cx2, cx1);
  cy2 = fmax(cy2, cy1);
  const double ac = tt_area(cx1, cy1, cx2, cy2);
  const double a1 = tt_area(g[0], g[1], g[2], g[3]);
  const double a2 = tt_area(r[0], r[1], r[2], r[3]);
  return ac / (a1 + a2 - ac);
}

__device__ __forceinline__ double tt_long_side(const double* b) { return fmax(b[2] - b[0], b[3] - b[1]); }

// (v, p) beats (bv, bp): larger IoU, then the earlier pair
__device__ __forceinline__ bool tt_better(double v, long long p, double bv, long long bp) {
  return p >= 0 && (bp < 0 || v > bv || (v == bv && p < bp));
}

__global__ __launch_bounds__(TT_THREADS) void k_tt_match(TtArgs a) {
  __shared__ double s_tile[TT_TILE];
  __shared__ double s_v[TT_WAVES];
  __shared__ long long s_p[TT_WAVES];
  __shared__ int s_cnt[3];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int TM = a.T * a.M;
  const long long items = (long long)a.I * TM;
  const double nan = __builtin_nan("");
  for (long long w = blockIdx.x; w < items; w += gridDim.x) {
    const int img = (int)(w / TM), tm = (int)(w % TM);
    if (!a.b.img_mask[img]) continue;
    const int g0 = a.b.gt_start[img], ng = a.b.gt_start[img + 1] - g0;
    const int d0 = a.b.det_start[img], nd = a.b.det_start[img + 1] - d0;
    const double thr = a.b.ious[tm / a.M], msc = a.b.minscores[tm % a.M];
    int* mg = a.b.gt_match + (size_t)tm * max(a.G, 1) + g0;
    int* mr = a.b.det_match + (size_t)tm * a.cap + d0;
    const double* gbox = a.b.gt_box + (size_t)g0 * 4;
    const int* gcat = a.b.gt_cat + g0;
    const double* dbox = a.sbox + (size_t)d0 * 4;
    const int* dcat = a.scat + d0;

    for (int i = tid; i < ng; i += TT_THREADS) {
      const int c = gcat[i];
      mg[i] = (c >= 0 && c < a.K && a.b.cat_in_types[c]) ? -1 : -2;
    }
    for (int j = tid; j < nd; j += TT_THREADS) {
      const int c = dcat[j];
      mr[j] = (c >= 0 && c < a.K && a.b.cat_in_types[c] && !(a.sscore[d0 + j] < msc)) ? -1 : -2;
    }
    __syncthreads();

    const long long pairs = (long long)ng * nd;
    const bool fits = pairs <= TT_TILE;
    if (fits) {
      for (int p = tid; p < (int)pairs; p += TT_THREADS) {
        const int i = p / nd, j = p - i * nd;
        double v = nan;
        if (mg[i] == -1 && mr[j] == -1 && (!a.match_same || gcat[i] == dcat[j])) {
          const double iou = tt_iou(gbox + (size_t)i * 4, dbox + (size_t)j * 4);
          if (iou > thr) v = iou;
        }
        s_tile[p] = v;
      }
      __syncthreads();
    }
    const int rounds = min(ng, nd);
    for (int round = 0; round < rounds; ++round) {
      double bv = 0.0;
      long long bp = -1;
      for (int i = 0; i < ng; ++i) {
        if (mg[i] != -1) continue;   // uniform over the workgroup
        const int ci = gcat[i];
        for (int j = tid; j < nd; j += TT_THREADS) {
          if (mr[j] != -1) continue;
          double v;
          if (fits) {
            v = s_tile[i * nd + j];
          } else {
            if (a.match_same && ci != dcat[j]) continue;
            v = tt_iou(gbox + (size_t)i * 4, dbox + (size_t)j * 4);
          }
          if (!(v > thr)) continue;   // NaN: no candidate
          const long long p = (long long)i * nd + j;
          if (tt_better(v, p, bv, bp)) {
            bv = v;
            bp = p;
          }
        }
      }
#pragma unroll
      for (int off = 32; off; off >>= 1) {
        const double ov = __shfl_down(bv, off);
        const long long op = __shfl_down(bp, off);
        if (tt_better(ov, op, bv, bp)) {
          bv = ov;
          bp = op;
        }
      }
      if (lane == 0) {
        s_v[wave] = bv;
        s_p[wave] = bp;
      }
      __syncthreads();
      bv = s_v[0];
      bp = s_p[0];
#pragma unroll
      for (int x = 1; x < TT_WAVES; ++x)
        if (tt_better(s_v[x], s_p[x], bv, bp)) {
          bv = s_v[x];
          bp = s_p[x];
        }
      if (bp < 0) break;             // the same value in every thread
      if (tid == 0) {
        const int i = (int)(bp / nd), j = (int)(bp - (long long)i * nd);
        mg[i] = j;
        mr[j] = i;
      }
      __syncthreads();
    }
    __syncthreads();

    // size bands and counting
    for (int s = 0; s < a.S; ++s) {
      const double lo = a.b.size_ranges[2 * s], hi = a.b.size_ranges[2 * s + 1];
      const size_t cell = (size_t)tm * a.S + s;
      if (tid < 3) s_cnt[tid] = 0;
      __syncthreads();
      int right = 0, acn = 0, rcn = 0;
      for (int i = tid; i < ng; i += TT_THREADS) {
        const int m = mg[i];
        const double size = tt_long_side(gbox + (size_t)i * 4);
        const bool inb = size >= lo && size < hi;
        const int code = (m == -2 || !inb) ? LFD_TT100K_GT_EXCLUDED : (m >= 0 ? LFD_TT100K_GT_MATCHED : LFD_TT100K_GT_MISSED);
        if (code != LFD_TT100K_GT_EXCLUDED) {
          ++rcn;
          if (a.percat) atomicAdd(&a.percat[(cell * a.K + gcat[i]) * 3 + 2], 1ull);
        }
        if (a.b.gt_code) a.b.gt_code[cell * max(a.G, 1) + g0 + i] = (uint8_t)code;
      }
      for (int j = tid; j < nd; j += TT_THREADS) {
        const int m = mr[j];
        int code = LFD_TT100K_DET_EXCLUDED;
        if (m >= 0) {
          const double size = tt_long_side(gbox + (size_t)m * 4);
          if (size >= lo && size < hi) code = (!a.check_type || gcat[m] == dcat[j]) ? LFD_TT100K_DET_RIGHT : LFD_TT100K_DET_WRONG;
        } else if (m == -1) {
          const double size = tt_long_side(dbox + (size_t)j * 4);
          if (size >= lo && size < hi) code = LFD_TT100K_DET_UNMATCHED;
        }
        if (code != LFD_TT100K_DET_EXCLUDED) {
          ++acn;
          right += code == LFD_TT100K_DET_RIGHT ? 1 : 0;
          if (a.percat) {
            u64* pc = a.percat + (cell * a.K + dcat[j]) * 3;
            atomicAdd(pc + 1, 1ull);
            if (code == LFD_TT100K_DET_RIGHT) atomicAdd(pc, 1ull);
          }
        }
        if (a.b.det_code) a.b.det_code[cell * a.cap + d0 + j] = (uint8_t)code;
      }
      if (right) atomicAdd(&s_cnt[0], right);
      if (acn) atomicAdd(&s_cnt[1], acn);
      if (rcn) atomicAdd(&s_cnt[2], rcn);
      __syncthreads();
      if (tid < 3 && s_cnt[tid]) atomicAdd(&a.totals[cell * 3 + tid], (u64)s_cnt[tid]);
      __syncthreads();
    }
  }
}

// ------------------------------------------------------------------ host
bool tt_desc_ok(const lfd_eval_tt100k_desc_t* d) {
  if (!d) return false;
  if (d->num_images < 1 || d->num_categories < 1 || d->num_gt < 0 || d->det_capacity < 1) return false;
  if (d->num_ious < 1 || d->num_minscores < 1 || d->num_size_ranges < 1) return false;
  return true;
}
// counters and offsets of the grouping are 32-bit
bool tt_desc_supported(const lfd_eval_tt100k_desc_t* d) {
  return d->num_images <= (1 << 24) && d->num_categories <= 65536 && d->det_capacity <= (1 << 30) && d->num_gt <= (1 << 24) &&
         (long long)d->num_ious * d->num_minscores <= 4096 && d->num_size_ranges <= 4096;
}

TtArgs tt_args(const lfd_eval_tt100k_desc_t* d, const lfd_eval_tt100k_bufs_t* b) {
  TtArgs a{};
  if (b) {
    a.b = *b;
    a.totals = reinterpret_cast<u64*>(b->totals);
    a.percat = reinterpret_cast<u64*>(b->per_category);
  }
  a.I = d->num_images; a.K = d->num_categories; a.G = d->num_gt; a.cap = d->det_capacity;
  a.T = d->num_ious; a.M = d->num_minscores; a.S = d->num_size_ranges;
  a.check_type = d->check_type ? 1 : 0;
  a.match_same = d->match_same ? 1 : 0;
  return a;
}

size_t tt_carve(TtArgs& a, void* ws) {
  LfdCarver c(ws);
  a.cnt = c.take<int>(2 * (size_t)a.I);   // cnt and fill are contiguous: one memset zeroes them
  a.fill = a.cnt + a.I;
  a.members = c.take<int>(a.cap);
  a.sbox = c.take<double>((size_t)a.cap * 4);
  a.sscore = c.take<double>(a.cap);
  a.scat = c.take<int>(a.cap);
  return c.used();
}

bool tt_store_ok(const lfd_eval_tt100k_bufs_t* b) {
  return b && b->det_box && b->det_score && b->det_img && b->det_cat && b->state && b->img_mask;
}

}  // namespace

extern "C" {

int lfd_eval_tt100k_append_dets_f32(const lfd_eval_tt100k_desc_t* desc, const lfd_eval_tt100k_bufs_t* bufs, const float* dets,
                                    const int32_t* labels, const int32_t* counts, int32_t n, int32_t cap, const int32_t* label_map,
                                    int32_t num_labels, const int32_t* img_ord, lfd_stream_t stream) {
  if (!tt_desc_ok(desc) || !tt_store_ok(bufs) || !dets || !labels || !counts || !label_map || !img_ord) return LFD_ERR_INVALID_ARGUMENT;
  if (n < 1 || cap < 1 || num_labels < 1) return LFD_ERR_INVALID_ARGUMENT;
  if (!tt_desc_supported(desc) || n > 65535) return LFD_ERR_UNSUPPORTED;
  TtDets p;
  p.label_map = label_map;
  p.num_labels = num_labels;
  return es_append_dets(tt_store(tt_args(desc, bufs)), p, dets, labels, counts, n, cap, img_ord, 0, stream);
}

int lfd_eval_tt100k_append_rows_f64(const lfd_eval_tt100k_desc_t* desc, const lfd_eval_tt100k_bufs_t* bufs, const double* rows,
                                    int64_t m, const int32_t* mark, int32_t num_mark, lfd_stream_t stream) {
  if (!tt_desc_ok(desc) || !tt_store_ok(bufs) || m < 0 || num_mark < 0) return LFD_ERR_INVALID_ARGUMENT;
  if ((m > 0 && !rows) || (num_mark > 0 && !mark)) return LFD_ERR_INVALID_ARGUMENT;
  if (!tt_desc_supported(desc)) return LFD_ERR_UNSUPPORTED;
  if (m == 0 && num_mark == 0) return LFD_OK;
  return es_append_rows(tt_store(tt_args(desc, bufs)), TtRows(), rows, (long long)m, mark, num_mark, stream);
}

size_t lfd_eval_tt100k_workspace_bytes(const lfd_eval_tt100k_desc_t* desc) {
  if (!tt_desc_ok(desc) || !tt_desc_supported(desc)) return 0;
  TtArgs a = tt_args(desc, nullptr);
  return tt_carve(a, nullptr);
}

int lfd_eval_tt100k_match(const lfd_eval_tt100k_desc_t* desc, const lfd_eval_tt100k_bufs_t* bufs, void* workspace,
                          size_t workspace_bytes, lfd_stream_t stream) {
  if (!tt_desc_ok(desc) || !tt_store_ok(bufs) || !workspace) return LFD_ERR_INVALID_ARGUMENT;
  if (!bufs->gt_start || !bufs->cat_in_types || !bufs->ious || !bufs->minscores || !bufs->size_ranges || !bufs->det_start ||
      !bufs->det_index || !bufs->det_match || !bufs->gt_match || !bufs->totals)
    return LFD_ERR_INVALID_ARGUMENT;
  if (desc->num_gt > 0 && (!bufs->gt_box || !bufs->gt_cat)) return LFD_ERR_INVALID_ARGUMENT;
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return LFD_ERR_INVALID_ARGUMENT;
  if (!tt_desc_supported(desc)) return LFD_ERR_UNSUPPORTED;
  TtArgs a = tt_args(desc, bufs);
  if (tt_carve(a, workspace) > workspace_bytes) return LFD_ERR_WORKSPACE_TOO_SMALL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const size_t cells = (size_t)a.T * a.M * a.S;
  if (hipMemsetAsync(a.cnt, 0, 2 * (size_t)a.I * sizeof(int), st) != hipSuccess) return LFD_ERR_LAUNCH_FAILED;
  if (hipMemsetAsync(a.totals, 0, cells * 3 * sizeof(u64), st) != hipSuccess) return LFD_ERR_LAUNCH_FAILED;
  if (a.percat && hipMemsetAsync(a.percat, 0, cells * a.K * 3 * sizeof(u64), st) != hipSuccess)
    return LFD_ERR_LAUNCH_FAILED;
  const EsStore s = tt_store(a);
  hipLaunchKernelGGL(k_es_count<TtImageKey>, dim3(es_grid(a.cap)), dim3(ES_THREADS), 0, st, s, a.cnt);
  LFD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_es_scan, dim3(1), dim3(ES_SCAN_THREADS), 0, st, a.cnt, a.I, a.b.det_start, a.b.state);
  LFD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_es_scatter<TtImageKey>, dim3(es_grid(a.cap)), dim3(ES_THREADS), 0, st, s, a.b.det_start, a.fill, a.members);
  LFD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_tt_order, dim3((unsigned)min(a.I, 65536)), dim3(TT_THREADS), 0, st, a);
  LFD_CHECK_LAUNCH();
  const long long items = (long long)a.I * a.T * a.M;
  hipLaunchKernelGGL(k_tt_match, dim3((unsigned)min(items, TT_MATCH_GRID)), dim3(TT_THREADS), 0, st, a);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

}  // extern "C"
