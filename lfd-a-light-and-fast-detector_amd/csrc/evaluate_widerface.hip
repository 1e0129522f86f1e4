// csrc/evaluate_widerface.hip -- the WIDERFACE protocol (easy / medium / hard AP) on the device (include/lfd_hip.h,
// lfd_eval_wf_*; the host side is lfd_amd/evaluation.py WIDERFACEEvaluator, the definition is DESIGN.md 9c).  The definition
// restates the dataset's eval_tools from knowledge of them; agreement with those tools is not verified.  Everything is float64
// and evaluated as the definition writes it (-ffp-contract=off, fp64 division is correctly rounded); what leaves the device
// are integer counts, summed with integer atomics, so the result does not depend on the schedule.
//
// The detection store, its status words, the append kernels and the grouping are eval_store.h (boxes are {x, y, w, h}, one
// class, no img_mask); WfDets / WfRows below are what this protocol makes of one row.  A row whose label the caller filters
// out keeps its slot with det_img = -1 and takes part in nothing.  lfd_eval_wf_match:
//   k_wf_minmax   minimum and maximum score over the store (an order-preserving 64-bit key, integer atomicMin / atomicMax);
//   k_wf_faces    faces[d] = sum of the keep-list lengths over every annotated image;
//   k_es_count / k_es_scan / k_es_scatter  group the stored detections by image (histogram, one-workgroup scan, atomic scatter);
//   k_wf_match    a persistent grid draws images from a ticket.  For an image with detections and ground truth a workgroup
//                 ranks the detections by counting (score descending, then store index: the stable sort), computes for every
//                 ranked detection the first ground truth of maximal IoU over 64-wide ground-truth tiles in LDS, lets three
//                 lanes (one per difficulty) walk the detections in rank order, 256 at a time staged through LDS, over the hit state (LDS while the image has at
//                 most WF_HIT_LDS boxes, caller-owned global memory otherwise: no per-image capacity), and lets all lanes
//                 share the thresholds: a binary search in the ranked normalised scores per threshold, the running counts
//                 added into a per-workgroup LDS copy of the curve that is flushed with 64-bit atomics at the end.
#include "eval_store.h"

namespace {

constexpr int WF_THREADS = ES_THREADS;
constexpr int WF_SCAN_THREADS = ES_SCAN_THREADS;
constexpr int WF_TILE = 64;             // ground-truth boxes per LDS tile
constexpr int WF_HIT_LDS = 256;         // images with at most this many boxes keep the hit state in LDS
constexpr int WF_MAX_T = 1024;          // thresholds: the per-workgroup curve is 3 * T * 2 uint32 in LDS
constexpr int WF_GRID = 512;

struct WfArgs {
  lfd_eval_wf_bufs_t b;
  int I, G, cap, T, as_written, label_index;
  double iou;
  // workspace
  int* cnt;        // [I] detections per image
  int* fill;       // [I]
  int* ticket;     // [1] next image of the persistent grid
  int* members;    // [cap] store indices, image-major, any order inside an image
  u64* mm;         // [2] keys of the minimum and the maximum score
  double* rscore;  // [cap] normalised score per grouped position (rank order)
  signed char* hit;  // [3, G] hit state of the images that do not fit LDS
  u64* curve;      // the caller's uint64_t outputs, as the type atomicAdd takes
  u64* faces;
};

__host__ __device__ __forceinline__ EsStore wf_store(const WfArgs& a) {   // one class, no img_mask
  return EsStore{a.b.det_box, a.b.det_score, a.b.det_img, nullptr, a.b.state, nullptr, a.I, 1, a.cap};
}

// order-preserving map double -> u64 (and back): the reduction then is an integer minimum / maximum
__device__ __forceinline__ u64 wf_key(double v) {
  const u64 b = (u64)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double wf_unkey(u64 k) {
  const u64 b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

// float('%.03f' % min(s, 1)) for an fp32 score: 2000 * s is exact in float64 (24-bit significand times 2000 < 2^53), so the
// round-half-even of 1000 * s is decided exactly; k / 1000 is the float64 nearest the three-decimal string
__device__ __forceinline__ double wf_quantise_score(float s32) {
  const double s = (double)s32 <= 1.0 ? (double)s32 : 1.0;
  const double p = 2000.0 * s;
  const double f = floor(p * 0.5);
  const double r = p - 2.0 * f;          // exact, in [0, 2)
  double k = f;
  if (r > 1.0) k = f + 1.0;
  else if (r == 1.0 && fmod(f, 2.0) != 0.0) k = f + 1.0;
  if (k == 0.0) return __builtin_signbit(s) ? -0.0 : 0.0;
  return k / 1000.0;
}

// ------------------------------------------------------------------ appends (the frame is eval_store.h)
struct WfDets : EsDetsDefaults {
  int as_written, label_index;
  static constexpr bool kImageFirst = false;   // an entry that does not fit reports nothing, whatever its ordinal
  __device__ bool marks(int, bool) const { return false; }
  __device__ void drop(const EsStore& s, long long o) const {   // a bad ordinal keeps its slots (the commit counts them), dropped
    s.det_img[o] = -1;
    s.det_score[o] = 0.0;
  }
  __device__ void first(const EsStore& s, long long o, int ord) const {   // as_written: the writer's first line of every file
    es_put(s, o, 0.0, 0.0, 0.0, 0.0, 0.001, ord);
  }
  __device__ void row(const EsStore& s, long long o, int ord, float x1, float y1, float w, float h, float score, int lab) const {
    double x = (double)x1, y = (double)y1, ww = (double)w, hh = (double)h, sc = (double)score;   // {x, y, w, h}
    if (as_written) {
      x = floor(x);
      y = floor(y);
      ww = ceil(ww);
      hh = ceil(hh);
      sc = wf_quantise_score(score);
    }
    es_put(s, o, x, y, ww, hh, sc, (label_index < 0 || lab == label_index) ? ord : -1);   // a filtered label keeps its slot
  }
};

struct WfRows {
  static constexpr int kCols = 6;   // ordinal, score, x, y, w, h
  __device__ void row(const EsStore& s, long long o, const double* r, int ord, bool bad) const {
    es_put(s, o, r[2], r[3], r[4], r[5], r[1], bad ? -1 : ord);
  }
};

// ------------------------------------------------------------------ score range, faces
struct WfImageKey {
  __device__ int operator()(const EsStore& s, int d) const {
    const int img = s.det_img[d];
    return (img >= 0 && img < s.I) ? img : -1;
  }
};
__device__ __forceinline__ int wf_image_of(const WfArgs& a, int d) { return WfImageKey()(wf_store(a), d); }

__global__ __launch_bounds__(WF_THREADS) void k_wf_minmax(WfArgs a) {
  const int n = min(max(a.b.state[0], 0), a.cap);
  u64 lo = ~0ull, hi = 0ull;
  for (int d = blockIdx.x * WF_THREADS + threadIdx.x; d < n; d += gridDim.x * WF_THREADS) {
    if (wf_image_of(a, d) < 0) continue;
    const u64 k = wf_key(a.b.det_score[d]);
    lo = k < lo ? k : lo;
    hi = k > hi ? k : hi;
  }
#pragma unroll
  for (int off = 32; off; off >>= 1) {
    const u64 ol = (u64)__shfl_down((long long)lo, off);
    const u64 oh = (u64)__shfl_down((long long)hi, off);
    lo = ol < lo ? ol : lo;
    hi = oh > hi ? oh : hi;
  }
  if ((threadIdx.x & 63) == 0 && lo <= hi) {
    atomicMin(&a.mm[0], lo);
    atomicMax(&a.mm[1], hi);
  }
}

// one workgroup: faces[d] = sum over every annotated image of its keep-list length
__global__ __launch_bounds__(WF_SCAN_THREADS) void k_wf_faces(WfArgs a) {
  __shared__ u64 s[3];
  if (threadIdx.x < 3) s[threadIdx.x] = 0;
  __syncthreads();
  u64 loc[3] = {0, 0, 0};
  for (int i = threadIdx.x; i < a.I; i += WF_SCAN_THREADS)
    for (int d = 0; d < 3; ++d) loc[d] += (u64)max(a.b.keep_len[i * 3 + d], 0);
  for (int d = 0; d < 3; ++d)
    if (loc[d]) atomicAdd(&s[d], loc[d]);
  __syncthreads();
  if (threadIdx.x < 3) a.faces[threadIdx.x] = s[threadIdx.x];
}

// ------------------------------------------------------------------ matching
// step 4 of the definition for one difficulty: the sequential walk over one chunk of the ranked detections.  code[j] is -1
// (best IoU below the threshold) or (m << 3) | kept bits of m; the running counts go to LDS and carry over in prop / rec
template <typename Hit>
__device__ __forceinline__ void wf_walk(Hit hit, int bit, int lim, const int* code, int* prop_out, int* rec_out, int& prop, int& rec) {
  for (int j = 0; j < lim; ++j) {
    const int c = code[j];
    int p = 1;
    if (c >= 0) {
      const int m = c >> 3;
      if (!(c & bit)) {
        hit[m] = -1;
        p = 0;
      } else if (hit[m] == 0) {
        hit[m] = 1;
        ++rec;
      }
    }
    prop += p;
    prop_out[j] = prop;
    rec_out[j] = rec;
  }
}

__global__ __launch_bounds__(WF_THREADS) void k_wf_match(WfArgs a) {
  __shared__ unsigned s_curve[3 * WF_MAX_T * 2];
  __shared__ double s_gt[WF_TILE * 4];
  __shared__ u64 s_sc[WF_THREADS];
  __shared__ int s_ix[WF_THREADS];
  __shared__ signed char s_hit[3 * WF_HIT_LDS];
  __shared__ int s_code[WF_THREADS], s_prop[3 * WF_THREADS], s_rec[3 * WF_THREADS];
  __shared__ int s_img;
  const int tid = threadIdx.x;
  const int T = a.T;
  for (int c = tid; c < 6 * T; c += WF_THREADS) s_curve[c] = 0;
  // step 1: one subtraction and one division per score
  const double lo = wf_unkey(a.mm[0]), hi = wf_unkey(a.mm[1]);
  double diff = hi - lo;
  if (diff == 0.0) diff = 1.0;
  if (blockIdx.x == 0 && tid == 0 && a.b.minmax) {
    a.b.minmax[0] = lo;
    a.b.minmax[1] = hi;
  }
  for (;;) {
    __syncthreads();
    if (tid == 0) s_img = atomicAdd(a.ticket, 1);
    __syncthreads();
    const int img = s_img;
    if (img >= a.I) break;
    const int d0 = a.b.det_start[img], nd = a.b.det_start[img + 1] - d0;
    const int g0 = a.b.gt_start[img], ng = a.b.gt_start[img + 1] - g0;
    if (nd <= 0 || ng <= 0) continue;

    // step 2: rank = number of the image's detections that come first (higher score, or the same score and stored earlier)
    for (int ib = 0; ib < nd; ib += WF_THREADS) {
      const bool valid = ib + tid < nd;
      const int my = valid ? a.members[d0 + ib + tid] : -1;
      const double ms = valid ? a.b.det_score[my] : 0.0;
      const u64 mk = wf_key(ms + 0.0);       // -0 counts as +0; the keys order NaNs too, so the ranks are always a permutation
      int r = 0;
      for (int jb = 0; jb < nd; jb += WF_THREADS) {
        __syncthreads();
        if (jb + tid < nd) {
          const int ix = a.members[d0 + jb + tid];
          s_ix[tid] = ix;
          s_sc[tid] = wf_key(a.b.det_score[ix] + 0.0);
        }
        __syncthreads();
        if (valid) {
          const int lim = min(WF_THREADS, nd - jb);
          for (int jj = 0; jj < lim; ++jj) {
            const u64 kj = s_sc[jj];
            r += (kj > mk || (kj == mk && s_ix[jj] < my)) ? 1 : 0;
          }
        }
      }
      if (valid && r < nd) {
        a.b.det_index[d0 + r] = my;
        a.rscore[d0 + r] = (ms - lo) / diff;
      }
    }
    __syncthreads();

    // step 3: per ranked detection the first ground truth of maximal IoU; ground truth in ascending order and a strict
    // comparison keep the first index
    for (int ib = 0; ib < nd; ib += WF_THREADS) {
      const bool valid = ib + tid < nd;
      const int pos = d0 + ib + tid;
      double dx = 0, dy = 0, dw = 0, dh = 0;
      if (valid) {
        const double* bx = a.b.det_box + (size_t)a.b.det_index[pos] * 4;
        dx = bx[0]; dy = bx[1]; dw = bx[2]; dh = bx[3];
      }
      const double dx2 = dx + dw, dy2 = dy + dh;
      const double da = (dw + 1.0) * (dh + 1.0);
      double best = -1.0;
      int bm = 0;
      for (int gb = 0; gb < ng; gb += WF_TILE) {
        const int lim = min(WF_TILE, ng - gb);
        __syncthreads();
        if (tid < lim * 4) s_gt[tid] = a.b.gt_box[(size_t)(g0 + gb) * 4 + tid];
        __syncthreads();
        if (valid) {
          for (int gg = 0; gg < lim; ++gg) {
            const double gx = s_gt[gg * 4 + 0], gy = s_gt[gg * 4 + 1], gw = s_gt[gg * 4 + 2], gh = s_gt[gg * 4 + 3];
            const double iw = (fmin(dx2, gx + gw) - fmax(dx, gx)) + 1.0;
            const double ih = (fmin(dy2, gy + gh) - fmax(dy, gy)) + 1.0;
            double iou = 0.0;
            if (iw > 0.0 && ih > 0.0) {
              const double inter = iw * ih;
              iou = inter / ((da + (gw + 1.0) * (gh + 1.0)) - inter);
            }
            if (iou > best) {
              best = iou;
              bm = gb + gg;
            }
          }
        }
      }
      if (valid) {
        a.b.det_gt[pos] = bm;
        a.b.det_over[pos] = best >= a.iou ? 1 : 0;
      }
    }

    // step 4: three lanes, one per difficulty
    const bool lds_hit = ng <= WF_HIT_LDS;
    if (lds_hit) {
      for (int i = tid; i < 3 * WF_HIT_LDS; i += WF_THREADS) s_hit[i] = 0;
    } else {
      for (int i = tid; i < ng; i += WF_THREADS)
        for (int d = 0; d < 3; ++d) a.hit[(size_t)d * a.G + g0 + i] = 0;
    }
    __syncthreads();
    int prop = 0, rec = 0;                       // lanes 0..2: the running counts of their difficulty
    for (int cb = 0; cb < nd; cb += WF_THREADS) {
      const int lim = min(WF_THREADS, nd - cb);
      if (tid < lim) {
        const int pos = d0 + cb + tid;
        const int m = a.b.det_gt[pos];
        s_code[tid] = (a.b.det_over[pos] && m >= 0 && m < ng) ? ((m << 3) | (a.b.gt_kept[g0 + m] & 7)) : -1;
      }
      __syncthreads();
      if (tid < 3) {
        if (lds_hit) wf_walk(s_hit + tid * WF_HIT_LDS, 1 << tid, lim, s_code, s_prop + tid * WF_THREADS, s_rec + tid * WF_THREADS, prop, rec);
        else wf_walk(a.hit + (size_t)tid * a.G + g0, 1 << tid, lim, s_code, s_prop + tid * WF_THREADS, s_rec + tid * WF_THREADS, prop, rec);
      }
      __syncthreads();
      if (tid < lim) {
        for (int d = 0; d < 3; ++d) {
          a.b.det_prop[(size_t)d * a.cap + d0 + cb + tid] = s_prop[d * WF_THREADS + tid];
          a.b.det_rec[(size_t)d * a.cap + d0 + cb + tid] = s_rec[d * WF_THREADS + tid];
        }
      }
    }
    __syncthreads();

    // step 5: the ranked normalised scores do not increase, so n = #{s' >= thr} is a binary search
    for (int t = tid; t < T; t += WF_THREADS) {
      const double thr = a.b.thr[t];
      int l = 0, h = nd;
      while (l < h) {
        const int mid = (l + h) >> 1;
        if (a.rscore[d0 + mid] >= thr) l = mid + 1;
        else h = mid;
      }
      if (l > 0) {
        for (int d = 0; d < 3; ++d) {
          s_curve[(d * T + t) * 2 + 0] += (unsigned)a.b.det_prop[(size_t)d * a.cap + d0 + l - 1];
          s_curve[(d * T + t) * 2 + 1] += (unsigned)a.b.det_rec[(size_t)d * a.cap + d0 + l - 1];
        }
      }
    }
    if (a.b.det_flags) {
      for (int j = tid; j < nd; j += WF_THREADS) {
        int f = a.b.det_over[d0 + j] ? 1 : 0;
        for (int d = 0; d < 3; ++d) {
          const int32_t* po = a.b.det_prop + (size_t)d * a.cap + d0;
          f |= (po[j] - (j ? po[j - 1] : 0)) ? (2 << d) : 0;
        }
        a.b.det_flags[d0 + j] = (uint8_t)f;
      }
    }
  }
  __syncthreads();
  // a cell of s_curve was only ever touched by thread (t mod WF_THREADS); a workgroup's sums stay below det_capacity <= 2^30
  for (int c = tid; c < 6 * T; c += WF_THREADS)
    if (s_curve[c]) atomicAdd(&a.curve[c], (u64)s_curve[c]);
}

// ------------------------------------------------------------------ host
bool wf_desc_ok(const lfd_eval_wf_desc_t* d) {
  if (!d) return false;
  if (d->num_images < 1 || d->num_gt < 0 || d->det_capacity < 1 || d->num_thresholds < 1) return false;
  return d->iou_thresh == d->iou_thresh;
}
// counters and offsets of the grouping are 32-bit; the per-workgroup curve lives in LDS
bool wf_desc_supported(const lfd_eval_wf_desc_t* d) {
  return d->num_images <= (1 << 24) && d->det_capacity <= (1 << 30) && d->num_gt <= (1 << 24) && d->num_thresholds <= WF_MAX_T;
}

WfArgs wf_args(const lfd_eval_wf_desc_t* d, const lfd_eval_wf_bufs_t* b) {
  WfArgs a{};
  if (b) {
    a.b = *b;
    a.curve = reinterpret_cast<u64*>(b->curve);
    a.faces = reinterpret_cast<u64*>(b->faces);
  }
  a.I = d->num_images; a.G = d->num_gt; a.cap = d->det_capacity; a.T = d->num_thresholds;
  a.as_written = d->as_written ? 1 : 0;
  a.label_index = d->label_index;
  a.iou = d->iou_thresh;
  return a;
}

size_t wf_carve(WfArgs& a, void* ws) {
  LfdCarver c(ws);
  a.cnt = c.take<int>(2 * (size_t)a.I + 1);   // cnt, fill and the ticket are contiguous: one memset zeroes them
  a.fill = a.cnt + a.I;
  a.ticket = a.fill + a.I;
  a.members = c.take<int>(a.cap);
  a.mm = c.take<u64>(2);
  a.rscore = c.take<double>(a.cap);
  a.hit = c.take<signed char>(3 * (size_t)max(a.G, 1));
  return c.used();
}

bool wf_store_ok(const lfd_eval_wf_bufs_t* b) { return b && b->det_box && b->det_score && b->det_img && b->state; }

}  // namespace

extern "C" {

int lfd_eval_wf_append_dets_f32(const lfd_eval_wf_desc_t* desc, const lfd_eval_wf_bufs_t* bufs, const float* dets,
                                const int32_t* labels, const int32_t* counts, int32_t n, int32_t cap, const int32_t* img_ord,
                                lfd_stream_t stream) {
  if (!wf_desc_ok(desc) || !wf_store_ok(bufs) || !dets || !labels || !counts || !img_ord) return LFD_ERR_INVALID_ARGUMENT;
  if (n < 1 || cap < 1) return LFD_ERR_INVALID_ARGUMENT;
  if (!wf_desc_supported(desc) || n > 65535) return LFD_ERR_UNSUPPORTED;
  const WfArgs a = wf_args(desc, bufs);
  WfDets p;
  p.as_written = a.as_written;
  p.label_index = a.label_index;
  return es_append_dets(wf_store(a), p, dets, labels, counts, n, cap, img_ord, a.as_written, stream);   // as_written: one dummy row per entry
}

int lfd_eval_wf_append_rows_f64(const lfd_eval_wf_desc_t* desc, const lfd_eval_wf_bufs_t* bufs, const double* rows, int64_t m,
                                lfd_stream_t stream) {
  if (!wf_desc_ok(desc) || !wf_store_ok(bufs) || m < 0) return LFD_ERR_INVALID_ARGUMENT;
  if (m > 0 && !rows) return LFD_ERR_INVALID_ARGUMENT;
  if (!wf_desc_supported(desc)) return LFD_ERR_UNSUPPORTED;
  if (m == 0) return LFD_OK;
  return es_append_rows(wf_store(wf_args(desc, bufs)), WfRows(), rows, (long long)m, nullptr, 0, stream);
}

size_t lfd_eval_wf_workspace_bytes(const lfd_eval_wf_desc_t* desc) {
  if (!wf_desc_ok(desc) || !wf_desc_supported(desc)) return 0;
  WfArgs a = wf_args(desc, nullptr);
  return wf_carve(a, nullptr);
}

int lfd_eval_wf_match(const lfd_eval_wf_desc_t* desc, const lfd_eval_wf_bufs_t* bufs, void* workspace, size_t workspace_bytes,
                      lfd_stream_t stream) {
  if (!wf_desc_ok(desc) || !wf_store_ok(bufs) || !workspace) return LFD_ERR_INVALID_ARGUMENT;
  if (!bufs->gt_start || !bufs->keep_len || !bufs->thr || !bufs->det_start || !bufs->det_index || !bufs->det_gt || !bufs->det_over ||
      !bufs->det_prop || !bufs->det_rec || !bufs->curve || !bufs->faces)
    return LFD_ERR_INVALID_ARGUMENT;
  if (desc->num_gt > 0 && (!bufs->gt_box || !bufs->gt_kept)) return LFD_ERR_INVALID_ARGUMENT;
  if (reinterpret_cast<uintptr_t>(workspace) & 255) return LFD_ERR_INVALID_ARGUMENT;
  if (!wf_desc_supported(desc)) return LFD_ERR_UNSUPPORTED;
  WfArgs a = wf_args(desc, bufs);
  if (wf_carve(a, workspace) > workspace_bytes) return LFD_ERR_WORKSPACE_TOO_SMALL;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(a.cnt, 0, (2 * (size_t)a.I + 1) * sizeof(int), st) != hipSuccess) return LFD_ERR_LAUNCH_FAILED;
  if (hipMemsetAsync(a.mm, 0xff, sizeof(u64), st) != hipSuccess) return LFD_ERR_LAUNCH_FAILED;
  if (hipMemsetAsync(a.mm + 1, 0, sizeof(u64), st) != hipSuccess) return LFD_ERR_LAUNCH_FAILED;
  if (hipMemsetAsync(a.curve, 0, (size_t)3 * a.T * 2 * sizeof(u64), st) != hipSuccess) return LFD_ERR_LAUNCH_FAILED;
  hipLaunchKernelGGL(k_wf_minmax, dim3(es_grid(a.cap)), dim3(WF_THREADS), 0, st, a);
  LFD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_wf_faces, dim3(1), dim3(WF_SCAN_THREADS), 0, st, a);
  LFD_CHECK_LAUNCH();
  const EsStore s = wf_store(a);
  hipLaunchKernelGGL(k_es_count<WfImageKey>, dim3(es_grid(a.cap)), dim3(ES_THREADS), 0, st, s, a.cnt);
  LFD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_es_scan, dim3(1), dim3(ES_SCAN_THREADS), 0, st, a.cnt, a.I, a.b.det_start, a.b.state);
  LFD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_es_scatter<WfImageKey>, dim3(es_grid(a.cap)), dim3(ES_THREADS), 0, st, s, a.b.det_start, a.fill, a.members);
  LFD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_wf_match, dim3((unsigned)min(a.I, WF_GRID)), dim3(WF_THREADS), 0, st, a);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

}  // extern "C"
