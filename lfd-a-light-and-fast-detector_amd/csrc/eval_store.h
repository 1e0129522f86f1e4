// csrc/eval_store.h -- what the three evaluation protocols share (evaluate.hip: COCO, evaluate_tt100k.hip, evaluate_widerface.hip):
// the detection store with its two append paths, and the grouping of the stored detections by a dense key.
//
// The store is caller-owned: det_box [cap, 4], det_score [cap], det_img [cap] (float64, float64, image ordinal), det_cat [cap]
// where the protocol has categories, and the status words state[0] = detections stored, state[1] = LFD_EVAL_ERR_* bits
// (sticky), state[2] = detections grouped by the last match; img_mask [I] marks the images that are evaluated where the
// protocol keeps such a list.  An append is two launches: the append kernel converts and writes its rows behind state[0]
// WITHOUT moving it -- and writes nothing where they would not fit --, the one-thread commit kernel then either advances
// state[0] or raises LFD_EVAL_ERR_CAPACITY.  So every workgroup of the append kernel reads the same state[0].
//   append_dets  one workgroup per batch entry of an ops.DetectOutputs: thread 0 sums the kept counts (counts[j * 4 + 1],
//                clamped to [0, cap]) of the entries before its own, the workgroup forms the fp32 w = x2 - x1 + 1, h (the two
//                roundings of LFD._pack) and hands every row to the protocol;
//   append_rows  a grid-stride loop over float64 rows [ordinal, ...] and over a list of image ordinals to mark.
// What a protocol does differently is its policy, a small struct passed by value (see EsDetsPolicy / EsRowsPolicy below).
// Grouping: es_count<Key> histograms key(detection) over the store, es_scan turns the histogram into offsets with one
// workgroup, es_scatter<Key> writes every detection's store index into a slot of its key (atomic: any order inside a key).
#pragma once
#include "common.h"

namespace {

typedef unsigned long long u64;

constexpr int ES_THREADS = 256;
constexpr int ES_SCAN_THREADS = 1024;

struct EsStore {
  double* det_box;
  double* det_score;
  int32_t* det_img;
  int32_t* det_cat;    // nullptr: the protocol has one class
  int32_t* state;
  int32_t* img_mask;   // nullptr: the protocol evaluates every image
  int I, K, cap;
};

struct OpAdd { __device__ u64 operator()(u64 x, u64 y) const { return x + y; } };

// inclusive Hillis-Steele scan over the workgroup, s: [2 * NT]
template <typename T, int NT, typename Op>
__device__ __forceinline__ T ev_block_scan(T v, T* s, Op op) {
  const int t = threadIdx.x;
  int cur = 0;
  s[t] = v;
  __syncthreads();
#pragma unroll 1
  for (int off = 1; off < NT; off <<= 1) {
    T x = s[cur * NT + t];
    if (t >= off) x = op(s[cur * NT + t - off], x);
    s[(cur ^ 1) * NT + t] = x;
    cur ^= 1;
    __syncthreads();
  }
  const T r = s[cur * NT + t];
  __syncthreads();
  return r;
}

// ------------------------------------------------------------------ small pieces
__device__ __forceinline__ int es_count_of(const int32_t* counts, int j, int cap) { return min(max(counts[j * 4 + 1], 0), cap); }

// slots that the batch entries [0, n) take: their kept boxes and `extra` more each
__device__ __forceinline__ long long es_slots(const int32_t* counts, int n, int cap, int extra) {
  long long total = 0;
  for (int j = 0; j < n; ++j) total += es_count_of(counts, j, cap) + extra;
  return total;
}

__device__ __forceinline__ int es_stored(const EsStore& s) { return min(max(s.state[0], 0), s.cap); }

__device__ __forceinline__ bool es_image_ok(const EsStore& s, int ord) { return ord >= 0 && ord < s.I; }

__device__ __forceinline__ void es_put(const EsStore& s, long long o, double b0, double b1, double b2, double b3, double score, int img) {
  s.det_box[o * 4 + 0] = b0;
  s.det_box[o * 4 + 1] = b1;
  s.det_box[o * 4 + 2] = b2;
  s.det_box[o * 4 + 3] = b3;
  s.det_score[o] = score;
  s.det_img[o] = img;
}

// label -> category index through the caller's table; a label without a category raises LFD_EVAL_ERR_LABEL and gives -1
__device__ __forceinline__ int es_label_category(const EsStore& s, const int32_t* label_map, int num_labels, int lab) {
  const int cat = (lab >= 0 && lab < num_labels) ? label_map[lab] : -1;
  if (cat >= 0 && cat < s.K) return cat;
  atomicOr(&s.state[1], LFD_EVAL_ERR_LABEL);
  return -1;
}

// ------------------------------------------------------------------ appends
// EsDetsPolicy: what a protocol says about append_dets.
//   kImageFirst      a bad image ordinal is reported before (true) or after (false) the capacity test
//   marks(c, fits)   whether thread 0 marks the entry's image in img_mask; c kept boxes, fits: the entry passed the capacity test
//   drop(s, o)       what slot o of an entry with a bad ordinal becomes (only reached when the entry fits)
//   first(s, o, ord) the row that precedes the entry's boxes when the call has extra = 1
//   row(s, o, ord, x1, y1, w, h, score, label)   converts and stores one kept box
struct EsDetsDefaults {   // a protocol's policy derives from this and says where it differs
  static constexpr bool kImageFirst = true;
  __device__ void drop(const EsStore&, long long) const {}
  __device__ void first(const EsStore&, long long, int) const {}
};

template <typename P>
__global__ __launch_bounds__(ES_THREADS) void k_es_append_dets(EsStore s, P p, const float* dets, const int32_t* labels, const int32_t* counts,
                                                               int cap, const int32_t* img_ord, int extra) {
  __shared__ long long s_base;
  const int i = blockIdx.x;
  if (threadIdx.x == 0) s_base = s.state[0] + es_slots(counts, i, cap, extra);
  __syncthreads();
  long long base = s_base;
  const int c = es_count_of(counts, i, cap);
  const int ord = img_ord[i];
  const bool fits = base + c + extra <= s.cap;   // where not, k_es_commit_dets raises LFD_EVAL_ERR_CAPACITY
  if (!es_image_ok(s, ord)) {
    if (!fits && !P::kImageFirst) return;
    if (threadIdx.x == 0) atomicOr(&s.state[1], LFD_EVAL_ERR_IMAGE);
    if (fits)
      for (int j = threadIdx.x; j < c + extra; j += ES_THREADS) p.drop(s, base + j);
    return;
  }
  if (threadIdx.x == 0 && p.marks(c, fits)) s.img_mask[ord] = 1;
  if (!fits) return;
  if (extra) {
    if (threadIdx.x == 0) p.first(s, base, ord);
    base += 1;
  }
  for (int j = threadIdx.x; j < c; j += ES_THREADS) {
    const float* d = dets + ((long long)i * cap + j) * 5;
    const float x1 = d[0], y1 = d[1];
    const float w = d[2] - x1 + 1.0f, h = d[3] - y1 + 1.0f;   // fp32, as LFD._pack
    p.row(s, base + j, ord, x1, y1, w, h, d[4], labels[(long long)i * cap + j]);
  }
}

__device__ __forceinline__ void es_commit(const EsStore& s, long long total) {
  if ((long long)s.state[0] + total > s.cap) atomicOr(&s.state[1], LFD_EVAL_ERR_CAPACITY);
  else s.state[0] += (int)total;
}

__global__ void k_es_commit_dets(EsStore s, const int32_t* counts, int n, int cap, int extra) {
  if (blockIdx.x == 0 && threadIdx.x == 0) es_commit(s, es_slots(counts, n, cap, extra));
}

// EsRowsPolicy: what a protocol says about append_rows.
//   kCols                      float64 columns of one row; column 0 is the image ordinal
//   row(s, o, r, ord, bad)     converts and stores row r; bad: the ordinal is out of range (LFD_EVAL_ERR_IMAGE is already raised)
// The marks are processed even when the rows do not fit; a good row marks its image where the protocol has an img_mask.
template <typename P>
__global__ __launch_bounds__(ES_THREADS) void k_es_append_rows(EsStore s, P p, const double* rows, long long m, const int32_t* mark, int num_mark) {
  const long long base = s.state[0];
  const long long stride = (long long)gridDim.x * ES_THREADS;
  const long long t0 = (long long)blockIdx.x * ES_THREADS + threadIdx.x;
  for (long long j = t0; j < num_mark; j += stride) {
    const int ord = mark[j];
    if (es_image_ok(s, ord)) s.img_mask[ord] = 1;
    else atomicOr(&s.state[1], LFD_EVAL_ERR_IMAGE);
  }
  if (base + m > s.cap) return;   // k_es_commit_rows raises LFD_EVAL_ERR_CAPACITY
  for (long long j = t0; j < m; j += stride) {
    const double* r = rows + j * P::kCols;
    const int ord = (int)r[0];
    const bool bad = !es_image_ok(s, ord);
    if (bad) atomicOr(&s.state[1], LFD_EVAL_ERR_IMAGE);
    else if (s.img_mask) s.img_mask[ord] = 1;
    p.row(s, base + j, r, ord, bad);
  }
}

__global__ void k_es_commit_rows(EsStore s, long long m) {
  if (blockIdx.x == 0 && threadIdx.x == 0) es_commit(s, m);
}

// ------------------------------------------------------------------ grouping by a dense key
// Key()(s, d): the key of stored detection d in [0, N), or -1: the detection takes part in nothing
template <typename Key>
__global__ __launch_bounds__(ES_THREADS) void k_es_count(EsStore s, int* cnt) {
  const int n = es_stored(s);
  for (int d = blockIdx.x * ES_THREADS + threadIdx.x; d < n; d += gridDim.x * ES_THREADS) {
    const int k = Key()(s, d);
    if (k >= 0) atomicAdd(&cnt[k], 1);
  }
}

// one workgroup: start[0 .. N] = exclusive scan of cnt[0 .. N), the total also into state[2]
__global__ __launch_bounds__(ES_SCAN_THREADS) void k_es_scan(const int* cnt, int N, int* start, int32_t* state) {
  __shared__ u64 sh[2 * ES_SCAN_THREADS];
  const int t = threadIdx.x;
  const int chunk = (N + ES_SCAN_THREADS - 1) / ES_SCAN_THREADS;
  const int p0 = min(N, t * chunk), p1 = min(N, p0 + chunk);
  u64 loc = 0;
  for (int p = p0; p < p1; ++p) loc += (u64)cnt[p];
  const u64 inc = ev_block_scan<u64, ES_SCAN_THREADS>(loc, sh, OpAdd());
  u64 run = inc - loc;
  for (int p = p0; p < p1; ++p) {
    start[p] = (int)run;
    run += (u64)cnt[p];
  }
  if (t == ES_SCAN_THREADS - 1) {
    start[N] = (int)inc;
    state[2] = (int)inc;
  }
}

// fill[] starts at zero; members[start[k] .. start[k + 1]) receives the store indices of key k
template <typename Key>
__global__ __launch_bounds__(ES_THREADS) void k_es_scatter(EsStore s, const int* start, int* fill, int* members) {
  const int n = es_stored(s);
  for (int d = blockIdx.x * ES_THREADS + threadIdx.x; d < n; d += gridDim.x * ES_THREADS) {
    const int k = Key()(s, d);
    if (k < 0) continue;
    const int slot = start[k] + atomicAdd(&fill[k], 1);
    if (slot < start[k + 1] && slot < s.cap) members[slot] = d;
  }
}

// ------------------------------------------------------------------ host
int es_grid(long long items) { return (int)max(1LL, min((items + ES_THREADS - 1) / ES_THREADS, 2048LL)); }

// the two launches of an append; the entry points have checked their arguments
template <typename P>
int es_append_dets(const EsStore& s, const P& p, const float* dets, const int32_t* labels, const int32_t* counts, int n, int cap,
                   const int32_t* img_ord, int extra, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_es_append_dets<P>, dim3(n), dim3(ES_THREADS), 0, st, s, p, dets, labels, counts, cap, img_ord, extra);
  LFD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_es_commit_dets, dim3(1), dim3(64), 0, st, s, counts, n, cap, extra);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

template <typename P>
int es_append_rows(const EsStore& s, const P& p, const double* rows, long long m, const int32_t* mark, int num_mark, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(k_es_append_rows<P>, dim3(es_grid(max(m, (long long)num_mark))), dim3(ES_THREADS), 0, st, s, p, rows, m, mark, num_mark);
  LFD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_es_commit_rows, dim3(1), dim3(64), 0, st, s, m);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

}  // namespace
