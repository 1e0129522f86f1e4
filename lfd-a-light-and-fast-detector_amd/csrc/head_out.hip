// csrc/head_out.hip -- the glue around the head's OUTPUT convs in a training iteration, one launch where autograd ran ~25.
//
// The reference's head ends, per pyramid level, in a classification conv and a regression conv whose outputs leave as
// fp32, the regression one through a learnable per-level `Scale` (lfd_head.py:157-185), and LFD.forward concatenates the
// levels along the point axis (lfd.py:526-542).  The training engine runs the level's convs as ONE padded 1x1 conv
// (ROWS output rows: class rows, 4 regression rows, zeros) on the MFMA kernel; this file is what sits on both sides of it:
//   forward :  y [n, hw, ROWS] fp16  ->  cls[:, p0:p0+hw, :] / reg[:, p0:p0+hw, :] fp32 (x scale) of the concatenated tensors
//   backward:  dcls / dreg fp32 (slices of the concatenated gradients)  ->  dy [n, hw, ROWS] fp16 (x scale x loss scale, rows
//              outside every segment ZERO -- they feed the conv's weight and data gradients), and  dbias += sum d,
//              dscale += sum dreg * raw  through per-block partials + one fixed-order fp64 final (deterministic, no atomics --
//              like every other reduction of train.hip).
// As PyTorch ops this was, per level and iteration: 2 slices -> float, 1 multiply, then 3 multiplies, 3 sums, 5 adds, a
// zero fill, 2 half conversions and 2 strided copies -- 130 of the iteration's 155 PyTorch launches for five levels.
//
// ONE implementation, templated on ROWS and instantiated for 64 (up to 60 class channels + 4) and 128 (merged heads with
// 61..124 class channels -- COCO's 80 + 4 --, separate towers with up to 128):
//   - a pixel's line of y / dy is ROWS / 8 pieces of 16 B, read and written by as many consecutive lanes; a thread is a
//     (pixel, piece) pair and its 8 rows are rows [8 * piece, + 8) -- in both directions at 128 rows, in the backward at 64
//     (the 64-row forward is a thread per (pixel, channel): out_split_body<64>)
//   - fp32 stores of the forward and fp32 gradient loads of the backward go as 16-byte vectors where the segment's layout allows
//     it (channels and first row multiples of 4: 80 + 4, 60 + 4), element by element otherwise (the shipped 1 + 4)
//   - the block partials are 2 quantities x ROWS rows, written by the block's first 2 * ROWS threads
//   - workspace: kMaxBlocks x 2 x ROWS floats per level (512 KB / 1 MB); the final launch has one block per row
//   - 32-bit pixel / piece indices: n * hw * ROWS < 2^31
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;    // the gradient kernel is a chain of gathers per trip: many short walks, not few long ones

struct Seg {
  float* out;           // forward: [n, points_total, channels] fp32
  const float* grad;    // backward: same layout
  float* dbias;         // [channels], +=
  const float* scale;   // device scalar or null
  float* dscale;        // device scalar, += (null: none)
  int channels, row0;
  int vec4;             // out / grad may be moved as float4 from channel offsets that are multiples of 4
};

struct Args {
  const __half* y;      // [n, hw, ROWS]
  __half* dy;           // [n, hw, ROWS]
  int n, hw;
  int64_t points_total, point0;
  int64_t y_total, y_point0;   // y / dy row of (img, p) = img * y_total + y_point0 + p  (a level's own tensor: hw, 0; a level inside
                               // the level-concatenated conv output of the training schedule: points_total, point0)
  Seg seg[2];
  int nsegs;
  float loss_scale;
  float* partials;      // [blocks][2][ROWS]
};

// all pyramid levels of one output conv in ONE launch (blockIdx.y = level; every level keeps the block count of its own launch, so
// values, partial rows and their sums are those of the per-level launches, bit for bit)
struct LevelsArgs {
  Args lv[LFD_MAX_LEVELS];
  int nblocks[LFD_MAX_LEVELS];
  int nlev;
};

// which segment (if any) and which of its channels each of this thread's 8 rows is; quad[h]: rows 4h .. 4h + 3 are four
// consecutive channels of one segment and may move as one float4
struct RowMap {
  int sidx[8], sch[8];
  bool quad[2], any;
};

__device__ __forceinline__ RowMap row_map(const Args& a, int piece) {
  RowMap m;
  m.any = false;
  for (int e = 0; e < 8; ++e) {
    const int r = piece * 8 + e;
    m.sidx[e] = -1; m.sch[e] = 0;
    for (int s = 0; s < a.nsegs; ++s)
      if (r >= a.seg[s].row0 && r < a.seg[s].row0 + a.seg[s].channels) { m.sidx[e] = s; m.sch[e] = r - a.seg[s].row0; m.any = true; }
  }
  for (int h = 0; h < 2; ++h) {
    const int s = m.sidx[4 * h];
    bool q = s >= 0 && a.seg[s].vec4 && (m.sch[4 * h] & 3) == 0;
    for (int e = 1; e < 4; ++e) q = q && m.sidx[4 * h + e] == s;      // (same segment + consecutive rows = consecutive channels)
    m.quad[h] = q;
  }
  return m;
}

union Line8 { uint4 u; _Float16 h[8]; };

template <int ROWS>
__device__ __forceinline__ void out_split_body(const Args& a, int bx, int nbx) {
  constexpr int PIECES = ROWS / 8;
  const int piece = threadIdx.x & (PIECES - 1);
  const RowMap m = row_map(a, piece);
  if (!m.any) return;          // a piece of padding rows only (no barrier below)
  float mul[2] = {1.f, 1.f};
  for (int s = 0; s < a.nsegs; ++s)
    if (a.seg[s].scale) mul[s] = *a.seg[s].scale;
  const int64_t vecs = (int64_t)a.n * a.hw * PIECES;
  for (int64_t v = (int64_t)bx * kThreads + threadIdx.x; v < vecs; v += (int64_t)nbx * kThreads) {
    // 32-bit index arithmetic (fill() refuses n * hw * ROWS >= 2^31): as 64-bit divisions these lines were ~400 instructions
    const unsigned pxu = (unsigned)((uint64_t)v / PIECES), imgu = pxu / (unsigned)a.hw;
    const int64_t img = imgu, p = pxu - imgu * (unsigned)a.hw;
    Line8 in;
    in.u = reinterpret_cast<const uint4*>(a.y)[(img * a.y_total + a.y_point0 + p) * PIECES + piece];
    const int64_t orow = img * a.points_total + a.point0 + p;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float f[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int s = m.sidx[4 * h + e];
        const float v32 = (float)in.h[4 * h + e];
        f[e] = (s >= 0 && a.seg[s].scale) ? v32 * mul[s] : v32;
      }
      if (m.quad[h]) {
        const Seg& g = a.seg[m.sidx[4 * h]];
        *reinterpret_cast<float4*>(g.out + orow * g.channels + m.sch[4 * h]) = make_float4(f[0], f[1], f[2], f[3]);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int s = m.sidx[4 * h + e];
          if (s >= 0) a.seg[s].out[orow * a.seg[s].channels + m.sch[4 * h + e]] = f[e];
        }
      }
    }
  }
}

// ROWS == 64 keeps the form it had before the widths shared a file: one thread per (pixel, segment channel), 2-byte gathers from
// the pixel's 128-byte line.  The shipped 1-class head has 5 live rows of 64, so in the piece form one lane in 8 works and lanes
// of a wave store to 8 distant pixels: 28.0 us against 13.9 us for the five levels of WIDERFACE_LFD_S at 640 x 640, bs 32
// ("Heads with more than 64 output rows"; profiles/head_out_unified_kernel_stats.csv)
template <>
__device__ __forceinline__ void out_split_body<64>(const Args& a, int bx, int nbx) {
  const int64_t pixels = (int64_t)a.n * a.hw;
  for (int s = 0; s < a.nsegs; ++s) {
    const Seg g = a.seg[s];
    const float mul = g.scale ? *g.scale : 1.f;
    const int64_t total = pixels * g.channels;
    for (int64_t i = (int64_t)bx * kThreads + threadIdx.x; i < total; i += (int64_t)nbx * kThreads) {
      const unsigned iu = (unsigned)i, pxu = iu / (unsigned)g.channels, imgu = pxu / (unsigned)a.hw;       // 32-bit, as above
      const int j = (int)(iu - pxu * (unsigned)g.channels);
      const int64_t img = imgu, p = pxu - imgu * (unsigned)a.hw;
      const float v = __half2float(a.y[(img * a.y_total + a.y_point0 + p) * 64 + g.row0 + j]);
      g.out[(img * a.points_total + a.point0 + p) * g.channels + j] = g.scale ? v * mul : v;
    }
  }
}

// the piece is the same in every trip of the grid-stride loop (the stride is a multiple of PIECES), so 8 + 8 sums per thread
// last the walk
template <int ROWS>
__device__ __forceinline__ void out_grad_body(const Args& a, int bx, int nbx) {
  constexpr int PIECES = ROWS / 8;
  static_assert(kThreads % PIECES == 0 && 2 * ROWS <= kThreads, "a thread keeps its piece; the partials have a thread per slot");
  __shared__ float red[kThreads][17];
  const int piece = threadIdx.x & (PIECES - 1);
  const RowMap m = row_map(a, piece);
  bool raw = false;          // does one of my rows belong to a segment with a Scale gradient?
  for (int e = 0; e < 8; ++e) raw = raw || (m.sidx[e] >= 0 && a.seg[m.sidx[e]].dscale);
  float mul[2] = {1.f, 1.f};
  for (int s = 0; s < a.nsegs; ++s)
    if (a.seg[s].scale) mul[s] = *a.seg[s].scale;
  float acc_d[8], acc_r[8];
  for (int e = 0; e < 8; ++e) acc_d[e] = acc_r[e] = 0.f;
  const int64_t vecs = (int64_t)a.n * a.hw * PIECES;
  for (int64_t v = (int64_t)bx * kThreads + threadIdx.x; v < vecs; v += (int64_t)nbx * kThreads) {
    const unsigned pxu = (unsigned)((uint64_t)v / PIECES), imgu = pxu / (unsigned)a.hw;       // 32-bit, see out_split_body
    const int64_t img = imgu, p = pxu - imgu * (unsigned)a.hw;
    const int64_t yrow = img * a.y_total + a.y_point0 + p, grow = img * a.points_total + a.point0 + p;
    Line8 in, o;
    in.u = make_uint4(0, 0, 0, 0);
    if (raw) in.u = reinterpret_cast<const uint4*>(a.y)[yrow * PIECES + piece];
    o.u = make_uint4(0, 0, 0, 0);          // rows outside every segment leave as zero
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float d4[4] = {0.f, 0.f, 0.f, 0.f};
      if (m.quad[h]) {
        const Seg& g = a.seg[m.sidx[4 * h]];
        const float4 t = *reinterpret_cast<const float4*>(g.grad + grow * g.channels + m.sch[4 * h]);
        d4[0] = t.x; d4[1] = t.y; d4[2] = t.z; d4[3] = t.w;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int s = m.sidx[4 * h + e];
          if (s >= 0) d4[e] = a.seg[s].grad[grow * a.seg[s].channels + m.sch[4 * h + e]];
        }
      }
#pragma unroll
      for (int e4 = 0; e4 < 4; ++e4) {
        const int e = 4 * h + e4, s = m.sidx[e];
        if (s < 0) continue;
        const Seg& g = a.seg[s];
        float d = d4[e4];
        if (g.dscale) acc_r[e] += d * (float)in.h[e];          // dL/dscale: sum of dreg * raw
        if (g.scale) d = d * mul[s];
        acc_d[e] += d;                                          // dL/dbias
        o.h[e] = (_Float16)(d * a.loss_scale);
      }
    }
    reinterpret_cast<uint4*>(a.dy)[yrow * PIECES + piece] = o.u;
  }
  for (int e = 0; e < 8; ++e) { red[threadIdx.x][e] = acc_d[e]; red[threadIdx.x][8 + e] = acc_r[e]; }
  __syncthreads();
  // slot (q, r) of the block's partial row: the sum over the threads whose piece holds row r, in thread order
  if (threadIdx.x < 2 * ROWS) {
    const int q = threadIdx.x / ROWS, r = threadIdx.x % ROWS;
    float s = 0.f;
    for (int t = r >> 3; t < kThreads; t += PIECES) s += red[t][q * 8 + (r & 7)];
    a.partials[((size_t)bx * 2 + q) * ROWS + r] = s;
  }
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// sum over the blocks' partials of quantity q, row r: lanes stride over the rows of partials, four requests in flight
// (one thread walking 256 rows one dependent load after the other was 45 us); the order of the additions depends on nblocks alone
template <int ROWS>
__device__ __forceinline__ double column_sum(const float* partials, int nblocks, int q, int r) {
  double s = 0.0;
  int b = threadIdx.x & 63;
  for (; b + 192 < nblocks; b += 256) {
    float u[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = partials[((size_t)(b + 64 * k) * 2 + q) * ROWS + r];
#pragma unroll
    for (int k = 0; k < 4; ++k) s += (double)u[k];
  }
  for (; b < nblocks; b += 64) s += (double)partials[((size_t)b * 2 + q) * ROWS + r];
  return wave_sum(s);
}

// block = output row r; wave 0: dbias of the row; wave 1 of a Scale segment's first row: dscale over the segment's rows
template <int ROWS>
__device__ __forceinline__ void out_grad_final_body(const Args& a, int nblocks) {
  const int q = threadIdx.x >> 6, r = blockIdx.x;
  for (int k = 0; k < a.nsegs; ++k) {
    const Seg& g = a.seg[k];
    if (q == 0) {
      if (!g.dbias || r < g.row0 || r >= g.row0 + g.channels) continue;
      const double s = column_sum<ROWS>(a.partials, nblocks, 0, r);
      if ((threadIdx.x & 63) == 0) g.dbias[r - g.row0] += (float)s;
    } else {
      if (!g.dscale || r != g.row0) continue;
      double t = 0.0;
      for (int j = 0; j < g.channels; ++j) t += column_sum<ROWS>(a.partials, nblocks, 1, g.row0 + j);
      if ((threadIdx.x & 63) == 0) *g.dscale += (float)t;
    }
  }
}

template <int ROWS> __global__ __launch_bounds__(kThreads) void k_out_split(Args a) { out_split_body<ROWS>(a, blockIdx.x, gridDim.x); }
template <int ROWS> __global__ __launch_bounds__(kThreads) void k_out_split_levels(LevelsArgs L) {
  const int l = blockIdx.y;
  if ((int)blockIdx.x < L.nblocks[l]) out_split_body<ROWS>(L.lv[l], blockIdx.x, L.nblocks[l]);
}
template <int ROWS> __global__ __launch_bounds__(kThreads) void k_out_grad(Args a) { out_grad_body<ROWS>(a, blockIdx.x, gridDim.x); }
template <int ROWS> __global__ __launch_bounds__(kThreads) void k_out_grad_levels(LevelsArgs L) {
  const int l = blockIdx.y;
  if ((int)blockIdx.x < L.nblocks[l]) out_grad_body<ROWS>(L.lv[l], blockIdx.x, L.nblocks[l]);
}
template <int ROWS> __global__ __launch_bounds__(128) void k_out_grad_final(Args a, int nblocks) { out_grad_final_body<ROWS>(a, nblocks); }
// the levels one after the other in level order: the += into the shared biases happens in the order of the per-level launches
template <int ROWS> __global__ __launch_bounds__(128) void k_out_grad_final_levels(LevelsArgs L) {
  for (int l = 0; l < L.nlev; ++l) out_grad_final_body<ROWS>(L.lv[l], L.nblocks[l]);
}

template <int ROWS> constexpr size_t kLevelPartialFloats = (size_t)kMaxBlocks * 2 * ROWS;

template <int ROWS>
bool fill(Args& a, const void* y, int32_t n, int32_t hw, int64_t points_total, int64_t point0, const lfd_head_out_seg_t* segs,
          int32_t nsegs, bool backward) {
  if (!y || !lfd_aligned16(y) || !segs || n < 1 || hw < 1 || nsegs < 1 || nsegs > 2 || point0 < 0 || point0 + hw > points_total)
    return false;
  if ((int64_t)n * hw * ROWS >= ((int64_t)1 << 31)) return false;       // the kernels index pixels and pieces in 32 bits
  a.y = (const __half*)y; a.n = n; a.hw = hw; a.points_total = points_total; a.point0 = point0; a.nsegs = nsegs;
  a.y_total = hw; a.y_point0 = 0;
  for (int s = 0; s < nsegs; ++s) {
    const lfd_head_out_seg_t& g = segs[s];
    if (g.channels < 1 || g.row0 < 0 || g.row0 + g.channels > ROWS) return false;
    if (s == 1 && !(segs[0].row0 + segs[0].channels <= g.row0 || g.row0 + g.channels <= segs[0].row0)) return false;
    const void* t = backward ? (const void*)g.grad : (const void*)g.out;      // (null: refused by has_tensors)
    a.seg[s] = Seg{g.out, g.grad, g.dbias, g.scale, g.dscale, g.channels, g.row0, (g.channels % 4 == 0 && lfd_aligned16(t)) ? 1 : 0};
  }
  return true;
}

// every segment has its destination (forward) / its gradient, and a Scale behind every Scale gradient (backward)
bool has_tensors(const Args& a, bool backward) {
  for (int s = 0; s < a.nsegs; ++s) {
    if (!backward && !a.seg[s].out) return false;
    if (backward && (!a.seg[s].grad || (a.seg[s].dscale && !a.seg[s].scale))) return false;
  }
  return true;
}

// blocks of a level: a thread per (pixel, piece); the 64-row forward: a thread per (pixel, channel of the larger segment)
template <int ROWS>
int blocks_for(const Args& a, bool backward) {
  int per_pixel = ROWS / 8;
  if (ROWS == 64 && !backward) {
    per_pixel = 0;
    for (int s = 0; s < a.nsegs; ++s)
      if (a.seg[s].channels > per_pixel) per_pixel = a.seg[s].channels;
  }
  const int64_t b = ((int64_t)a.n * a.hw * per_pixel + kThreads - 1) / kThreads;
  return (int)(b > kMaxBlocks ? kMaxBlocks : b);
}

template <int ROWS>
int out_split(const void* y, int32_t n, int32_t hw, int64_t points_total, int64_t point0, const lfd_head_out_seg_t* segs,
              int32_t nsegs, bool concat, lfd_stream_t stream) {
  Args a{};
  if (!fill<ROWS>(a, y, n, hw, points_total, point0, segs, nsegs, false)) return LFD_ERR_INVALID_ARGUMENT;
  if (concat) { a.y_total = points_total; a.y_point0 = point0; }
  if (!has_tensors(a, false)) return LFD_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_out_split<ROWS>, dim3((unsigned)blocks_for<ROWS>(a, false)), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), a);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

template <int ROWS>
int out_grad(const void* y, int32_t n, int32_t hw, int64_t points_total, int64_t point0, const lfd_head_out_seg_t* segs,
             int32_t nsegs, float loss_scale, void* dy, void* workspace, size_t workspace_bytes, bool concat, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  Args a{};
  if (!fill<ROWS>(a, y, n, hw, points_total, point0, segs, nsegs, true) || !dy || !workspace || !lfd_aligned16(dy))
    return LFD_ERR_INVALID_ARGUMENT;
  if (concat) { a.y_total = points_total; a.y_point0 = point0; }
  if (workspace_bytes < kLevelPartialFloats<ROWS> * sizeof(float)) return LFD_ERR_WORKSPACE_TOO_SMALL;
  if (!has_tensors(a, true)) return LFD_ERR_INVALID_ARGUMENT;
  a.dy = (__half*)dy; a.loss_scale = loss_scale; a.partials = reinterpret_cast<float*>(workspace);
  const int b = blocks_for<ROWS>(a, true);
  hipLaunchKernelGGL(k_out_grad<ROWS>, dim3((unsigned)b), dim3(kThreads), 0, st, a);
  LFD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_out_grad_final<ROWS>, dim3(ROWS), dim3(128), 0, st, a, b);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

// mx: the largest block count of a level (the launch's grid.x)
template <int ROWS>
int fill_levels(LevelsArgs& L, int& mx, const void* y_concat, int32_t n, int64_t points_total, const lfd_head_out_level_t* levels,
                int32_t nlevels, bool backward) {
  if (!levels || nlevels < 1 || nlevels > LFD_MAX_LEVELS) return LFD_ERR_INVALID_ARGUMENT;
  L.nlev = nlevels;
  mx = 1;
  for (int l = 0; l < nlevels; ++l) {
    if (!fill<ROWS>(L.lv[l], y_concat, n, levels[l].hw, points_total, levels[l].point0, levels[l].segs, levels[l].nsegs, backward))
      return LFD_ERR_INVALID_ARGUMENT;
    L.lv[l].y_total = points_total; L.lv[l].y_point0 = levels[l].point0;
    L.nblocks[l] = blocks_for<ROWS>(L.lv[l], backward);          // the block count of the per-level entry points
    if (L.nblocks[l] > mx) mx = L.nblocks[l];
  }
  return LFD_OK;
}

template <int ROWS>
int split_levels(const void* y_concat, int32_t n, int64_t points_total, const lfd_head_out_level_t* levels, int32_t nlevels,
                 lfd_stream_t stream) {
  LevelsArgs L{};
  int mx;
  const int rc = fill_levels<ROWS>(L, mx, y_concat, n, points_total, levels, nlevels, false);
  if (rc != LFD_OK) return rc;
  for (int l = 0; l < nlevels; ++l)
    if (!has_tensors(L.lv[l], false)) return LFD_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_out_split_levels<ROWS>, dim3((unsigned)mx, (unsigned)nlevels), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), L);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

template <int ROWS>
int grad_levels(const void* y_concat, int32_t n, int64_t points_total, const lfd_head_out_level_t* levels, int32_t nlevels,
                float loss_scale, void* dy_concat, void* workspace, size_t workspace_bytes, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LevelsArgs L{};
  int mx;
  const int rc = fill_levels<ROWS>(L, mx, y_concat, n, points_total, levels, nlevels, true);
  if (rc != LFD_OK) return rc;
  if (!dy_concat || !workspace || !lfd_aligned16(dy_concat)) return LFD_ERR_INVALID_ARGUMENT;
  if (workspace_bytes < (size_t)nlevels * kLevelPartialFloats<ROWS> * sizeof(float)) return LFD_ERR_WORKSPACE_TOO_SMALL;
  for (int l = 0; l < nlevels; ++l) {
    Args& a = L.lv[l];
    if (!has_tensors(a, true)) return LFD_ERR_INVALID_ARGUMENT;
    a.dy = (__half*)dy_concat; a.loss_scale = loss_scale;
    a.partials = reinterpret_cast<float*>(workspace) + (size_t)l * kLevelPartialFloats<ROWS>;
  }
  hipLaunchKernelGGL(k_out_grad_levels<ROWS>, dim3((unsigned)mx, (unsigned)nlevels), dim3(kThreads), 0, st, L);
  LFD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_out_grad_final_levels<ROWS>, dim3(ROWS), dim3(128), 0, st, L);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

}  // namespace

extern "C" {

// the entry points without `_w` are the 64-row forms the shipped models have always called; the `_w` ones take the row count
#define LFD_HEAD_OUT_ROWS(fn, ...)                  \
  switch (rows) {                                   \
    case 64: return fn<64>(__VA_ARGS__);            \
    case 128: return fn<128>(__VA_ARGS__);          \
    default: return LFD_ERR_INVALID_ARGUMENT;       \
  }

int lfd_head_out_split_f16(const void* y, int32_t n, int32_t hw, int64_t points_total, int64_t point0,
                           const lfd_head_out_seg_t* segs, int32_t nsegs, lfd_stream_t stream) {
  return out_split<64>(y, n, hw, points_total, point0, segs, nsegs, false, stream);
}

int lfd_head_out_split_w_f16(const void* y, int32_t n, int32_t hw, int64_t points_total, int64_t point0,
                             const lfd_head_out_seg_t* segs, int32_t nsegs, int32_t rows, lfd_stream_t stream) {
  LFD_HEAD_OUT_ROWS(out_split, y, n, hw, points_total, point0, segs, nsegs, false, stream)
}

int lfd_head_out_split_concat_f16(const void* y_concat, int32_t n, int32_t hw, int64_t points_total, int64_t point0,
                                  const lfd_head_out_seg_t* segs, int32_t nsegs, lfd_stream_t stream) {
  return out_split<64>(y_concat, n, hw, points_total, point0, segs, nsegs, true, stream);
}

int lfd_head_out_split_concat_w_f16(const void* y_concat, int32_t n, int32_t hw, int64_t points_total, int64_t point0,
                                    const lfd_head_out_seg_t* segs, int32_t nsegs, int32_t rows, lfd_stream_t stream) {
  LFD_HEAD_OUT_ROWS(out_split, y_concat, n, hw, points_total, point0, segs, nsegs, true, stream)
}

int lfd_head_out_grad_f16(const void* y, int32_t n, int32_t hw, int64_t points_total, int64_t point0,
                          const lfd_head_out_seg_t* segs, int32_t nsegs, float loss_scale, void* dy, void* workspace,
                          size_t workspace_bytes, lfd_stream_t stream) {
  return out_grad<64>(y, n, hw, points_total, point0, segs, nsegs, loss_scale, dy, workspace, workspace_bytes, false, stream);
}

int lfd_head_out_grad_w_f16(const void* y, int32_t n, int32_t hw, int64_t points_total, int64_t point0,
                            const lfd_head_out_seg_t* segs, int32_t nsegs, int32_t rows, float loss_scale, void* dy,
                            void* workspace, size_t workspace_bytes, lfd_stream_t stream) {
  LFD_HEAD_OUT_ROWS(out_grad, y, n, hw, points_total, point0, segs, nsegs, loss_scale, dy, workspace, workspace_bytes, false, stream)
}

int lfd_head_out_grad_concat_f16(const void* y_concat, int32_t n, int32_t hw, int64_t points_total, int64_t point0,
                                 const lfd_head_out_seg_t* segs, int32_t nsegs, float loss_scale, void* dy_concat, void* workspace,
                                 size_t workspace_bytes, lfd_stream_t stream) {
  return out_grad<64>(y_concat, n, hw, points_total, point0, segs, nsegs, loss_scale, dy_concat, workspace, workspace_bytes, true, stream);
}

int lfd_head_out_grad_concat_w_f16(const void* y_concat, int32_t n, int32_t hw, int64_t points_total, int64_t point0,
                                   const lfd_head_out_seg_t* segs, int32_t nsegs, int32_t rows, float loss_scale, void* dy_concat,
                                   void* workspace, size_t workspace_bytes, lfd_stream_t stream) {
  LFD_HEAD_OUT_ROWS(out_grad, y_concat, n, hw, points_total, point0, segs, nsegs, loss_scale, dy_concat, workspace, workspace_bytes, true,
                    stream)
}

int lfd_head_out_split_levels_f16(const void* y_concat, int32_t n, int64_t points_total, const lfd_head_out_level_t* levels,
                                  int32_t nlevels, lfd_stream_t stream) {
  return split_levels<64>(y_concat, n, points_total, levels, nlevels, stream);
}

int lfd_head_out_split_levels_w_f16(const void* y_concat, int32_t n, int64_t points_total, const lfd_head_out_level_t* levels,
                                    int32_t nlevels, int32_t rows, lfd_stream_t stream) {
  LFD_HEAD_OUT_ROWS(split_levels, y_concat, n, points_total, levels, nlevels, stream)
}

int lfd_head_out_grad_levels_f16(const void* y_concat, int32_t n, int64_t points_total, const lfd_head_out_level_t* levels,
                                 int32_t nlevels, float loss_scale, void* dy_concat, void* workspace, size_t workspace_bytes,
                                 lfd_stream_t stream) {
  return grad_levels<64>(y_concat, n, points_total, levels, nlevels, loss_scale, dy_concat, workspace, workspace_bytes, stream);
}

int lfd_head_out_grad_levels_w_f16(const void* y_concat, int32_t n, int64_t points_total, const lfd_head_out_level_t* levels,
                                   int32_t nlevels, int32_t rows, float loss_scale, void* dy_concat, void* workspace,
                                   size_t workspace_bytes, lfd_stream_t stream) {
  LFD_HEAD_OUT_ROWS(grad_levels, y_concat, n, points_total, levels, nlevels, loss_scale, dy_concat, workspace, workspace_bytes, stream)
}

#undef LFD_HEAD_OUT_ROWS

}  // extern "C"
