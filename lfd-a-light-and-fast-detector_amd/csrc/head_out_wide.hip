// csrc/head_out_wide.hip -- head_out.hip for output convs padded to 128 rows: merged heads with 61..124 class channels (COCO's
// 80 + 4 regression rows), separate towers with up to 128.  Same contract as the 64-row file on both sides of the padded conv:
//   forward :  y [n, hw, 128] fp16  ->  cls / reg fp32 (x scale) slices of the level-concatenated tensors
//   backward:  dcls / dreg fp32  ->  dy [n, hw, 128] fp16 (x scale x loss scale, rows outside every segment ZERO -- they feed the
//              conv's weight and data gradients), dbias += / dscale += through per-block partials + one fixed-order fp64 final.
// What differs from the 64-row kernels, which stay as they are in head_out.hip:
//   - a pixel's line of y / dy is 256 B = 16 pieces of 16 B, read and written by 16 consecutive lanes (4 pixels per wave); the
//     forward too is one thread per (pixel, piece) -- its fp32 stores (and the backward's fp32 gradient loads) go as 16-byte
//     vectors where the segment's layout allows it (channels and first row multiples of 4: 80 + 4), element by element otherwise
//   - a thread's 8 rows are rows [8 * (tid & 15), + 8): the segment table is built for 16 pieces
//   - the block partials are 2 quantities x 128 rows = 256 slots, one per thread of the block (kThreads == 2 * kRows)
//   - workspace: kMaxBlocks x 2 x 128 floats = 1 MB per level; the final launch has one block per row, 128
//   - 32-bit pixel / element indices: n * hw * 128 < 2^31
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRows = 128;             // output rows of the padded conv
constexpr int kPieces = kRows / 8;     // 16-byte pieces of a pixel's line
constexpr int kMaxBlocks = 1024;
static_assert(kThreads == 2 * kRows, "the block partials are written one slot per thread");
static_assert(kThreads % kPieces == 0, "a thread keeps its piece over the grid-stride walk");

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
  const __half* y;      // [n, hw, 128]
  __half* dy;           // [n, hw, 128]
  int n, hw;
  int64_t points_total, point0;
  int64_t y_total, y_point0;   // y / dy row of (img, p) = img * y_total + y_point0 + p  (as in head_out.hip)
  Seg seg[2];
  int nsegs;
  float loss_scale;
  float* partials;      // [blocks][2][128]
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

__device__ __forceinline__ void out_split_body(const Args& a, int bx, int nbx) {
  const int piece = threadIdx.x & (kPieces - 1);
  const RowMap m = row_map(a, piece);
  if (!m.any) return;          // a piece of padding rows only (no barrier below)
  float mul[2] = {1.f, 1.f};
  for (int s = 0; s < a.nsegs; ++s)
    if (a.seg[s].scale) mul[s] = *a.seg[s].scale;
  const int64_t vecs = (int64_t)a.n * a.hw * kPieces;
  for (int64_t v = (int64_t)bx * kThreads + threadIdx.x; v < vecs; v += (int64_t)nbx * kThreads) {
    const unsigned pxu = (unsigned)(v >> 4), imgu = pxu / (unsigned)a.hw;       // 32-bit: fill() refuses n * hw * 128 >= 2^31
    const int64_t img = imgu, p = pxu - imgu * (unsigned)a.hw;
    Line8 in;
    in.u = reinterpret_cast<const uint4*>(a.y)[(img * a.y_total + a.y_point0 + p) * kPieces + piece];
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

__global__ __launch_bounds__(kThreads) void k_out_split_wide(Args a) { out_split_body(a, blockIdx.x, gridDim.x); }

// all pyramid levels of one output conv in ONE launch (blockIdx.y = level; every level keeps the block count of its own launch, so
// values, partial rows and their sums are those of the per-level launches, bit for bit)
struct LevelsArgs {
  Args lv[LFD_MAX_LEVELS];
  int nblocks[LFD_MAX_LEVELS];
  int nlev;
};
__global__ __launch_bounds__(kThreads) void k_out_split_levels_wide(LevelsArgs L) {
  const int l = blockIdx.y;
  if ((int)blockIdx.x < L.nblocks[l]) out_split_body(L.lv[l], blockIdx.x, L.nblocks[l]);
}

// thread = (pixel, 16-byte piece of its dy line); the piece is the same in every trip of the grid-stride loop (the stride is a
// multiple of 16), so 8 + 8 sums per thread last the walk
__device__ __forceinline__ void out_grad_body(const Args& a, int bx, int nbx) {
  __shared__ float red[kThreads][17];
  const int piece = threadIdx.x & (kPieces - 1);
  const RowMap m = row_map(a, piece);
  bool raw = false;          // does one of my rows belong to a segment with a Scale gradient?
  for (int e = 0; e < 8; ++e) raw = raw || (m.sidx[e] >= 0 && a.seg[m.sidx[e]].dscale);
  float mul[2] = {1.f, 1.f};
  for (int s = 0; s < a.nsegs; ++s)
    if (a.seg[s].scale) mul[s] = *a.seg[s].scale;
  float acc_d[8], acc_r[8];
  for (int e = 0; e < 8; ++e) acc_d[e] = acc_r[e] = 0.f;
  const int64_t vecs = (int64_t)a.n * a.hw * kPieces;
  for (int64_t v = (int64_t)bx * kThreads + threadIdx.x; v < vecs; v += (int64_t)nbx * kThreads) {
    const unsigned pxu = (unsigned)(v >> 4), imgu = pxu / (unsigned)a.hw;       // 32-bit, see out_split_body
    const int64_t img = imgu, p = pxu - imgu * (unsigned)a.hw;
    const int64_t yrow = img * a.y_total + a.y_point0 + p, grow = img * a.points_total + a.point0 + p;
    Line8 in, o;
    in.u = make_uint4(0, 0, 0, 0);
    if (raw) in.u = reinterpret_cast<const uint4*>(a.y)[yrow * kPieces + piece];
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
    reinterpret_cast<uint4*>(a.dy)[yrow * kPieces + piece] = o.u;
  }
  for (int e = 0; e < 8; ++e) { red[threadIdx.x][e] = acc_d[e]; red[threadIdx.x][8 + e] = acc_r[e]; }
  __syncthreads();
  // slot (q, r) of the block's partial row: the sum over the 16 threads whose piece holds row r, in thread order
  const int q = threadIdx.x >> 7, r = threadIdx.x & (kRows - 1);
  float s = 0.f;
  for (int t = r >> 3; t < kThreads; t += kPieces) s += red[t][q * 8 + (r & 7)];
  a.partials[((size_t)bx * 2 + q) * kRows + r] = s;
}
__global__ __launch_bounds__(kThreads) void k_out_grad_wide(Args a) { out_grad_body(a, blockIdx.x, gridDim.x); }
__global__ __launch_bounds__(kThreads) void k_out_grad_levels_wide(LevelsArgs L) {
  const int l = blockIdx.y;
  if ((int)blockIdx.x < L.nblocks[l]) out_grad_body(L.lv[l], blockIdx.x, L.nblocks[l]);
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// sum over the blocks' partials of quantity q, row r: lanes stride over the rows of partials, four requests in flight; the order
// of the additions depends on nblocks alone
__device__ __forceinline__ double column_sum(const float* partials, int nblocks, int q, int r) {
  double s = 0.0;
  int b = threadIdx.x & 63;
  for (; b + 192 < nblocks; b += 256) {
    float u[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) u[k] = partials[((size_t)(b + 64 * k) * 2 + q) * kRows + r];
#pragma unroll
    for (int k = 0; k < 4; ++k) s += (double)u[k];
  }
  for (; b < nblocks; b += 64) s += (double)partials[((size_t)b * 2 + q) * kRows + r];
  return wave_sum(s);
}

// block = output row r (128 blocks); wave 0: dbias of the row; wave 1 of a Scale segment's first row: dscale over the segment's rows
__device__ __forceinline__ void out_grad_final_body(const Args& a, int nblocks) {
  const int q = threadIdx.x >> 6, r = blockIdx.x;
  for (int k = 0; k < a.nsegs; ++k) {
    const Seg& g = a.seg[k];
    if (q == 0) {
      if (!g.dbias || r < g.row0 || r >= g.row0 + g.channels) continue;
      const double s = column_sum(a.partials, nblocks, 0, r);
      if ((threadIdx.x & 63) == 0) g.dbias[r - g.row0] += (float)s;
    } else {
      if (!g.dscale || r != g.row0) continue;
      double t = 0.0;
      for (int j = 0; j < g.channels; ++j) t += column_sum(a.partials, nblocks, 1, g.row0 + j);
      if ((threadIdx.x & 63) == 0) *g.dscale += (float)t;
    }
  }
}

__global__ __launch_bounds__(128) void k_out_grad_final_wide(Args a, int nblocks) { out_grad_final_body(a, nblocks); }
// the levels one after the other in level order: the += into the shared biases happens in the order of the per-level launches
__global__ __launch_bounds__(128) void k_out_grad_final_levels_wide(LevelsArgs L) {
  for (int l = 0; l < L.nlev; ++l) out_grad_final_body(L.lv[l], L.nblocks[l]);
}

constexpr size_t kLevelPartialFloats = (size_t)kMaxBlocks * 2 * kRows;

bool fill(Args& a, const void* y, int32_t n, int32_t hw, int64_t points_total, int64_t point0, const lfd_head_out_seg_t* segs,
          int32_t nsegs, bool backward) {
  if (!y || !lfd_aligned16(y) || !segs || n < 1 || hw < 1 || nsegs < 1 || nsegs > 2 || point0 < 0 || point0 + hw > points_total)
    return false;
  if ((int64_t)n * hw * kRows >= ((int64_t)1 << 31)) return false;       // the kernels index pixels and pieces in 32 bits
  a.y = (const __half*)y; a.n = n; a.hw = hw; a.points_total = points_total; a.point0 = point0; a.nsegs = nsegs;
  a.y_total = hw; a.y_point0 = 0;
  for (int s = 0; s < nsegs; ++s) {
    const lfd_head_out_seg_t& g = segs[s];
    if (g.channels < 1 || g.row0 < 0 || g.row0 + g.channels > kRows) return false;
    if (s == 1 && !(segs[0].row0 + segs[0].channels <= g.row0 || g.row0 + g.channels <= segs[0].row0)) return false;
    const void* t = backward ? (const void*)g.grad : (const void*)g.out;      // (null: refused by the caller, as in head_out.hip)
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

int blocks_for(int32_t n, int32_t hw) {
  int64_t b = ((int64_t)n * hw * kPieces + kThreads - 1) / kThreads;
  return (int)(b > kMaxBlocks ? kMaxBlocks : b);
}

int out_split(const void* y, int32_t n, int32_t hw, int64_t points_total, int64_t point0, const lfd_head_out_seg_t* segs,
              int32_t nsegs, bool concat, lfd_stream_t stream) {
  Args a{};
  if (!fill(a, y, n, hw, points_total, point0, segs, nsegs, false)) return LFD_ERR_INVALID_ARGUMENT;
  if (concat) { a.y_total = points_total; a.y_point0 = point0; }
  if (!has_tensors(a, false)) return LFD_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_out_split_wide, dim3((unsigned)blocks_for(n, hw)), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), a);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

int out_grad(const void* y, int32_t n, int32_t hw, int64_t points_total, int64_t point0, const lfd_head_out_seg_t* segs,
             int32_t nsegs, float loss_scale, void* dy, void* workspace, size_t workspace_bytes, bool concat, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  Args a{};
  if (!fill(a, y, n, hw, points_total, point0, segs, nsegs, true) || !dy || !workspace || !lfd_aligned16(dy))
    return LFD_ERR_INVALID_ARGUMENT;
  if (concat) { a.y_total = points_total; a.y_point0 = point0; }
  if (workspace_bytes < kLevelPartialFloats * sizeof(float)) return LFD_ERR_WORKSPACE_TOO_SMALL;
  if (!has_tensors(a, true)) return LFD_ERR_INVALID_ARGUMENT;
  a.dy = (__half*)dy; a.loss_scale = loss_scale; a.partials = reinterpret_cast<float*>(workspace);
  const int b = blocks_for(n, hw);
  hipLaunchKernelGGL(k_out_grad_wide, dim3((unsigned)b), dim3(kThreads), 0, st, a);
  LFD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_out_grad_final_wide, dim3(kRows), dim3(128), 0, st, a, b);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

int fill_levels(LevelsArgs& L, const void* y_concat, int32_t n, int64_t points_total, const lfd_head_out_level_t* levels,
                int32_t nlevels, bool backward) {
  if (!levels || nlevels < 1 || nlevels > LFD_MAX_LEVELS) return LFD_ERR_INVALID_ARGUMENT;
  L.nlev = nlevels;
  for (int l = 0; l < nlevels; ++l) {
    if (!fill(L.lv[l], y_concat, n, levels[l].hw, points_total, levels[l].point0, levels[l].segs, levels[l].nsegs, backward))
      return LFD_ERR_INVALID_ARGUMENT;
    L.lv[l].y_total = points_total; L.lv[l].y_point0 = levels[l].point0;
    L.nblocks[l] = blocks_for(n, levels[l].hw);          // the block count of the per-level entry points
  }
  return LFD_OK;
}

}  // namespace

extern "C" {

int lfd_head_out_split_w_f16(const void* y, int32_t n, int32_t hw, int64_t points_total, int64_t point0,
                             const lfd_head_out_seg_t* segs, int32_t nsegs, int32_t rows, lfd_stream_t stream) {
  if (rows == 64) return lfd_head_out_split_f16(y, n, hw, points_total, point0, segs, nsegs, stream);
  if (rows != kRows) return LFD_ERR_INVALID_ARGUMENT;
  return out_split(y, n, hw, points_total, point0, segs, nsegs, false, stream);
}

int lfd_head_out_split_concat_w_f16(const void* y_concat, int32_t n, int32_t hw, int64_t points_total, int64_t point0,
                                    const lfd_head_out_seg_t* segs, int32_t nsegs, int32_t rows, lfd_stream_t stream) {
  if (rows == 64) return lfd_head_out_split_concat_f16(y_concat, n, hw, points_total, point0, segs, nsegs, stream);
  if (rows != kRows) return LFD_ERR_INVALID_ARGUMENT;
  return out_split(y_concat, n, hw, points_total, point0, segs, nsegs, true, stream);
}

int lfd_head_out_grad_w_f16(const void* y, int32_t n, int32_t hw, int64_t points_total, int64_t point0,
                            const lfd_head_out_seg_t* segs, int32_t nsegs, int32_t rows, float loss_scale, void* dy,
                            void* workspace, size_t workspace_bytes, lfd_stream_t stream) {
  if (rows == 64)
    return lfd_head_out_grad_f16(y, n, hw, points_total, point0, segs, nsegs, loss_scale, dy, workspace, workspace_bytes, stream);
  if (rows != kRows) return LFD_ERR_INVALID_ARGUMENT;
  return out_grad(y, n, hw, points_total, point0, segs, nsegs, loss_scale, dy, workspace, workspace_bytes, false, stream);
}

int lfd_head_out_grad_concat_w_f16(const void* y_concat, int32_t n, int32_t hw, int64_t points_total, int64_t point0,
                                   const lfd_head_out_seg_t* segs, int32_t nsegs, int32_t rows, float loss_scale, void* dy_concat,
                                   void* workspace, size_t workspace_bytes, lfd_stream_t stream) {
  if (rows == 64)
    return lfd_head_out_grad_concat_f16(y_concat, n, hw, points_total, point0, segs, nsegs, loss_scale, dy_concat, workspace,
                                        workspace_bytes, stream);
  if (rows != kRows) return LFD_ERR_INVALID_ARGUMENT;
  return out_grad(y_concat, n, hw, points_total, point0, segs, nsegs, loss_scale, dy_concat, workspace, workspace_bytes, true, stream);
}

int lfd_head_out_split_levels_w_f16(const void* y_concat, int32_t n, int64_t points_total, const lfd_head_out_level_t* levels,
                                    int32_t nlevels, int32_t rows, lfd_stream_t stream) {
  if (rows == 64) return lfd_head_out_split_levels_f16(y_concat, n, points_total, levels, nlevels, stream);
  if (rows != kRows) return LFD_ERR_INVALID_ARGUMENT;
  LevelsArgs L{};
  const int rc = fill_levels(L, y_concat, n, points_total, levels, nlevels, false);
  if (rc != LFD_OK) return rc;
  int mx = 1;
  for (int l = 0; l < nlevels; ++l) {
    if (!has_tensors(L.lv[l], false)) return LFD_ERR_INVALID_ARGUMENT;
    if (L.nblocks[l] > mx) mx = L.nblocks[l];
  }
  hipLaunchKernelGGL(k_out_split_levels_wide, dim3((unsigned)mx, (unsigned)nlevels), dim3(kThreads), 0,
                     reinterpret_cast<hipStream_t>(stream), L);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

int lfd_head_out_grad_levels_w_f16(const void* y_concat, int32_t n, int64_t points_total, const lfd_head_out_level_t* levels,
                                   int32_t nlevels, int32_t rows, float loss_scale, void* dy_concat, void* workspace,
                                   size_t workspace_bytes, lfd_stream_t stream) {
  if (rows == 64)
    return lfd_head_out_grad_levels_f16(y_concat, n, points_total, levels, nlevels, loss_scale, dy_concat, workspace, workspace_bytes,
                                        stream);
  if (rows != kRows) return LFD_ERR_INVALID_ARGUMENT;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  LevelsArgs L{};
  const int rc = fill_levels(L, y_concat, n, points_total, levels, nlevels, true);
  if (rc != LFD_OK) return rc;
  if (!dy_concat || !workspace || !lfd_aligned16(dy_concat)) return LFD_ERR_INVALID_ARGUMENT;
  if (workspace_bytes < (size_t)nlevels * kLevelPartialFloats * sizeof(float)) return LFD_ERR_WORKSPACE_TOO_SMALL;
  int mx = 1;
  for (int l = 0; l < nlevels; ++l) {
    Args& a = L.lv[l];
    if (!has_tensors(a, true)) return LFD_ERR_INVALID_ARGUMENT;
    a.dy = (__half*)dy_concat; a.loss_scale = loss_scale;
    a.partials = reinterpret_cast<float*>(workspace) + (size_t)l * kLevelPartialFloats;
    if (L.nblocks[l] > mx) mx = L.nblocks[l];
  }
  hipLaunchKernelGGL(k_out_grad_levels_wide, dim3((unsigned)mx, (unsigned)nlevels), dim3(kThreads), 0, st, L);
  LFD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_out_grad_final_levels_wide, dim3(kRows), dim3(128), 0, st, L);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

}  // extern "C"
