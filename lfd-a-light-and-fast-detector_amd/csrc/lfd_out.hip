// csrc/lfd_out.hip -- the glue around LFDHead's OUTPUT convs with fp32 logits in a training iteration: all pyramid levels and
// both output convs of a level in one launch.
//
// LFDHead ends, per level, in a classification conv1x1 (C' rows) and a regression conv1x1 (4 rows), the regression output
// through the level's learnable Scale where the regression loss is of the IoU family (lfd_head.py:157-185); LFD.forward
// concatenates the levels along the point axis (lfd.py:526-542).  The detector node runs them as ONE conv (both read the same
// activation: merged path, or no tower layers) or TWO convs (separate towers) padded to ROWS output rows with fp32 outputs
// (lfd_conv2d_nhwc_f16_acc32).  A SEGMENT is the row range [row0, row0 + channels) of one of the reference's convs inside
// such a padded conv; a level has exactly one classification and one regression segment.  This file sits on both sides:
//   forward :  raw [n, hw, ROWS] fp32 of every conv of every level  ->  cls[:, p0:p0+hw, :] = the classification rows (a copy),
//              reg[:, p0:p0+hw, :] = fl32(raw * scale_i) (one fp32 multiply; a copy without a Scale)
//   backward:  dcls / dreg fp32 (the concatenated gradients)  ->  dy [n, hw, ROWS] fp16 of every conv: dcls * loss_scale and
//              dreg * scale_i * loss_scale (formed in fp64, rounded to fp32 once, then to fp16 once) in the segments' rows, ZERO
//              elsewhere (the rows feed the convs' weight and data gradients), and  dbias[j] += sum dcls | sum dreg * scale_i over
//              ALL levels that name the same target,  dscale_i += sum_k sum dreg * raw  per level, through per-block fp32 partials
//              + one fixed-order fp64 final launch (no atomics: equal bits run after run).
//
// Shape (as csrc/fcos_out.hip): a thread is a (pixel, conv, 8-row piece) triple; a pixel's fp16 line of dy is ROWS / 8 pieces of
// 16 B written by as many consecutive lanes (the forward walks only the leading pieces that hold segment rows, rounded up to a
// power of two), the raw fp32 lines are read as float4; the [n, P, C'] / [n, P, 4] tensors move as
// float4 where a segment's first row and channel count are multiples of 4 (then a 4-row half piece lies wholly inside or outside
// the segment and every address is 16-byte aligned), element by element otherwise.  256 % (convs x pieces) == 0, so the (conv,
// piece) of a thread is the same in every trip of the grid-stride loop and 8 + 8 sums per thread last the walk.  Partials:
// kMaxBlocks x 2 convs x 2 x ROWS floats per level; 32-bit pixel / piece indices: n * hw * ROWS < 2^31 (refused otherwise).
#include <algorithm>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;

struct Seg {
  float* dbias;           // [ch], +=
  int row0, ch, kind;     // kind 0: classification, 1: regression
  int vec;                // the segment's rows move as float4
};

struct Conv {
  const float* raw;       // [n, hw, ROWS]
  __half* dy;             // [n, hw, ROWS]
  Seg s[2];
  int nsegs, pad;
};

struct Level {
  const float* scale;     // device scalar or null
  float* dscale;          // device scalar, +=
  float* partials;        // [nblocks][nconvs][2][ROWS]
  int64_t point0;
  int hw, nblocks, nconvs;
  int lp;                 // pack: pieces per conv that the walk covers (a power of two; the pieces behind it are padding rows only)
  Conv c[2];
};

struct Args {
  Level lv[LFD_MAX_LEVELS];
  int nlev, n, C, pad;
  int64_t P;
  float* cls;  float* reg;                  // forward destinations
  const float* dcls;  const float* dreg;    // backward sources
  float loss_scale;
};

union Line8 { uint4 u; _Float16 h[8]; };

// What a thread keeps in registers for its walk (the kernel arguments are read once, before the loop): per row of its 8-row
// piece the kind of the segment it lies in (-1: a padding row) and its column in cls / reg, per 4-row half whether it moves as a
// float4 (then the half lies wholly inside one segment).
struct Piece {
  int kind[8], col[8];
  bool vec[2], any;
};

__device__ __forceinline__ Piece rows_of_piece(const Conv& cv, int piece) {
  const int nsegs = cv.nsegs;
  int row0[2], ch[2], kd[2], vc[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) { row0[s] = cv.s[s].row0; ch[s] = s < nsegs ? cv.s[s].ch : 0; kd[s] = cv.s[s].kind; vc[s] = cv.s[s].vec; }
  Piece P;
  P.any = false;
  P.vec[0] = P.vec[1] = false;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int r = piece * 8 + e;
    P.kind[e] = -1;
    P.col[e] = 0;
#pragma unroll
    for (int s = 0; s < 2; ++s)
      if (r >= row0[s] && r < row0[s] + ch[s]) {
        P.kind[e] = kd[s];
        P.col[e] = r - row0[s];
        if ((e & 3) == 0) P.vec[e >> 2] = vc[s] != 0;
      }
    P.any = P.any || P.kind[e] >= 0;
  }
  return P;
}

template <int ROWS>
__device__ __forceinline__ void pack_body(const Args& A, const Level& L, int bx, int nbx) {
  const int lp = L.lp, slots = L.nconvs * lp;          // (256 % slots == 0: a thread keeps its (conv, piece))
  const int slot = threadIdx.x % slots, ci = slot / lp, piece = slot - ci * lp;
  const Piece P = rows_of_piece(L.c[ci], piece);
  if (!P.any) return;          // a piece of padding rows only (no barrier below)
  const float* raw = L.c[ci].raw + piece * 8;
  const bool scaled = L.scale != nullptr;
  const float scale = scaled ? *L.scale : 1.f;
  float* const cls = A.cls;
  float* const reg = A.reg;
  const int C = A.C, hw = L.hw;
  const int64_t row_of_img = A.P, point0 = L.point0;
  const unsigned vecs = (unsigned)A.n * (unsigned)hw * (unsigned)slots;
  for (unsigned v = (unsigned)bx * kThreads + threadIdx.x; v < vecs; v += (unsigned)nbx * kThreads) {
    const unsigned px = v / (unsigned)slots, img = px / (unsigned)hw, p = px - img * (unsigned)hw;
    const int64_t orow = (int64_t)img * row_of_img + point0 + p;
    const float4* src = reinterpret_cast<const float4*>(raw + (int64_t)px * ROWS);
    const float4 a = src[0], b = src[1];
    const float f[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (P.vec[h]) {          // (row0 and ch multiples of 4: the half piece lies wholly inside the segment)
        const bool mul = P.kind[4 * h] == 1 && scaled;
        float4 o;
        o.x = mul ? f[4 * h] * scale : f[4 * h];
        o.y = mul ? f[4 * h + 1] * scale : f[4 * h + 1];
        o.z = mul ? f[4 * h + 2] * scale : f[4 * h + 2];
        o.w = mul ? f[4 * h + 3] * scale : f[4 * h + 3];
        float* dst = P.kind[4 * h] == 0 ? cls + orow * C : reg + orow * 4;
        *reinterpret_cast<float4*>(dst + P.col[4 * h]) = o;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = P.kind[4 * h + e];
          if (k < 0) continue;
          if (k == 0) cls[orow * C + P.col[4 * h + e]] = f[4 * h + e];
          else reg[orow * 4 + P.col[4 * h + e]] = scaled ? f[4 * h + e] * scale : f[4 * h + e];
        }
      }
    }
  }
}

template <int ROWS>
__device__ __forceinline__ void grad_body(const Args& A, const Level& L, int bx, int nbx) {
  constexpr int PIECES = ROWS / 8;
  static_assert(kThreads % (2 * PIECES) == 0, "a thread keeps its (conv, piece)");
  __shared__ float red[kThreads][17];
  const int slots = L.nconvs * PIECES;
  const int slot = threadIdx.x % slots, ci = slot / PIECES, piece = slot - ci * PIECES;
  const Piece P = rows_of_piece(L.c[ci], piece);
  const bool scaled = L.scale != nullptr;
  const double scale = scaled ? (double)*L.scale : 1.0, ls = (double)A.loss_scale;
  bool need_raw = false;          // my piece holds regression rows of a level with a Scale: the dscale terms read raw
#pragma unroll
  for (int e = 0; e < 8; ++e) need_raw = need_raw || (P.kind[e] == 1 && scaled);
  const float* raw = L.c[ci].raw + piece * 8;
  uint4* const dy = reinterpret_cast<uint4*>(L.c[ci].dy) + piece;
  const float* const dcls = A.dcls;
  const float* const dreg = A.dreg;
  const int C = A.C, hw = L.hw;
  const int64_t row_of_img = A.P, point0 = L.point0;
  float acc_b[8], acc_s[8];       // per row of my piece: the bias gradient's sum, the Scale gradient's sum
  for (int e = 0; e < 8; ++e) acc_b[e] = acc_s[e] = 0.f;
  const unsigned vecs = (unsigned)A.n * (unsigned)hw * (unsigned)slots;
  for (unsigned v = (unsigned)bx * kThreads + threadIdx.x; v < vecs; v += (unsigned)nbx * kThreads) {
    const unsigned px = v / (unsigned)slots, img = px / (unsigned)hw, p = px - img * (unsigned)hw;
    const int64_t grow = (int64_t)img * row_of_img + point0 + p;
    Line8 o;
    o.u = make_uint4(0, 0, 0, 0);          // rows outside the segments leave as zero
    if (P.any) {
      float w[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (need_raw) {
        const float4* src = reinterpret_cast<const float4*>(raw + (int64_t)px * ROWS);
        const float4 a = src[0], b = src[1];
        w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w; w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float d4[4] = {0.f, 0.f, 0.f, 0.f};
        if (P.vec[h]) {
          const float* src = P.kind[4 * h] == 0 ? dcls + grow * C : dreg + grow * 4;
          const float4 t = *reinterpret_cast<const float4*>(src + P.col[4 * h]);
          d4[0] = t.x; d4[1] = t.y; d4[2] = t.z; d4[3] = t.w;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int k = P.kind[4 * h + e];
            if (k < 0) continue;
            d4[e] = k == 0 ? dcls[grow * C + P.col[4 * h + e]] : dreg[grow * 4 + P.col[4 * h + e]];
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int k = P.kind[4 * h + e];
          if (k < 0) continue;
          const float d = d4[e];
          if (k == 1 && scaled) {
            acc_b[4 * h + e] += (float)((double)d * scale);                       // dL/d(raw regression row)
            acc_s[4 * h + e] += (float)((double)d * (double)w[4 * h + e]);        // dL/dscale
            o.h[4 * h + e] = (_Float16)(float)((double)d * scale * ls);
          } else {
            acc_b[4 * h + e] += d;
            o.h[4 * h + e] = (_Float16)(float)((double)d * ls);
          }
        }
      }
    }
    dy[(int64_t)px * PIECES] = o.u;
  }
  for (int e = 0; e < 8; ++e) { red[threadIdx.x][e] = acc_b[e]; red[threadIdx.x][8 + e] = acc_s[e]; }
  __syncthreads();
  // slot (conv c, quantity q, row r) of the block's partial row: the sum over the threads that hold (c, r's piece), in thread order
  for (int k = threadIdx.x; k < L.nconvs * 2 * ROWS; k += kThreads) {
    const int c = k / (2 * ROWS), q = (k / ROWS) & 1, r = k % ROWS;
    float s = 0.f;
    for (int t = c * PIECES + (r >> 3); t < kThreads; t += slots) s += red[t][q * 8 + (r & 7)];
    L.partials[(size_t)bx * (L.nconvs * 2 * ROWS) + k] = s;
  }
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// sum over a level's block partials of conv c, quantity q, row r: lanes stride over the partial rows; the order depends on
// nblocks alone
template <int ROWS>
__device__ __forceinline__ double column_sum(const Level& L, int c, int q, int r) {
  double s = 0.0;
  for (int b = threadIdx.x & 63; b < L.nblocks; b += 64)
    s += (double)L.partials[(size_t)b * (L.nconvs * 2 * ROWS) + (size_t)(c * 2 + q) * ROWS + r];
  return wave_sum(s);
}

template <int ROWS> __global__ __launch_bounds__(kThreads) void k_lfd_out_pack(Args A) {
  const Level& L = A.lv[blockIdx.y];
  if ((int)blockIdx.x < L.nblocks) pack_body<ROWS>(A, L, blockIdx.x, L.nblocks);
}

template <int ROWS> __global__ __launch_bounds__(kThreads) void k_lfd_out_grad(Args A) {
  const Level& L = A.lv[blockIdx.y];
  if ((int)blockIdx.x < L.nblocks) grad_body<ROWS>(A, L, blockIdx.x, L.nblocks);
}

// One wave per block.  blockIdx.y < 2: row r = blockIdx.x of conv slot blockIdx.y, the levels in level order: the sums of
// consecutive levels that name the same bias element are added in fp64 and reach it with one rounding.  blockIdx.y == 2: the
// Scale gradient of level blockIdx.x over its 4 regression rows.  Nothing else writes these targets, so no two blocks meet.
template <int ROWS> __global__ __launch_bounds__(64) void k_lfd_out_grad_final(Args A) {
  const bool lane0 = (threadIdx.x & 63) == 0;
  if (blockIdx.y == 2) {
    const int l = blockIdx.x;
    if (l >= A.nlev || A.lv[l].scale == nullptr) return;
    const Level& L = A.lv[l];
    for (int c = 0; c < L.nconvs; ++c)
      for (int s = 0; s < L.c[c].nsegs; ++s) {
        const Seg& S = L.c[c].s[s];
        if (S.kind != 1) continue;
        double t = 0.0;
        for (int k = 0; k < S.ch; ++k) t += column_sum<ROWS>(L, c, 1, S.row0 + k);
        if (lane0) *L.dscale += (float)t;
      }
    return;
  }
  const int c = blockIdx.y, r = blockIdx.x;
  float* cur = nullptr;
  double sum = 0.0;
  for (int l = 0; l < A.nlev; ++l) {
    const Level& L = A.lv[l];
    float* tgt = nullptr;
    if (c < L.nconvs)
      for (int s = 0; s < L.c[c].nsegs; ++s) {
        const Seg& S = L.c[c].s[s];
        if (r >= S.row0 && r < S.row0 + S.ch) tgt = S.dbias + (r - S.row0);
      }
    if (tgt != cur) {
      if (cur != nullptr && lane0) *cur += (float)sum;
      cur = tgt;
      sum = 0.0;
    }
    if (tgt != nullptr) sum += column_sum<ROWS>(L, c, 0, r);
  }
  if (cur != nullptr && lane0) *cur += (float)sum;
}

template <int ROWS> constexpr size_t kLevelPartialFloats = (size_t)kMaxBlocks * 2 * 2 * ROWS;

// -> LFD_OK and mx = the largest block count of a level (the launch's grid.x)
template <int ROWS>
int fill(Args& A, int& mx, const lfd_lfdhead_out_level_t* levels, int32_t nlevels, int32_t n, int32_t cls_channels,
         int64_t points_total, const float* fcls, const float* freg, bool backward) {
  if (!levels || nlevels < 1 || nlevels > LFD_MAX_LEVELS || n < 1 || cls_channels < 1 || points_total < 1) return LFD_ERR_INVALID_ARGUMENT;
  A.nlev = nlevels; A.n = n; A.C = cls_channels; A.P = points_total;
  mx = 1;
  for (int l = 0; l < nlevels; ++l) {
    const lfd_lfdhead_out_level_t& s = levels[l];
    Level& L = A.lv[l];
    if (s.hw < 1 || s.point0 < 0 || s.point0 + s.hw > points_total || s.nconvs < 1 || s.nconvs > 2) return LFD_ERR_INVALID_ARGUMENT;
    if (backward && ((s.scale != nullptr) != (s.dscale != nullptr))) return LFD_ERR_INVALID_ARGUMENT;
    int kinds[2] = {0, 0};
    for (int c = 0; c < s.nconvs; ++c) {
      const lfd_lfdhead_out_conv_t& sc = s.convs[c];
      Conv& D = L.c[c];
      if (sc.nsegs < 1 || sc.nsegs > 2 || (sc.raw && !lfd_aligned16(sc.raw))) return LFD_ERR_INVALID_ARGUMENT;
      if (backward && (!sc.dy || !lfd_aligned16(sc.dy))) return LFD_ERR_INVALID_ARGUMENT;
      D.raw = sc.raw; D.dy = (__half*)sc.dy; D.nsegs = sc.nsegs;
      for (int k = 0; k < sc.nsegs; ++k) {
        const lfd_lfdhead_out_seg_t& g = sc.segs[k];
        if (g.kind < 0 || g.kind > 1 || g.row0 < 0 || g.channels < 1 || g.row0 + g.channels > ROWS) return LFD_ERR_INVALID_ARGUMENT;
        if (g.channels != (g.kind == 0 ? cls_channels : 4) || (backward && !g.dbias)) return LFD_ERR_INVALID_ARGUMENT;
        if (k == 1 && g.row0 < sc.segs[0].row0 + sc.segs[0].channels && sc.segs[0].row0 < g.row0 + g.channels)
          return LFD_ERR_INVALID_ARGUMENT;          // overlapping segments
        ++kinds[g.kind];
        Seg& S = D.s[k];
        S.dbias = g.dbias; S.row0 = g.row0; S.ch = g.channels; S.kind = g.kind;
        S.vec = (g.row0 % 4 == 0 && g.channels % 4 == 0 && lfd_aligned16(g.kind == 0 ? fcls : freg)) ? 1 : 0;
        // the backward reads raw for the Scale gradient alone: the conv that holds the regression rows of a level with a Scale
        if (!sc.raw && (!backward || (g.kind == 1 && s.scale))) return LFD_ERR_INVALID_ARGUMENT;
      }
    }
    if (kinds[0] != 1 || kinds[1] != 1) return LFD_ERR_INVALID_ARGUMENT;      // one classification and one regression segment
    if ((int64_t)n * s.hw * ROWS >= ((int64_t)1 << 31)) return LFD_ERR_UNSUPPORTED;      // 32-bit pixel / piece indices
    L.scale = s.scale; L.dscale = s.dscale; L.hw = s.hw; L.point0 = s.point0; L.nconvs = s.nconvs;
    int last = 1;          // one past the last row of a segment
    for (int c = 0; c < s.nconvs; ++c)
      for (int k = 0; k < s.convs[c].nsegs; ++k) last = std::max(last, s.convs[c].segs[k].row0 + s.convs[c].segs[k].channels);
    L.lp = 1;
    while (L.lp * 8 < last) L.lp *= 2;
    // the backward writes every piece of dy (the padding rows as zeros), the forward walks the pieces that hold segment rows
    const int64_t b = ((int64_t)n * s.hw * s.nconvs * (backward ? ROWS / 8 : L.lp) + kThreads - 1) / kThreads;
    L.nblocks = (int)(b > kMaxBlocks ? kMaxBlocks : b);
    if (L.nblocks > mx) mx = L.nblocks;
  }
  return LFD_OK;
}

template <int ROWS>
int pack_levels(const lfd_lfdhead_out_level_t* levels, int32_t nlevels, int32_t n, int32_t cls_channels, int64_t points_total,
                float* cls, float* reg, lfd_stream_t stream) {
  Args A{};
  int mx;
  if (!cls || !reg || !lfd_aligned16(reg)) return LFD_ERR_INVALID_ARGUMENT;
  const int rc = fill<ROWS>(A, mx, levels, nlevels, n, cls_channels, points_total, cls, reg, false);
  if (rc != LFD_OK) return rc;
  A.cls = cls; A.reg = reg;
  hipLaunchKernelGGL(k_lfd_out_pack<ROWS>, dim3((unsigned)mx, (unsigned)nlevels), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), A);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

template <int ROWS>
int grad_levels(const lfd_lfdhead_out_level_t* levels, int32_t nlevels, int32_t n, int32_t cls_channels, int64_t points_total,
                const float* dcls, const float* dreg, float loss_scale, void* workspace, size_t workspace_bytes, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  Args A{};
  int mx;
  if (!dcls || !dreg || !workspace || !lfd_aligned16(dreg) || !lfd_aligned16(workspace)) return LFD_ERR_INVALID_ARGUMENT;
  const int rc = fill<ROWS>(A, mx, levels, nlevels, n, cls_channels, points_total, dcls, dreg, true);
  if (rc != LFD_OK) return rc;
  if (workspace_bytes < (size_t)nlevels * kLevelPartialFloats<ROWS> * sizeof(float)) return LFD_ERR_WORKSPACE_TOO_SMALL;
  for (int l = 0; l < nlevels; ++l) A.lv[l].partials = reinterpret_cast<float*>(workspace) + (size_t)l * kLevelPartialFloats<ROWS>;
  A.dcls = dcls; A.dreg = dreg; A.loss_scale = loss_scale;
  hipLaunchKernelGGL(k_lfd_out_grad<ROWS>, dim3((unsigned)mx, (unsigned)nlevels), dim3(kThreads), 0, st, A);
  LFD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_lfd_out_grad_final<ROWS>, dim3(ROWS, 3), dim3(64), 0, st, A);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

}  // namespace

extern "C" {

size_t lfd_lfdhead_out_grad_workspace_bytes(int32_t nlevels, int32_t rows) {
  if (nlevels < 1 || nlevels > LFD_MAX_LEVELS || (rows != 64 && rows != 128)) return 0;
  return (size_t)nlevels * kMaxBlocks * 2 * 2 * rows * sizeof(float);
}

int lfd_lfdhead_out_pack_levels_f32(const lfd_lfdhead_out_level_t* levels, int32_t nlevels, int32_t n, int32_t rows,
                                    int32_t cls_channels, int64_t points_total, float* cls, float* reg, lfd_stream_t stream) {
  switch (rows) {
    case 64: return pack_levels<64>(levels, nlevels, n, cls_channels, points_total, cls, reg, stream);
    case 128: return pack_levels<128>(levels, nlevels, n, cls_channels, points_total, cls, reg, stream);
    default: return LFD_ERR_INVALID_ARGUMENT;
  }
}

int lfd_lfdhead_out_grad_levels_f32(const lfd_lfdhead_out_level_t* levels, int32_t nlevels, int32_t n, int32_t rows,
                                    int32_t cls_channels, int64_t points_total, const float* dcls, const float* dreg,
                                    float loss_scale, void* workspace, size_t workspace_bytes, lfd_stream_t stream) {
  switch (rows) {
    case 64:
      return grad_levels<64>(levels, nlevels, n, cls_channels, points_total, dcls, dreg, loss_scale, workspace, workspace_bytes, stream);
    case 128:
      return grad_levels<128>(levels, nlevels, n, cls_channels, points_total, dcls, dreg, loss_scale, workspace, workspace_bytes, stream);
    default: return LFD_ERR_INVALID_ARGUMENT;
  }
}

}  // extern "C"
