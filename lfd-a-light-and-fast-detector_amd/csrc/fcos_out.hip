// csrc/fcos_out.hip -- the glue around FCOSHead's OUTPUT convs in a training iteration: all pyramid levels in one launch.
//
// FCOSHead ends, per level, in three 3x3 convs (fcos_head.py:140-150): classification (C rows) and centerness (1 row) on the
// classification tower, regression (4 rows) on the regression tower, the regression output leaving as exp(Scale_i * conv);
// FCOS.forward concatenates the levels along the point axis (fcos.py:414-449).  The training engine runs them as TWO convs
// padded to ROWS output rows with fp32 outputs (lfd_conv2d_nhwc_f16_acc32: the logits stay fp32, so that exp does not amplify an
// fp16 rounding): rows [0, C) classification, row C centerness, the rest zero; rows [0, 4) regression, the rest zero.  This
// file is what sits on both sides of them:
//   forward :  raw_cls / raw_reg [n, hw, ROWS] fp32 of every level  ->  cls[:, p0:p0+hw, :], ctr[:, p0:p0+hw, 0] (copies) and
//              reg[:, p0:p0+hw, :] = expf(raw * scale_i) -- the expression of lfd_pack_level_outputs_f32, bit for bit
//   backward:  dcls / dctr / dreg fp32 (slices of the concatenated gradients), the stored reg and the raw regression rows  ->
//              dy_cls = d * loss_scale, dy_reg = dreg * reg * scale_i * loss_scale [n, hw, ROWS] fp16 (each ONE fp16 rounding
//              of a correctly rounded fp32 value; rows outside the segments ZERO -- they feed the convs' weight and data
//              gradients) and  dbias_cls[c] += sum dcls, dbias_ctr += sum dctr, dbias_reg[k] += sum dreg * reg * scale_i (over
//              ALL levels: shared parameters), dscale_i += sum_k sum dreg * reg * raw (per level)
//              through per-block fp32 partials + one fixed-order fp64 final launch (no atomics: equal bits run after run).
//
// Shape (as csrc/head_out.hip): a thread is a (pixel, 8-row piece) pair; a pixel's fp16 line of dy is ROWS / 8 pieces of 16 B
// written by as many consecutive lanes, the fp32 lines move as float4; the [n, P, C] / [n, P, 1] tensors element by element
// unless C is a multiple of 4 (C + 1 and the point offset break the alignment otherwise); reg / dreg rows are always one float4.
// Piece 0 of a pixel also owns its 4 regression rows.  The piece of a thread is the same in every trip of the grid-stride loop,
// so 8 + 8 sums per thread last the walk.  Partials: kMaxBlocks x 2 x ROWS floats per level; 32-bit pixel / piece indices:
// n * hw * ROWS < 2^31 (refused otherwise).
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;

struct Level {
  const float* raw_cls;   // [n, hw, ROWS]
  const float* raw_reg;   // [n, hw, ROWS]
  const float* scale;     // device scalar
  float* dscale;          // device scalar, +=
  __half* dy_cls;         // [n, hw, ROWS]
  __half* dy_reg;         // [n, hw, ROWS]
  float* partials;        // [nblocks][2][ROWS]
  int hw, nblocks;
  int64_t point0;
};

struct Args {
  Level lv[LFD_MAX_LEVELS];
  int nlev, n, C, vec4;         // vec4: cls / dcls rows may move as float4 (C % 4 == 0, 16-byte aligned)
  int64_t P;
  float* cls;  float* reg;  float* ctr;                               // forward destinations
  const float* dcls;  const float* dreg;  const float* dctr;  const float* regv;   // backward sources (regv: the stored reg)
  float* dbias_cls;  float* dbias_ctr;  float* dbias_reg;
  float loss_scale;
};

union Line8 { uint4 u; _Float16 h[8]; };

template <int ROWS>
__device__ __forceinline__ void pack_body(const Args& A, const Level& L, int bx, int nbx) {
  constexpr int PIECES = ROWS / 8;
  const int piece = threadIdx.x & (PIECES - 1);
  const int C = A.C;
  if (piece * 8 > C && piece != 0) return;          // a piece of padding rows only (no barrier below)
  const float scale = *L.scale;
  const unsigned vecs = (unsigned)A.n * (unsigned)L.hw * PIECES;
  for (unsigned v = (unsigned)bx * kThreads + threadIdx.x; v < vecs; v += (unsigned)nbx * kThreads) {
    const unsigned px = v / PIECES, img = px / (unsigned)L.hw, p = px - img * (unsigned)L.hw;
    const int64_t orow = (int64_t)img * A.P + L.point0 + p;
    if (piece * 8 <= C) {
      const float4* src = reinterpret_cast<const float4*>(L.raw_cls + (int64_t)px * ROWS + piece * 8);
      const float4 a = src[0], b = src[1];
      const float f[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int r0 = piece * 8 + 4 * h;
        if (A.vec4 && r0 + 4 <= C) {
          *reinterpret_cast<float4*>(A.cls + orow * C + r0) = make_float4(f[4 * h], f[4 * h + 1], f[4 * h + 2], f[4 * h + 3]);
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = r0 + e;
            if (r < C) A.cls[orow * C + r] = f[4 * h + e];
            else if (r == C) A.ctr[orow] = f[4 * h + e];
          }
        }
      }
    }
    if (piece == 0) {
      const float4 t = *reinterpret_cast<const float4*>(L.raw_reg + (int64_t)px * ROWS);
      float4 o;          // (as k_pack_level of csrc/sibling.hip: the product, then expf)
      o.x = expf(t.x * scale); o.y = expf(t.y * scale); o.z = expf(t.z * scale); o.w = expf(t.w * scale);
      reinterpret_cast<float4*>(A.reg)[orow] = o;
    }
  }
}

// a product of three fp32 values, rounded to fp32 once
__device__ __forceinline__ float mul3(float a, float b, float c) { return (float)((double)a * (double)b * (double)c); }

template <int ROWS>
__device__ __forceinline__ void grad_body(const Args& A, const Level& L, int bx, int nbx) {
  constexpr int PIECES = ROWS / 8;
  static_assert(kThreads % PIECES == 0 && 2 * ROWS <= kThreads, "a thread keeps its piece; the partials have a thread per slot");
  __shared__ float red[kThreads][17];
  const int piece = threadIdx.x & (PIECES - 1);
  const int C = A.C;
  const float scale = *L.scale, ls = A.loss_scale;
  float acc_c[8], acc_r[8];          // acc_c: my 8 rows of the classification conv; acc_r (piece 0): dbias_reg[0..3], dscale terms [4..7]
  for (int e = 0; e < 8; ++e) acc_c[e] = acc_r[e] = 0.f;
  const unsigned vecs = (unsigned)A.n * (unsigned)L.hw * PIECES;
  for (unsigned v = (unsigned)bx * kThreads + threadIdx.x; v < vecs; v += (unsigned)nbx * kThreads) {
    const unsigned px = v / PIECES, img = px / (unsigned)L.hw, p = px - img * (unsigned)L.hw;
    const int64_t grow = (int64_t)img * A.P + L.point0 + p;
    Line8 oc, orr;
    oc.u = make_uint4(0, 0, 0, 0);          // rows outside the segments leave as zero
    orr.u = make_uint4(0, 0, 0, 0);
    if (piece * 8 <= C) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int r0 = piece * 8 + 4 * h;
        float d4[4] = {0.f, 0.f, 0.f, 0.f};
        bool live[4] = {false, false, false, false};
        if (A.vec4 && r0 + 4 <= C) {
          const float4 t = *reinterpret_cast<const float4*>(A.dcls + grow * C + r0);
          d4[0] = t.x; d4[1] = t.y; d4[2] = t.z; d4[3] = t.w;
          live[0] = live[1] = live[2] = live[3] = true;
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int r = r0 + e;
            if (r < C) { d4[e] = A.dcls[grow * C + r]; live[e] = true; }
            else if (r == C) { d4[e] = A.dctr[grow]; live[e] = true; }
          }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (!live[e]) continue;
          acc_c[4 * h + e] += d4[e];
          oc.h[4 * h + e] = (_Float16)(d4[e] * ls);
        }
      }
    }
    if (piece == 0) {
      const float4 d = reinterpret_cast<const float4*>(A.dreg)[grow], g = reinterpret_cast<const float4*>(A.regv)[grow];
      const float4 w = *reinterpret_cast<const float4*>(L.raw_reg + (int64_t)px * ROWS);
      const float dd[4] = {d.x, d.y, d.z, d.w}, gg[4] = {g.x, g.y, g.z, g.w}, ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float t = mul3(dd[k], gg[k], scale);          // dL/d(raw regression row)
        acc_r[k] += t;
        acc_r[4 + k] += mul3(dd[k], gg[k], ww[k]);           // dL/dscale
        orr.h[k] = (_Float16)(t * ls);
      }
    }
    reinterpret_cast<uint4*>(L.dy_cls)[(int64_t)px * PIECES + piece] = oc.u;
    reinterpret_cast<uint4*>(L.dy_reg)[(int64_t)px * PIECES + piece] = orr.u;
  }
  for (int e = 0; e < 8; ++e) { red[threadIdx.x][e] = acc_c[e]; red[threadIdx.x][8 + e] = acc_r[e]; }
  __syncthreads();
  // slot (q, r) of the block's partial row: the sum over the threads whose piece holds row r, in thread order
  if (threadIdx.x < 2 * ROWS) {
    const int q = threadIdx.x / ROWS, r = threadIdx.x % ROWS;
    float s = 0.f;
    for (int t = r >> 3; t < kThreads; t += PIECES) s += red[t][q * 8 + (r & 7)];
    L.partials[((size_t)bx * 2 + q) * ROWS + r] = s;
  }
}

__device__ __forceinline__ double wave_sum(double v) {
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// sum over a level's block partials of quantity q, slot r: lanes stride over the partial rows; the order depends on nblocks alone
template <int ROWS>
__device__ __forceinline__ double column_sum(const float* partials, int nblocks, int q, int r) {
  double s = 0.0;
  for (int b = threadIdx.x & 63; b < nblocks; b += 64) s += (double)partials[((size_t)b * 2 + q) * ROWS + r];
  return wave_sum(s);
}

template <int ROWS> __global__ __launch_bounds__(kThreads) void k_fcos_pack(Args A) {
  const Level& L = A.lv[blockIdx.y];
  if ((int)blockIdx.x < L.nblocks) pack_body<ROWS>(A, L, blockIdx.x, L.nblocks);
}

template <int ROWS> __global__ __launch_bounds__(kThreads) void k_fcos_grad(Args A) {
  const Level& L = A.lv[blockIdx.y];
  if ((int)blockIdx.x < L.nblocks) grad_body<ROWS>(A, L, blockIdx.x, L.nblocks);
}

// block = row r.  Wave 0: the row of the classification conv over all levels in level order (r < C: dbias_cls[r], r == C:
// dbias_ctr).  Wave 1: r < 4: dbias_reg[r] over all levels; r < nlev: dscale of level r over its 4 rows.
template <int ROWS> __global__ __launch_bounds__(128) void k_fcos_grad_final(Args A) {
  const int wave = threadIdx.x >> 6, r = blockIdx.x;
  const bool lane0 = (threadIdx.x & 63) == 0;
  if (wave == 0) {
    if (r > A.C) return;
    double s = 0.0;
    for (int l = 0; l < A.nlev; ++l) s += column_sum<ROWS>(A.lv[l].partials, A.lv[l].nblocks, 0, r);
    if (lane0) {
      if (r < A.C) A.dbias_cls[r] += (float)s;
      else A.dbias_ctr[0] += (float)s;
    }
  } else {
    if (r < 4) {
      double s = 0.0;
      for (int l = 0; l < A.nlev; ++l) s += column_sum<ROWS>(A.lv[l].partials, A.lv[l].nblocks, 1, r);
      if (lane0) A.dbias_reg[r] += (float)s;
    }
    if (r < A.nlev) {
      double t = 0.0;
      for (int k = 0; k < 4; ++k) t += column_sum<ROWS>(A.lv[r].partials, A.lv[r].nblocks, 1, 4 + k);
      if (lane0) *A.lv[r].dscale += (float)t;
    }
  }
}

template <int ROWS> constexpr size_t kLevelPartialFloats = (size_t)kMaxBlocks * 2 * ROWS;

// -> LFD_OK and mx = the largest block count of a level (the launch's grid.x)
template <int ROWS>
int fill(Args& A, int& mx, const lfd_fcos_out_level_t* levels, int32_t nlevels, int32_t n, int32_t num_classes, int64_t points_total,
         bool backward) {
  if (!levels || nlevels < 1 || n < 1 || num_classes < 1 || points_total < 1) return LFD_ERR_INVALID_ARGUMENT;
  if (nlevels > LFD_MAX_LEVELS || num_classes + 1 > ROWS) return LFD_ERR_INVALID_ARGUMENT;
  A.nlev = nlevels; A.n = n; A.C = num_classes; A.P = points_total;
  mx = 1;
  for (int l = 0; l < nlevels; ++l) {
    const lfd_fcos_out_level_t& s = levels[l];
    Level& L = A.lv[l];
    if (!s.raw_reg || !s.scale || !lfd_aligned16(s.raw_reg) || s.hw < 1 || s.point0 < 0 || s.point0 + s.hw > points_total)
      return LFD_ERR_INVALID_ARGUMENT;
    if (!backward && (!s.raw_cls || !lfd_aligned16(s.raw_cls))) return LFD_ERR_INVALID_ARGUMENT;
    if (backward && (!s.dscale || !s.dy_cls || !s.dy_reg || !lfd_aligned16(s.dy_cls) || !lfd_aligned16(s.dy_reg)))
      return LFD_ERR_INVALID_ARGUMENT;
    if ((int64_t)n * s.hw * ROWS >= ((int64_t)1 << 31)) return LFD_ERR_UNSUPPORTED;      // 32-bit pixel / piece indices
    L.raw_cls = s.raw_cls; L.raw_reg = s.raw_reg; L.scale = s.scale; L.dscale = s.dscale;
    L.dy_cls = (__half*)s.dy_cls; L.dy_reg = (__half*)s.dy_reg; L.hw = s.hw; L.point0 = s.point0;
    const int64_t b = ((int64_t)n * s.hw * (ROWS / 8) + kThreads - 1) / kThreads;
    L.nblocks = (int)(b > kMaxBlocks ? kMaxBlocks : b);
    if (L.nblocks > mx) mx = L.nblocks;
  }
  return LFD_OK;
}

template <int ROWS>
int pack_levels(const lfd_fcos_out_level_t* levels, int32_t nlevels, int32_t n, int32_t num_classes, int64_t points_total, float* cls,
                float* reg, float* ctr, lfd_stream_t stream) {
  Args A{};
  int mx;
  if (!cls || !reg || !ctr || !lfd_aligned16(reg)) return LFD_ERR_INVALID_ARGUMENT;
  const int rc = fill<ROWS>(A, mx, levels, nlevels, n, num_classes, points_total, false);
  if (rc != LFD_OK) return rc;
  A.cls = cls; A.reg = reg; A.ctr = ctr;
  A.vec4 = (num_classes % 4 == 0 && lfd_aligned16(cls)) ? 1 : 0;
  hipLaunchKernelGGL(k_fcos_pack<ROWS>, dim3((unsigned)mx, (unsigned)nlevels), dim3(kThreads), 0, reinterpret_cast<hipStream_t>(stream), A);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

template <int ROWS>
int grad_levels(const lfd_fcos_out_level_t* levels, int32_t nlevels, int32_t n, int32_t num_classes, int64_t points_total,
                const float* dcls, const float* dreg, const float* dctr, const float* reg, float loss_scale, float* dbias_cls,
                float* dbias_ctr, float* dbias_reg, void* workspace, size_t workspace_bytes, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  Args A{};
  int mx;
  if (!dcls || !dreg || !dctr || !reg || !dbias_cls || !dbias_ctr || !dbias_reg || !workspace || !lfd_aligned16(dreg) ||
      !lfd_aligned16(reg) || !lfd_aligned16(workspace))
    return LFD_ERR_INVALID_ARGUMENT;
  const int rc = fill<ROWS>(A, mx, levels, nlevels, n, num_classes, points_total, true);
  if (rc != LFD_OK) return rc;
  if (workspace_bytes < (size_t)nlevels * kLevelPartialFloats<ROWS> * sizeof(float)) return LFD_ERR_WORKSPACE_TOO_SMALL;
  for (int l = 0; l < nlevels; ++l) A.lv[l].partials = reinterpret_cast<float*>(workspace) + (size_t)l * kLevelPartialFloats<ROWS>;
  A.dcls = dcls; A.dreg = dreg; A.dctr = dctr; A.regv = reg; A.loss_scale = loss_scale;
  A.dbias_cls = dbias_cls; A.dbias_ctr = dbias_ctr; A.dbias_reg = dbias_reg;
  A.vec4 = (num_classes % 4 == 0 && lfd_aligned16(dcls)) ? 1 : 0;
  hipLaunchKernelGGL(k_fcos_grad<ROWS>, dim3((unsigned)mx, (unsigned)nlevels), dim3(kThreads), 0, st, A);
  LFD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_fcos_grad_final<ROWS>, dim3(ROWS), dim3(128), 0, st, A);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

}  // namespace

extern "C" {

size_t lfd_fcos_out_grad_workspace_bytes(int32_t nlevels, int32_t rows) {
  if (nlevels < 1 || nlevels > LFD_MAX_LEVELS || (rows != 32 && rows != 64)) return 0;
  return (size_t)nlevels * kMaxBlocks * 2 * rows * sizeof(float);
}

int lfd_fcos_out_pack_levels_f32(const lfd_fcos_out_level_t* levels, int32_t nlevels, int32_t n, int32_t rows, int32_t num_classes,
                                 int64_t points_total, float* cls, float* reg, float* ctr, lfd_stream_t stream) {
  switch (rows) {
    case 32: return pack_levels<32>(levels, nlevels, n, num_classes, points_total, cls, reg, ctr, stream);
    case 64: return pack_levels<64>(levels, nlevels, n, num_classes, points_total, cls, reg, ctr, stream);
    default: return LFD_ERR_INVALID_ARGUMENT;
  }
}

int lfd_fcos_out_grad_levels_f32(const lfd_fcos_out_level_t* levels, int32_t nlevels, int32_t n, int32_t rows, int32_t num_classes,
                                 int64_t points_total, const float* dcls, const float* dreg, const float* dctr, const float* reg,
                                 float loss_scale, float* dbias_cls, float* dbias_ctr, float* dbias_reg, void* workspace,
                                 size_t workspace_bytes, lfd_stream_t stream) {
  switch (rows) {
    case 32:
      return grad_levels<32>(levels, nlevels, n, num_classes, points_total, dcls, dreg, dctr, reg, loss_scale, dbias_cls, dbias_ctr,
                             dbias_reg, workspace, workspace_bytes, stream);
    case 64:
      return grad_levels<64>(levels, nlevels, n, num_classes, points_total, dcls, dreg, dctr, reg, loss_scale, dbias_cls, dbias_ctr,
                             dbias_reg, workspace, workspace_bytes, stream);
    default: return LFD_ERR_INVALID_ARGUMENT;
  }
}

}  // extern "C"
