// csrc/train_bn.h -- per-element arithmetic of train-mode BatchNorm's backward (lfd_resnet.py:358-359 `BatchNorm2d` + ReLU),
// shared by k_bn_bwd_apply (train.hip) and the first-conv kernels that apply it on the fly (stem_gray_train.hip), so that
// both produce the same bits.  -ffp-contract=off: every expression is evaluated as written (no fma).
#pragma once
#include "common.h"

// Macros rather than functions: with these three as inline functions the compiler vectorises k_bn_bwd_apply differently (same
// values, different ISA); as macros the expressions are the tokens train.hip always had.
// xhat = (y - mean) * rstd
#define LFD_BN_XHAT(y, mean, rstd) (((y) - (mean)) * (rstd))
// the ReLU behind the BatchNorm passed (mask recomputed from y): gamma * xhat + beta > 0
#define LFD_BN_RELU_OPEN(gamma, beta, xh) ((gamma) * (xh) + (beta) > 0.f)
// dy = a * (g - mean(g) - xhat * mean(g * xhat)), a = gamma * rstd, rounded to fp16
#define LFD_BN_BWD_DY(a, g, mg, xh, mgx) ((_Float16)((a) * ((g) - (mg) - (xh) * (mgx))))

// One 16-byte chunk (8 channels) of dz and y -> dy, ReLU mask recomputed from y (the relu_y mode of k_bn_bwd_apply)
struct LfdBnBwdChunk {
  float mean[8], rstd[8], a[8], mg[8], mgx[8], ga[8], be[8];
};
__device__ __forceinline__ uint4 lfd_bn_bwd_dy_relu_y8(uint4 dz, uint4 y, const LfdBnBwdChunk& p) {
  union { uint4 q; _Float16 h[8]; } d, yy, o;
  d.q = dz;
  yy.q = y;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    float g = (float)d.h[e];
    const float xh = LFD_BN_XHAT((float)yy.h[e], p.mean[e], p.rstd[e]);
    if (!LFD_BN_RELU_OPEN(p.ga[e], p.be[e], xh)) g = 0.f;
    o.h[e] = LFD_BN_BWD_DY(p.a[e], g, p.mg[e], xh, p.mgx[e]);
  }
  return o.q;
}

// Training-workspace layout of the first unit's fused BatchNorm backward + weight gradient (lfd_stem_conv0_bn_bwd_wgrad_rows and
// its gray twin): BatchNorm's partial rows at float 0 (<= 1024 rows x 2 x 256), its final sums [2][c] at kLfdBnSumsAt, the
// weight gradient's own partial rows at kLfdBnWpartAt.
constexpr size_t kLfdBnSumsAt = (size_t)1024 * 2 * 256;
constexpr size_t kLfdBnWpartAt = kLfdBnSumsAt + 2 * 256;

// host (train.hip): the sums stage of that backward -- k_bn_bwd_partial over (dz, y) unless sum_rows > 0 rows are already in
// the workspace (lfd_conv1x1_dgrad_bn_bwd_sums_nhwc_f16), then k_bn_bwd_final: dgamma / dbeta (+)= and the sums at kLfdBnSumsAt.
// No argument checks: the caller's entry point has made them.
int lfd_first_unit_bn_bwd_sums(const void* dz, const void* y, int64_t pixels, int32_t channels, const float* stats,
                               const float* gamma, const float* beta, float inv_scale, int32_t accumulate, int32_t sum_rows,
                               float* workspace, float* dgamma, float* dbeta, hipStream_t st);

// host (train.hip): k_bn_stats_final over `nblocks` rows [2][channels] of per-block sums / sums of squares in the workspace
// (a conv's stat_partials epilogue) -> stats [2][channels] (+ running_mean / running_var update)
int lfd_bn_stats_final_rows(const float* partials, int nblocks, int32_t channels, int64_t pixels, float eps, float momentum,
                            float* running_mean, float* running_var, float* stats, hipStream_t st);
