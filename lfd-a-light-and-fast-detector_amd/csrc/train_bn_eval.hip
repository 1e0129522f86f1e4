// csrc/train_bn_eval.hip -- eval-mode BatchNorm inside a TRAINING iteration: fine-tuning with frozen stages and / or
// norm_eval=True (lfd_resnet.py:476-509: frozen stages run in eval(), norm_eval puts every backbone BatchNorm2d in eval()).
//
//   running statistics -> (mean, rstd) rows     lfd_bn_eval_stats_f32       one launch for every eval-mode norm of the network
//   conv + eval norm folded (frozen units)      lfd_conv_bn_eval_fold_f32   w' = w * gamma * rstd, b' = beta - mean * gamma * rstd
//   backward of an eval-mode norm (+ ReLU)      lfd_bn_eval_bwd_f16         ONE pass over (dz, y): dy = gamma * rstd * g
//
// An eval-mode norm normalises with constants, so dy does not depend on the sums over the batch: where the training backward
// (train.hip, lfd_bn_train_bwd_f16) reads dz and y twice -- sums, then apply -- this one reads them once, writes dy and leaves
// the per-block partial sums of dgamma / dbeta behind; a one-wave-per-channel final adds them in block order (fp64), as the
// training kernels do: deterministic, no atomics.  The forward of such a unit is the plain conv + lfd_bn_train_apply_f16 on
// the row lfd_bn_eval_stats_f32 wrote (same float32[2C] = (mean, rstd) layout as the batch statistics).
#include "common.h"
#include "train_bn.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 1024;
constexpr int kMaxC = 256;

typedef _Float16 h8 __attribute__((ext_vector_type(8)));

union Vec16 {
  uint4 u;
  h8 h;
};

__device__ __forceinline__ h8 ld8(const __half* p, int64_t vec) {
  Vec16 v;
  v.u = reinterpret_cast<const uint4*>(p)[vec];
  return v.h;
}
__device__ __forceinline__ void st8(__half* p, int64_t vec, h8 h) {
  Vec16 v;
  v.h = h;
  reinterpret_cast<uint4*>(p)[vec] = v.u;
}

inline unsigned grid_for_vecs(int64_t vecs) {
  int64_t b = (vecs + kThreads - 1) / kThreads;
  if (b > kMaxBlocks) b = kMaxBlocks;
  if (b < 1) b = 1;
  return (unsigned)b;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

inline bool channels_ok(int c) { return c >= 8 && c <= kMaxC && (c & (c - 1)) == 0; }

// ---- running statistics -> stats rows ------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void k_bn_eval_stats(const lfd_bn_eval_job_t* __restrict__ jobs) {
  const lfd_bn_eval_job_t j = jobs[blockIdx.y];
  const int ch = blockIdx.x * kThreads + threadIdx.x;
  if (ch >= j.channels) return;
  j.stats[ch] = j.running_mean[ch];
  j.stats[j.channels + ch] = (float)(1.0 / sqrt((double)j.running_var[ch] + (double)j.eps));
}

// ---- conv weight x eval norm -> folded weight + bias ---------------------------------------------------
// job table in device memory (first_elem ascending), binary search per thread (as k_pack_weights)
__global__ __launch_bounds__(kThreads) void k_conv_bn_eval_fold(const lfd_bn_fold_job_t* __restrict__ jobs, int njobs, int total) {
  const int v = blockIdx.x * kThreads + threadIdx.x;
  if (v >= total) return;
  int lo = 0, hi = njobs - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (jobs[mid].first_elem <= v) lo = mid; else hi = mid - 1;
  }
  const lfd_bn_fold_job_t j = jobs[lo];
  const int i = v - j.first_elem;
  const int row = i / j.row_elems;
  const float a = j.gamma[row] * j.stats[j.cout + row];
  j.w_out[i] = j.w[i] * a;
  if (i - row * j.row_elems == 0) j.bias_out[row] = j.beta[row] - j.stats[row] * a;
}

// ---- backward ------------------------------------------------------------------------------------------
// Per-channel sums of a block: every thread owns one 8-channel group (the grid stride is a multiple of c / 8); the block
// combines the threads of a group through LDS and writes partial[block][2][c] (train.hip block_channel_reduce<2>).
__device__ __forceinline__ void block_channel_reduce2(float (&acc)[2][8], int c, float* partial_out) {
  __shared__ float red[kThreads][2 * 8 + 1];
  for (int q = 0; q < 2; ++q)
    for (int e = 0; e < 8; ++e) red[threadIdx.x][q * 8 + e] = acc[q][e];
  __syncthreads();
  const int groups = c >> 3;
  for (int o = threadIdx.x; o < 2 * c; o += kThreads) {
    const int q = o / c, ch = o - q * c;
    const int cg = ch >> 3, e = ch & 7;
    float s = 0.f;
    for (int t = cg; t < kThreads; t += groups) s += red[t][q * 8 + e];
    partial_out[(size_t)blockIdx.x * 2 * c + o] = s;
  }
}

// g = dz * [ReLU passed] (mask from the stored output z when given, else -- relu_y -- recomputed from y as
// [gamma * xhat + beta > 0], else no ReLU); dy = (gamma * rstd) * g; partial sums of g and g * xhat
__global__ __launch_bounds__(kThreads) void k_bn_eval_bwd(const __half* __restrict__ dz, const __half* __restrict__ y,
                                                         const __half* __restrict__ z, int64_t vecs, int c,
                                                         const float* __restrict__ stats, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, int relu_y, float* partials,
                                                         __half* __restrict__ dy, __half* __restrict__ g_out) {
  const int groups = c >> 3;
  const int64_t v0 = (int64_t)blockIdx.x * kThreads + threadIdx.x, stride = (int64_t)gridDim.x * kThreads;
  h8 d0, y0, z0;
  if (v0 < vecs) {       // the thread's first vectors are requested before the per-channel parameters (train.hip)
    d0 = ld8(dz, v0);
    y0 = ld8(y, v0);
    if (z) z0 = ld8(z, v0);
  }
  const int cg = (int)(v0 & (groups - 1));      // channel counts are powers of two (channels_ok): no 64-bit division
  float mean[8], rstd[8], a[8], ga[8], be[8], acc[2][8];
  for (int e = 0; e < 8; ++e) {
    const int ch = cg * 8 + e;
    mean[e] = stats[ch];
    rstd[e] = stats[c + ch];
    ga[e] = gamma[ch];
    be[e] = relu_y ? beta[ch] : 0.f;
    a[e] = gamma[ch] * rstd[e];
    acc[0][e] = acc[1][e] = 0.f;
  }
  auto body = [&](int64_t v, const h8& d, const h8& yy, const h8& zz) {
    h8 o, go;
    for (int e = 0; e < 8; ++e) {
      float g = (float)d[e];
      const float xh = LFD_BN_XHAT((float)yy[e], mean[e], rstd[e]);
      if (z && !((float)zz[e] > 0.f)) g = 0.f;
      if (relu_y && !LFD_BN_RELU_OPEN(ga[e], be[e], xh)) g = 0.f;
      acc[0][e] += g;
      acc[1][e] += g * xh;
      o[e] = (_Float16)(a[e] * g);
      go[e] = (_Float16)g;
    }
    st8(dy, v, o);
    if (g_out) st8(g_out, v, go);
  };
  if (v0 < vecs) {
    body(v0, d0, y0, z0);
    for (int64_t v = v0 + stride; v < vecs; v += stride) {
      const h8 d = ld8(dz, v), yy = ld8(y, v);
      h8 zz;
      if (z) zz = ld8(z, v);
      body(v, d, yy, zz);
    }
  }
  block_channel_reduce2(acc, c, partials);
}

// one wave per channel: lanes stride over the block partials, fp64, rows in a fixed order (train.hip k_bn_bwd_final)
__global__ __launch_bounds__(64) void k_bn_eval_bwd_final(const float* partials, int nblocks, int c, float inv_scale,
                                                         int accumulate, float* dgamma, float* dbeta) {
  const int ch = blockIdx.x;
  double s = 0.0, sx = 0.0;
  int b = threadIdx.x;
  for (; b + 192 < nblocks; b += 256) {        // four rows in flight, adds in row order
    float u[4], v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      u[k] = partials[(size_t)(b + 64 * k) * 2 * c + ch];
      v[k] = partials[(size_t)(b + 64 * k) * 2 * c + c + ch];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) { s += (double)u[k]; sx += (double)v[k]; }
  }
  for (; b < nblocks; b += 64) {
    s += (double)partials[(size_t)b * 2 * c + ch];
    sx += (double)partials[(size_t)b * 2 * c + c + ch];
  }
  s = wave_sum_d(s);
  sx = wave_sum_d(sx);
  if (threadIdx.x != 0) return;
  if (dbeta) dbeta[ch] = (accumulate ? dbeta[ch] : 0.f) + (float)(s * (double)inv_scale);
  if (dgamma) dgamma[ch] = (accumulate ? dgamma[ch] : 0.f) + (float)(sx * (double)inv_scale);
}

}  // namespace

extern "C" {

int lfd_bn_eval_stats_f32(const lfd_bn_eval_job_t* jobs_device, int32_t njobs, int32_t max_channels, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (njobs < 0 || njobs > 65535 || max_channels < 0) return LFD_ERR_INVALID_ARGUMENT;
  if (njobs == 0 || max_channels == 0) return LFD_OK;
  if (!jobs_device) return LFD_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_bn_eval_stats, dim3((max_channels + kThreads - 1) / kThreads, njobs), dim3(kThreads), 0, st, jobs_device);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

int lfd_conv_bn_eval_fold_f32(const lfd_bn_fold_job_t* jobs_device, int32_t njobs, int32_t total_elems, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (njobs < 0 || total_elems < 0) return LFD_ERR_INVALID_ARGUMENT;
  if (njobs == 0 || total_elems == 0) return LFD_OK;
  if (!jobs_device) return LFD_ERR_INVALID_ARGUMENT;
  hipLaunchKernelGGL(k_conv_bn_eval_fold, dim3((total_elems + kThreads - 1) / kThreads), dim3(kThreads), 0, st, jobs_device, njobs,
                     total_elems);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

int lfd_bn_eval_bwd_f16(const void* dz, const void* y, const void* z, int32_t relu, int64_t pixels, int32_t channels,
                        const float* stats, const float* gamma, const float* beta, float inv_scale, int32_t accumulate,
                        void* workspace, size_t workspace_bytes, float* dgamma, float* dbeta, void* dy, void* g_out,
                        lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!dz || !y || !stats || !gamma || !dy || !workspace || pixels < 1 || !channels_ok(channels)) return LFD_ERR_INVALID_ARGUMENT;
  if (!lfd_aligned16(dz) || !lfd_aligned16(y) || !lfd_aligned16(z) || !lfd_aligned16(dy) || !lfd_aligned16(g_out))
    return LFD_ERR_INVALID_ARGUMENT;
  if (workspace_bytes < lfd_train_workspace_bytes()) return LFD_ERR_WORKSPACE_TOO_SMALL;
  const int relu_y = (relu && !z) ? 1 : 0;       // no stored output given: the ReLU mask is recomputed from y
  if (relu_y && !beta) return LFD_ERR_INVALID_ARGUMENT;
  if (!relu) z = nullptr;
  const int64_t vecs = pixels * (channels / 8);
  const unsigned g = grid_for_vecs(vecs);
  float* partials = reinterpret_cast<float*>(workspace);      // g rows [2][channels], g <= kMaxBlocks
  hipLaunchKernelGGL(k_bn_eval_bwd, dim3(g), dim3(kThreads), 0, st, (const __half*)dz, (const __half*)y, (const __half*)z, vecs,
                     channels, stats, gamma, beta, relu_y, partials, (__half*)dy, (__half*)g_out);
  LFD_CHECK_LAUNCH();
  if (dgamma || dbeta) {
    hipLaunchKernelGGL(k_bn_eval_bwd_final, dim3(channels), dim3(64), 0, st, partials, (int)g, channels, inv_scale, accumulate,
                       dgamma, dbeta);
    LFD_CHECK_LAUNCH();
  }
  return LFD_OK;
}

}  // extern "C"
