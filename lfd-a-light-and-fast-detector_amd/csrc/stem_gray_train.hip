// csrc/stem_gray_train.hip -- first stem conv of a one-channel (grayscale) model in training: conv3x3 stride 2 pad 1, 1 -> C
// (C = 32, 64) on the NCHW fp32 image batch [N,1,H,W] (lfd_resnet.py:358 / :378 `nn.Conv2d(input_channels, stem_channels, 3, 2, 1,
// bias=False)` with input_channels = 1, followed by train-mode BatchNorm2d + ReLU).  The gray twins of the RGB first-conv kernels
// of train.hip (k_conv0_fwd_mfma, k_conv0_wgrad_mfma), with their numerics: image values rounded to fp16 for the MFMA, fp32
// accumulation, y NHWC fp16 (pre-norm), parameter gradients unscaled fp32, every reduction in a fixed order.
//
//   forward :  y[px][co] = sum_t W[co][t] * patch[px][t]     v_mfma_f32_32x32x16_f16, A = W (rows = co), B = patches (cols = 32
//              pixels); the 9 taps (t = 3 ky + kx) are ONE 16-wide k-step (half 0 of the wave holds t = 0..7, half 1 t = 8 and
//              seven zeros), where RGB needs two.  Interior groups load the three kx taps of a row as one 12-byte load: three
//              loads per pixel instead of nine gathers (LESSONS 42).  Output lines staged through LDS for 16-byte stores;
//              STATS: BatchNorm partial sums of the stored fp16 values (the stat_partials scheme of k_conv0_fwd_mfma).
//   wgrad   :  dW[co][t] = sum_px dy[px][co] * patch[px][t]  v_mfma_f32_16x16x32_f16, k = 32 consecutive output pixels of a
//              row; A = dy^T (rows = 16 channels, transposing LDS read), B = patches (cols = 16 taps, 9 real).  BN: dy is formed
//              from (dz, y) on each 16-byte chunk with train_bn.h -- the arithmetic of k_bn_bwd_apply, bit for bit.
#include "common.h"
#include "train_bn.h"

namespace {

constexpr int kThreads = 256;
constexpr int kFwdMaxBlocks = 2048;      // forward: <= 2048 stat rows x 2 x 64 floats (the start of the training workspace)
constexpr int kWgMaxBlocks = 1024;       // weight gradient: <= 1024 partial rows x C x 16 floats

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f16v __attribute__((ext_vector_type(16)));
typedef float f4v __attribute__((ext_vector_type(4)));
typedef float f3u __attribute__((ext_vector_type(3), aligned(4)));      // three consecutive floats at any 4-byte boundary
typedef short s4v __attribute__((__vector_size__(4 * sizeof(short))));
typedef __attribute__((address_space(3))) s4v lds_s4v;

__device__ __forceinline__ h8 tr_frag(const char* base, uint32_t off0, uint32_t off1) {
  union { s4v s[2]; h8 h; } u;
  u.s[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v*)(base + off0));
  u.s[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4v*)(base + off1));
  return u.h;
}

// ---------------------------------------------------------------------------------------------------------
// Forward.  One wave = 32 output pixels per trip (grid-stride); C / 32 MFMAs of one k-step each.  Pixel indices are 32-bit
// (the host refuses maps of 2^31 elements, LESSONS 38).
// ---------------------------------------------------------------------------------------------------------
template <int C>
__global__ __launch_bounds__(kThreads) void k_gray_conv0_fwd(const float* __restrict__ x, int n, int h, int w,
                                                            const float* __restrict__ wt, __half* __restrict__ y,
                                                            float* stat_partials) {
  constexpr int NCT = C / 32, CH = C / 8, LINE = C * 2;       // 32-channel tiles, 16-byte chunks per pixel line, line bytes
  __shared__ __attribute__((aligned(16))) uint4 s_stage[kThreads / 64][32 * CH];     // per wave: 32 pixels x LINE
  float st_s[8], st_q[8];
  for (int e = 0; e < 8; ++e) st_s[e] = st_q[e] = 0.f;
  const int l = threadIdx.x & 63, hk = l >> 5, px = l & 31;
  const int ho = (h + 1) / 2, wo = (w + 1) / 2;
  const int64_t total = (int64_t)n * ho * wo;
  // A fragments: W[ct*32 + (l&31)][8 hk + j], taps >= 9 zero
  h8 wa[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct)
    for (int j = 0; j < 8; ++j) {
      const int t = 8 * hk + j;
      wa[ct][j] = (_Float16)(t < 9 ? wt[(ct * 32 + px) * 9 + t] : 0.f);
    }
  char* stg = reinterpret_cast<char*>(s_stage[threadIdx.x >> 6]);
  const int64_t wave0 = ((int64_t)blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6)) * 32;
  const int64_t stride = (int64_t)gridDim.x * (kThreads / 64) * 32;
  for (int64_t p0 = wave0; p0 < total; p0 += stride) {
    const int64_t p = p0 + px;
    const bool pv = p < total;
    const unsigned pc = pv ? (unsigned)p : 0u;
    const unsigned qq = pc / (unsigned)wo;
    const int ox = (int)(pc - qq * (unsigned)wo);
    const unsigned im = qq / (unsigned)ho;
    const int oy = (int)(qq - im * (unsigned)ho);
    const float* xb = x + ((unsigned)im * (unsigned)h + 2u * (unsigned)oy) * (unsigned)w + 2 * ox;     // input pixel (2 oy, 2 ox)
    h8 b;
    const bool lr_inner = pv && ox > 0 && 2 * ox + 1 < w;
    if (__builtin_amdgcn_ballot_w64(pv && !lr_inner) == 0) {
      // no lane on the left / right border: rows ky = 0..2 as three 12-byte loads (columns 2 ox - 1 .. 2 ox + 1).  The wide
      // path implies w >= 4, so the safe address x[0..2] of rows outside the image and of idle lanes is in bounds.
      f3u T[3];
#pragma unroll
      for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * oy + ky - 1;
        const bool rv = pv && iy >= 0 && iy < h;
        const float* src = rv ? xb + (ky - 1) * w - 1 : x;     // (unconditional load from a safe address + select)
        const f3u v = *reinterpret_cast<const f3u*>(src);
        T[ky] = rv ? v : f3u{0.f, 0.f, 0.f};
      }
      // half 0: taps 0..7 = T[0][0..2] T[1][0..2] T[2][0..1]; half 1: tap 8 = T[2][2], then zeros
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float v0 = T[j / 3][j % 3];
        const float v1 = j == 0 ? T[2][2] : 0.f;
        b[j] = (_Float16)(hk ? v1 : v0);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int t = 8 * hk + j, ky = t / 3, kx = t - 3 * (t / 3);
        const int iy = 2 * oy + ky - 1, ix = 2 * ox + kx - 1;
        const bool ok = pv && t < 9 && iy >= 0 && iy < h && ix >= 0 && ix < w;
        const float raw = xb[ok ? (ky - 1) * w + kx - 1 : 0];      // (unconditional load from a safe address + select)
        b[j] = (_Float16)(ok ? raw : 0.f);
      }
    }
    // D layout: lane = pixel, register r -> channel ct*32 + 8 (r >> 2) + 4 hk + (r & 3).  Staged [pixel][CH chunks of 16 B],
    // chunk XOR (pixel % CH); LDS operations of one wave execute in order: no barrier.
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      f16v acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(wa[ct], b, acc, 0, 0, 0);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        h4 o;
        for (int e = 0; e < 4; ++e) o[e] = (_Float16)acc[4 * g + e];
        *reinterpret_cast<h4*>(stg + px * LINE + (((ct * 4 + g) ^ (px & (CH - 1))) << 4) + 8 * hk) = o;
      }
    }
    // 32 lines, fully coalesced 16-byte stores; chunk index = l % CH for every store of the lane
#pragma unroll
    for (int j = 0; j < CH / 2; ++j) {
      const int idx = j * 64 + l;
      const int q = idx / CH, ck = idx % CH;
      const uint4 v = *reinterpret_cast<const uint4*>(stg + q * LINE + ((ck ^ (q & (CH - 1))) << 4));
      const bool ok = p0 + q < total;
      if (ok) *reinterpret_cast<uint4*>(reinterpret_cast<char*>(y) + (p0 + q) * LINE + ck * 16) = v;
      if (stat_partials) {
        const uint32_t wd[4] = {ok ? v.x : 0u, ok ? v.y : 0u, ok ? v.z : 0u, ok ? v.w : 0u};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const float lo = (float)__builtin_bit_cast(_Float16, (unsigned short)(wd[k] & 0xffffu));
          const float hi = (float)__builtin_bit_cast(_Float16, (unsigned short)(wd[k] >> 16));
          st_s[2 * k] += lo;  st_q[2 * k] += lo * lo;
          st_s[2 * k + 1] += hi;  st_q[2 * k + 1] += hi * hi;
        }
      }
    }
  }
  if (stat_partials) {
    // lanes l, l + CH, ... hold the same chunk: butterfly, then the four waves through LDS in wave order -> row [block][2][C]
    for (int e = 0; e < 8; ++e)
      for (int d = 32; d >= CH; d >>= 1) {
        st_s[e] += __shfl_xor(st_s[e], d);
        st_q[e] += __shfl_xor(st_q[e], d);
      }
    __syncthreads();
    float* red = reinterpret_cast<float*>(&s_stage[0][0]);        // [4 waves][2][C]
    const int wv = threadIdx.x >> 6;
    if (l < CH)
      for (int e = 0; e < 8; ++e) {
        red[(wv * 2 + 0) * C + l * 8 + e] = st_s[e];
        red[(wv * 2 + 1) * C + l * 8 + e] = st_q[e];
      }
    __syncthreads();
    if (threadIdx.x < 2 * C) {
      const int q = threadIdx.x / C, ch = threadIdx.x % C;
      stat_partials[(size_t)blockIdx.x * 2 * C + threadIdx.x] =
          ((red[(0 * 2 + q) * C + ch] + red[(1 * 2 + q) * C + ch]) + red[(2 * 2 + q) * C + ch]) + red[(3 * 2 + q) * C + ch];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------
// Weight gradient.  k-step = 32 consecutive output pixels of one row (zero beyond the row); U k-steps per wave and trip, visited
// s, s + S, ... (S = all waves of the grid), all their loads requested before the first LDS write.  Per k-step a wave stages the
// dy tile [32 px][C] (144- / 80-byte pixel pitch), reads it back transposed as the A operand of C/16 16x16x32 MFMAs, and gathers
// its B operand -- patch[8 (l >> 4) + j][tap l & 15] -- from the image.  partial[block][co][16] (the four waves in fixed order).
// ---------------------------------------------------------------------------------------------------------
template <int C, bool BN>
__global__ __launch_bounds__(kThreads) void k_gray_conv0_wgrad(const float* __restrict__ x, const __half* __restrict__ dy, int n,
                                                              int h, int w, float* partials, const __half* __restrict__ yb,
                                                              const float* __restrict__ stats,
                                                              const float* __restrict__ gamma, const float* __restrict__ beta,
                                                              const float* __restrict__ sums, float inv_m) {
  constexpr int U = 2, NT = C / 16, CH = C / 8, PITCH = C * 2 + 16, TILE = 32 * PITCH, LPL = CH / 2;   // LPL: chunks per lane
  constexpr int STG = 4 * U * TILE, RED = 4 * C * 16 * 4;
  __shared__ __attribute__((aligned(16))) char smem[STG > RED ? STG : RED];
  float (*red)[C * 16] = reinterpret_cast<float (*)[C * 16]>(smem);          // after the loop (behind a barrier)
  const int wave = threadIdx.x >> 6, l = threadIdx.x & 63, grp = l >> 4, i16 = l & 15;
  char* my = smem + wave * U * TILE;
  const int ho = (h + 1) / 2, wo = (w + 1) / 2;
  const int segs = (wo + 31) / 32;
  const int64_t total = (int64_t)n * ho * segs;
  const int t = i16, ky = t / 3, kx = t - 3 * (t / 3);            // this lane's tap (B column); t >= 9: padding
  f4v acc[NT];
#pragma unroll
  for (int ct = 0; ct < NT; ++ct)
    for (int r = 0; r < 4; ++r) acc[ct][r] = 0.f;
  // A operand: lane i16 of group grp addresses pixel 8 grp + 4 r + (i16 >> 2), channels 4 (i16 & 3) .. + 3 of the 16-channel tile
  uint32_t a_off[2];
  for (int r = 0; r < 2; ++r) a_off[r] = (8 * grp + 4 * r + (i16 >> 2)) * PITCH + 4 * (i16 & 3) * 2;
  // BN: per-channel constants of this lane's 16-byte chunk (chunk l % CH in every load: 64 is a multiple of CH)
  LfdBnBwdChunk p;
  if constexpr (BN) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int ch = (l % CH) * 8 + e;
      p.mean[e] = stats[ch];
      p.rstd[e] = stats[C + ch];
      p.ga[e] = gamma[ch];
      p.be[e] = beta[ch];
      p.a[e] = gamma[ch] * p.rstd[e];
      p.mg[e] = sums[ch] * inv_m;
      p.mgx[e] = sums[C + ch] * inv_m;
    }
  }
  const int64_t S = (int64_t)gridDim.x * 4;
  for (int64_t s0 = (int64_t)blockIdx.x * 4 + wave; s0 < total; s0 += U * S) {
    uint4 dv[U][LPL];
    uint4 yv[BN ? U : 1][LPL];
    bool okd[U][LPL];
    float raw[U][8];
    bool okj[U][8];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t s = s0 + u * S;
      const bool sv = s < total;
      const unsigned sc = sv ? (unsigned)s : 0u;          // 32-bit index arithmetic (host-checked)
      const unsigned qq = sc / (unsigned)segs;
      const int seg = (int)(sc - qq * (unsigned)segs);
      const unsigned im = qq / (unsigned)ho;
      const int oy = (int)(qq - im * (unsigned)ho);
      const int ox0 = seg * 32;
      const int64_t row0 = ((int64_t)im * ho + oy) * wo + ox0;          // first output pixel of the k-step
#pragma unroll
      for (int k = 0; k < LPL; ++k) {
        const int i = l + 64 * k;
        const int q = i / CH, c8 = i % CH;
        const bool in = sv && ox0 + q < wo;
        const int64_t eo = in ? (row0 + q) * C + c8 * 8 : 0;
        dv[u][k] = *reinterpret_cast<const uint4*>(dy + eo);
        if constexpr (BN) yv[u][k] = *reinterpret_cast<const uint4*>(yb + eo);
        okd[u][k] = in;
      }
      const int iy = 2 * oy + ky - 1;
      const unsigned xrow = ((unsigned)im * (unsigned)h + (unsigned)iy) * (unsigned)w;     // used only where iy is in range
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const int ox = ox0 + 8 * grp + j, ix = 2 * ox + kx - 1;
        okj[u][j] = sv && t < 9 && ox < wo && iy >= 0 && iy < h && ix >= 0 && ix < w;
        raw[u][j] = x[okj[u][j] ? xrow + (unsigned)ix : 0u];      // unconditional load from a safe address + select
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int k = 0; k < LPL; ++k) {
        uint4 v = dv[u][k];
        if constexpr (BN) v = lfd_bn_bwd_dy_relu_y8(v, yv[u][k], p);
        const int i = l + 64 * k;
        *reinterpret_cast<uint4*>(my + u * TILE + (i / CH) * PITCH + (i % CH) * 16) = okd[u][k] ? v : make_uint4(0, 0, 0, 0);
      }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      h8 b;
#pragma unroll
      for (int j = 0; j < 8; ++j) b[j] = (_Float16)(okj[u][j] ? raw[u][j] : 0.f);
#pragma unroll
      for (int ct = 0; ct < NT; ++ct) {
        const h8 af = tr_frag(my + u * TILE, a_off[0] + ct * 32, a_off[1] + ct * 32);
        acc[ct] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, b, acc[ct], 0, 0, 0);
      }
    }
  }
  __syncthreads();     // red aliases the staging tiles of waves that may still have been contracting
  // D layout: lane -> column (tap) l & 15, register r -> row (channel) ct*16 + 4 (l >> 4) + r
#pragma unroll
  for (int ct = 0; ct < NT; ++ct)
    for (int r = 0; r < 4; ++r) red[wave][(ct * 16 + 4 * grp + r) * 16 + t] = acc[ct][r];
  __syncthreads();
  for (int o = threadIdx.x; o < C * 16; o += kThreads)
    partials[(size_t)blockIdx.x * C * 16 + o] = ((red[0][o] + red[1][o]) + red[2][o]) + red[3][o];
}

// dw[co][t] (+)= inv_scale * sum over blocks of partial[block][co][t], fp64 in block order; one wave per output (C x 9)
__global__ __launch_bounds__(64) void k_gray_wgrad_final(const float* partials, int nblocks, int c, float inv_scale,
                                                        int accumulate, float* out) {
  const int i = blockIdx.x, co = i / 9, t = i - co * 9;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 64) s += (double)partials[(size_t)b * c * 16 + co * 16 + t];
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
  if (threadIdx.x != 0) return;
  out[i] = (accumulate ? out[i] : 0.f) + (float)(s * (double)inv_scale);
}

// shared argument checks: status code, or LFD_OK
int check_map(const float* x, int32_t n, int32_t h, int32_t w, int32_t channels) {
  if (!x || n < 1 || h < 1 || w < 1 || (channels != 32 && channels != 64) || (reinterpret_cast<uintptr_t>(x) & 3))
    return LFD_ERR_INVALID_ARGUMENT;
  const int64_t pixels = (int64_t)n * ((h + 1) / 2) * ((w + 1) / 2);
  // 32-bit pixel / element indices in the kernels (LESSONS 38)
  if ((int64_t)n * h * w >= ((int64_t)1 << 31) || pixels * channels >= ((int64_t)1 << 31)) return LFD_ERR_UNSUPPORTED;
  return LFD_OK;
}

int gray_fwd(const float* x, int32_t n, int32_t h, int32_t w, int32_t channels, const float* wt, void* y, float* stat_partials,
             unsigned* blocks_out, hipStream_t st) {
  const int64_t groups = ((int64_t)n * ((h + 1) / 2) * ((w + 1) / 2) + 127) / 128;     // 4 waves x 32 pixels per block pass
  const unsigned blocks = (unsigned)(groups < kFwdMaxBlocks ? groups : kFwdMaxBlocks);
  if (blocks_out) *blocks_out = blocks;
  if (channels == 64)
    hipLaunchKernelGGL(k_gray_conv0_fwd<64>, dim3(blocks), dim3(kThreads), 0, st, x, n, h, w, wt, (__half*)y, stat_partials);
  else
    hipLaunchKernelGGL(k_gray_conv0_fwd<32>, dim3(blocks), dim3(kThreads), 0, st, x, n, h, w, wt, (__half*)y, stat_partials);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

// weight-gradient partials (BN: dy formed from dz, y and the sums at workspace + kLfdBnSumsAt) + the final sum into dw
int gray_wgrad(const float* x, const void* dy, int32_t n, int32_t h, int32_t w, int32_t channels, float* wpart, const void* y,
               const float* stats, const float* gamma, const float* beta, const float* sums, float inv_scale, int32_t accumulate,
               float* dw, hipStream_t st) {
  const int ho = (h + 1) / 2, wo = (w + 1) / 2;
  const int64_t ksteps = (int64_t)n * ho * ((wo + 31) / 32);
  const int nb = (int)(ksteps / 4 < 1 ? 1 : (ksteps / 4 > kWgMaxBlocks ? kWgMaxBlocks : ksteps / 4));
  const float inv_m = (float)(1.0 / ((double)n * ho * wo));
  const __half* d = (const __half*)dy;
  const __half* yb = (const __half*)y;
  if (channels == 64) {
    if (y)
      hipLaunchKernelGGL((k_gray_conv0_wgrad<64, true>), dim3(nb), dim3(kThreads), 0, st, x, d, n, h, w, wpart, yb, stats,
                         gamma, beta, sums, inv_m);
    else
      hipLaunchKernelGGL((k_gray_conv0_wgrad<64, false>), dim3(nb), dim3(kThreads), 0, st, x, d, n, h, w, wpart, yb, stats,
                         gamma, beta, sums, inv_m);
  } else {
    if (y)
      hipLaunchKernelGGL((k_gray_conv0_wgrad<32, true>), dim3(nb), dim3(kThreads), 0, st, x, d, n, h, w, wpart, yb, stats,
                         gamma, beta, sums, inv_m);
    else
      hipLaunchKernelGGL((k_gray_conv0_wgrad<32, false>), dim3(nb), dim3(kThreads), 0, st, x, d, n, h, w, wpart, yb, stats,
                         gamma, beta, sums, inv_m);
  }
  LFD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_gray_wgrad_final, dim3(channels * 9), dim3(64), 0, st, wpart, nb, channels, inv_scale, accumulate, dw);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

}  // namespace

extern "C" {

int lfd_stem_gray_train_fwd(const float* x_nchw, int32_t n, int32_t h, int32_t w, int32_t channels, const float* weight_oihw,
                            void* y, lfd_stream_t stream) {
  const int rc = check_map(x_nchw, n, h, w, channels);
  if (rc != LFD_OK) return rc;
  if (!weight_oihw || !y || !lfd_aligned16(y)) return LFD_ERR_INVALID_ARGUMENT;
  return gray_fwd(x_nchw, n, h, w, channels, weight_oihw, y, nullptr, nullptr, reinterpret_cast<hipStream_t>(stream));
}

int lfd_stem_gray_train_fwd_bn_stats(const float* x_nchw, int32_t n, int32_t h, int32_t w, int32_t channels,
                                     const float* weight_oihw, void* y, float eps, float momentum, float* running_mean,
                                     float* running_var, void* workspace, size_t workspace_bytes, float* stats,
                                     lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int rc = check_map(x_nchw, n, h, w, channels);
  if (rc != LFD_OK) return rc;
  if (!weight_oihw || !y || !lfd_aligned16(y) || !workspace || !stats || (running_mean == nullptr) != (running_var == nullptr))
    return LFD_ERR_INVALID_ARGUMENT;
  if (workspace_bytes < lfd_train_workspace_bytes()) return LFD_ERR_WORKSPACE_TOO_SMALL;
  const int64_t pixels = (int64_t)n * ((h + 1) / 2) * ((w + 1) / 2);
  if (channels != 64) {      // the 32-channel stem: conv, then the statistics pass (as RGB)
    const int r = gray_fwd(x_nchw, n, h, w, channels, weight_oihw, y, nullptr, nullptr, st);
    if (r != LFD_OK) return r;
    return lfd_bn_train_stats_f16(y, pixels, channels, eps, momentum, running_mean, running_var, workspace, workspace_bytes, stats,
                                  stream);
  }
  unsigned blocks = 0;
  float* partials = reinterpret_cast<float*>(workspace);
  const int r = gray_fwd(x_nchw, n, h, w, channels, weight_oihw, y, partials, &blocks, st);
  if (r != LFD_OK) return r;
  return lfd_bn_stats_final_rows(partials, (int)blocks, channels, pixels, eps, momentum, running_mean, running_var, stats, st);
}

int lfd_stem_gray_wgrad(const float* x_nchw, const void* dy, int32_t n, int32_t h, int32_t w, int32_t channels, float inv_scale,
                        int32_t accumulate, void* workspace, size_t workspace_bytes, float* dw, lfd_stream_t stream) {
  const int rc = check_map(x_nchw, n, h, w, channels);
  if (rc != LFD_OK) return rc;
  if (!dy || !lfd_aligned16(dy) || !dw || !workspace) return LFD_ERR_INVALID_ARGUMENT;
  if (workspace_bytes < lfd_train_workspace_bytes()) return LFD_ERR_WORKSPACE_TOO_SMALL;
  return gray_wgrad(x_nchw, dy, n, h, w, channels, reinterpret_cast<float*>(workspace), nullptr, nullptr, nullptr, nullptr, nullptr,
                    inv_scale, accumulate, dw, reinterpret_cast<hipStream_t>(stream));
}

int lfd_stem_gray_bn_bwd_wgrad_rows(const float* x_nchw, const void* dz, const void* y, int32_t n, int32_t h, int32_t w,
                                    int32_t channels, const float* stats, const float* gamma, const float* beta, float inv_scale,
                                    int32_t accumulate, int32_t sum_rows, void* workspace, size_t workspace_bytes, float* dgamma,
                                    float* dbeta, float* dw, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const int rc = check_map(x_nchw, n, h, w, channels);
  if (rc != LFD_OK) return rc;
  if (sum_rows < 0 || sum_rows > 1024) return LFD_ERR_INVALID_ARGUMENT;
  if (!dz || !y || !lfd_aligned16(dz) || !lfd_aligned16(y) || !stats || !gamma || !beta || !dw || !workspace)
    return LFD_ERR_INVALID_ARGUMENT;
  if (workspace_bytes < lfd_train_workspace_bytes()) return LFD_ERR_WORKSPACE_TOO_SMALL;
  const int64_t pixels = (int64_t)n * ((h + 1) / 2) * ((w + 1) / 2);
  float* ws = reinterpret_cast<float*>(workspace);
  int r = lfd_first_unit_bn_bwd_sums(dz, y, pixels, channels, stats, gamma, beta, inv_scale, accumulate, sum_rows, ws, dgamma, dbeta,
                                     st);
  if (r != LFD_OK) return r;
  return gray_wgrad(x_nchw, dz, n, h, w, channels, ws + kLfdBnWpartAt, y, stats, gamma, beta, ws + kLfdBnSumsAt, inv_scale, accumulate,
                    dw, st);
}

}  // extern "C"
