// csrc/sibling_train.hip -- the backward of the element-wise operators of csrc/sibling.hip and the bias gradient of a plain
// conv: what the training pass of an FPN / SimpleFPN neck needs next to the conv / norm kernels of csrc/train.hip.  Gradients are
// NHWC fp16 (they carry the loss scale), arithmetic is fp32 with one rounding to fp16.  All HBM-bound streaming kernels, 16-byte
// accesses, one (pixel, 8-channel chunk) per lane.  Every kernel is a GATHER -- the lane that owns an element of the result
// reads everything that flows into it -- so there is no atomic and two runs give the same bits.
#include "common.h"

namespace {

typedef _Float16 h8 __attribute__((ext_vector_type(8)));
constexpr int kThreads = 256;
constexpr int kBiasMaxBlocks = 512;       // rows of per-block partial sums of the bias gradient
constexpr int kBiasMaxChannels = 128;

// Adjoint of k_upsample_add (sibling.hip): g_src[n,yy,xx,:] += sum of g_dst[n,y,x,:] over the destination pixels whose forward
// source index is (yy, xx).  Membership is the FORWARD's own expression evaluated per candidate; [y0, y1] x [x0, x1] is only a
// conservative range around yy * H / h (one pixel of slack on both sides covers the float rounding of y * (h / H)).
__global__ __launch_bounds__(kThreads) void k_upsample_add_bwd(_Float16* g_src, const _Float16* g_dst, int N, int H, int W, int h,
                                                               int w, int c8, float sy, float sx) {
  const int64_t total = (int64_t)N * h * w * c8;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int q = (int)(i % c8);
    int64_t t = i / c8;
    const int xx = (int)(t % w);
    t /= w;
    const int yy = (int)(t % h);
    const int n = (int)(t / h);
    int y0 = (int)((int64_t)yy * H / h) - 1, y1 = (int)(((int64_t)(yy + 1) * H + h - 1) / h) + 1;
    int x0 = (int)((int64_t)xx * W / w) - 1, x1 = (int)(((int64_t)(xx + 1) * W + w - 1) / w) + 1;
    y0 = y0 < 0 ? 0 : y0;
    x0 = x0 < 0 ? 0 : x0;
    y1 = y1 > H - 1 ? H - 1 : y1;
    x1 = x1 > W - 1 ? W - 1 : x1;
    const h8 own = reinterpret_cast<const h8*>(g_src)[i];
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = (float)own[k];
    for (int y = y0; y <= y1; ++y) {
      int fy = (int)floorf((float)y * sy);
      fy = fy < h - 1 ? fy : h - 1;
      if (fy != yy) continue;
      for (int x = x0; x <= x1; ++x) {
        int fx = (int)floorf((float)x * sx);
        fx = fx < w - 1 ? fx : w - 1;
        if (fx != xx) continue;
        const h8 v = reinterpret_cast<const h8*>(g_dst)[(((int64_t)n * H + y) * W + x) * c8 + q];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] += (float)v[k];
      }
    }
    h8 r;
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = (_Float16)acc[k];
    reinterpret_cast<h8*>(g_src)[i] = r;
  }
}

// Backward of k_maxpool3s2 (sibling.hip).  An input pixel lies in at most 2 x 2 windows; for each the window's argmax is
// recomputed per channel: the FIRST position in scan order (dy, then dx ascending, padding skipped) that attains the maximum --
// a strict `>` update as in ATen's max_pool2d_with_indices (a NaN also takes over, as there).  After a ReLU ties are the rule.
// The running maximum is kept as fp32 and the "argmax is me" flags as one bit mask: a first form with an h8 maximum, _Float16
// compares and a bool per channel gave a wrong argmax for the 8th channel of a chunk in the gfx950 build (the same source
// compiled for the host was right; not followed up) -- tests/test_gpu_pyramid_train.py compares every element.
__global__ __launch_bounds__(kThreads) void k_maxpool3s2_bwd(const _Float16* x, const _Float16* g_out, _Float16* g_in, int N,
                                                             int H, int W, int OH, int OW, int c8, int accumulate) {
  const int64_t total = (int64_t)N * H * W * c8;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < total; i += (int64_t)gridDim.x * kThreads) {
    const int q = (int)(i % c8);
    int64_t t = i / c8;
    const int px = (int)(t % W);
    t /= W;
    const int py = (int)(t % H);
    const int n = (int)(t / H);
    float acc[8];
    if (accumulate) {
      const h8 own = reinterpret_cast<const h8*>(g_in)[i];
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = (float)own[k];
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) acc[k] = 0.f;
    }
    // windows oy with 2 * oy - 1 <= py <= 2 * oy + 1
    const int oy0 = py / 2, oy1 = (py + 1) / 2, ox0 = px / 2, ox1 = (px + 1) / 2;
    for (int oy = oy0; oy <= oy1 && oy < OH; ++oy) {
      for (int ox = ox0; ox <= ox1 && ox < OW; ++ox) {
        float m[8];
        unsigned mine = 0u;          // bit k: this pixel is the argmax of channel k so far
        bool first = true;
#pragma unroll
        for (int k = 0; k < 8; ++k) m[k] = -INFINITY;
        for (int dy = 0; dy < 3; ++dy) {
          const int y = oy * 2 - 1 + dy;
          if (y < 0 || y >= H) continue;
          for (int dx = 0; dx < 3; ++dx) {
            const int xx = ox * 2 - 1 + dx;
            if (xx < 0 || xx >= W) continue;
            const h8 v = reinterpret_cast<const h8*>(x)[(((int64_t)n * H + y) * W + xx) * c8 + q];
            const bool me = (y == py) && (xx == px);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
              const float f = (float)v[k];
              if (first || f > m[k] || f != f) {
                m[k] = f;
                mine = me ? (mine | (1u << k)) : (mine & ~(1u << k));
              }
            }
            first = false;
          }
        }
        const h8 g = reinterpret_cast<const h8*>(g_out)[(((int64_t)n * OH + oy) * OW + ox) * c8 + q];
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] += ((mine >> k) & 1u) ? (float)g[k] : 0.f;
      }
    }
    h8 r;
#pragma unroll
    for (int k = 0; k < 8; ++k) r[k] = (_Float16)acc[k];
    reinterpret_cast<h8*>(g_in)[i] = r;
  }
}

// out = (g_a + g_b) * [y > 0]: the gradient of a tensor that leaves as relu(y) and also feeds an extra level through that relu
__global__ __launch_bounds__(kThreads) void k_relu_bwd_add(const _Float16* y, const _Float16* g_a, const _Float16* g_b,
                                                           _Float16* out, int64_t n8) {
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n8; i += (int64_t)gridDim.x * kThreads) {
    const h8 v = reinterpret_cast<const h8*>(y)[i];
    const h8 a = reinterpret_cast<const h8*>(g_a)[i];
    h8 b;
    if (g_b) b = reinterpret_cast<const h8*>(g_b)[i];
    h8 r;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float s = g_b ? (float)a[k] + (float)b[k] : (float)a[k];
      r[k] = v[k] > (_Float16)0 ? (_Float16)s : (_Float16)0;
    }
    reinterpret_cast<h8*>(out)[i] = r;
  }
}

// Bias gradient, stage 1.  The grid stride is a multiple of c8 (c8 divides kThreads), so a thread keeps its 8 channels for the
// whole walk: 8 fp32 sums per thread, then per channel the sum over the threads that hold it, in thread order.
__global__ __launch_bounds__(kThreads) void k_bias_grad_partial(const _Float16* dy, int64_t rows, int c8, float* partials) {
  __shared__ float red[kThreads][9];
  float acc[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.f;
  const int64_t vecs = rows * c8;
  for (int64_t v = (int64_t)blockIdx.x * kThreads + threadIdx.x; v < vecs; v += (int64_t)gridDim.x * kThreads) {
    const h8 d = reinterpret_cast<const h8*>(dy)[v];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] += (float)d[k];
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) red[threadIdx.x][k] = acc[k];
  __syncthreads();
  const int c = c8 * 8;
  if ((int)threadIdx.x < c) {
    const int ch = threadIdx.x;
    float s = 0.f;
    for (int tt = ch >> 3; tt < kThreads; tt += c8) s += red[tt][ch & 7];
    partials[(size_t)blockIdx.x * c + ch] = s;
  }
}

// stage 2: one wave per channel, fp64 over the blocks' partials in an order that depends on nblocks alone
__global__ __launch_bounds__(64) void k_bias_grad_final(const float* partials, int nblocks, int c, float inv_scale, float* dbias) {
  const int ch = blockIdx.x;
  double s = 0.0;
  for (int b = threadIdx.x; b < nblocks; b += 64) s += (double)partials[(size_t)b * c + ch];
  for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
  if (threadIdx.x == 0) dbias[ch] += (float)(s * (double)inv_scale);
}

inline unsigned grid_for(int64_t total) {
  int64_t b = (total + kThreads - 1) / kThreads;
  return (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

}  // namespace

extern "C" {

int lfd_upsample_nearest_add_bwd_nhwc_f16(void* g_src, const void* g_dst, int32_t n, int32_t H, int32_t W, int32_t h, int32_t w,
                                          int32_t c, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!g_src || !g_dst || g_src == g_dst || n < 1 || H < 1 || W < 1 || h < 1 || w < 1 || c < 8) return LFD_ERR_INVALID_ARGUMENT;
  if (!lfd_aligned16(g_src) || !lfd_aligned16(g_dst)) return LFD_ERR_INVALID_ARGUMENT;
  if (c % 8) return LFD_ERR_UNSUPPORTED;
  const int64_t total = (int64_t)n * h * w * (c / 8);
  hipLaunchKernelGGL(k_upsample_add_bwd, dim3(grid_for(total)), dim3(kThreads), 0, st, (_Float16*)g_src, (const _Float16*)g_dst,
                     n, H, W, h, w, c / 8, (float)h / (float)H, (float)w / (float)W);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

int lfd_maxpool3x3s2_bwd_nhwc_f16(const void* x, const void* g_out, void* g_in, int32_t n, int32_t h, int32_t w, int32_t c,
                                  int32_t accumulate, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!x || !g_out || !g_in || g_in == x || g_in == g_out || n < 1 || h < 1 || w < 1 || c < 8) return LFD_ERR_INVALID_ARGUMENT;
  if (!lfd_aligned16(x) || !lfd_aligned16(g_out) || !lfd_aligned16(g_in)) return LFD_ERR_INVALID_ARGUMENT;
  if (c % 8) return LFD_ERR_UNSUPPORTED;
  const int oh = (h + 2 - 3) / 2 + 1, ow = (w + 2 - 3) / 2 + 1;
  const int64_t total = (int64_t)n * h * w * (c / 8);
  hipLaunchKernelGGL(k_maxpool3s2_bwd, dim3(grid_for(total)), dim3(kThreads), 0, st, (const _Float16*)x, (const _Float16*)g_out,
                     (_Float16*)g_in, n, h, w, oh, ow, c / 8, accumulate ? 1 : 0);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

int lfd_relu_bwd_add_f16(const void* y, const void* g_a, const void* g_b, void* out, int64_t count, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!y || !g_a || !out || count < 0) return LFD_ERR_INVALID_ARGUMENT;
  if (!lfd_aligned16(y) || !lfd_aligned16(g_a) || !lfd_aligned16(g_b) || !lfd_aligned16(out)) return LFD_ERR_INVALID_ARGUMENT;
  if (count % 8) return LFD_ERR_UNSUPPORTED;
  if (count == 0) return LFD_OK;
  hipLaunchKernelGGL(k_relu_bwd_add, dim3(grid_for(count / 8)), dim3(kThreads), 0, st, (const _Float16*)y, (const _Float16*)g_a,
                     (const _Float16*)g_b, (_Float16*)out, count / 8);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

size_t lfd_bias_grad_workspace_bytes(void) { return (size_t)kBiasMaxBlocks * kBiasMaxChannels * sizeof(float); }

int lfd_bias_grad_nhwc_f16(const void* dy, int64_t rows, int32_t c, float inv_scale, float* dbias, void* workspace,
                           size_t workspace_bytes, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!dy || !dbias || !workspace || rows < 1 || c < 8 || !lfd_aligned16(dy)) return LFD_ERR_INVALID_ARGUMENT;
  if (c != 32 && c != 64 && c != 128) return LFD_ERR_UNSUPPORTED;      // c / 8 must divide the block: a thread keeps its channels
  if (workspace_bytes < lfd_bias_grad_workspace_bytes()) return LFD_ERR_WORKSPACE_TOO_SMALL;
  int64_t nb = (rows * (c / 8) + kThreads - 1) / kThreads;
  nb = nb > kBiasMaxBlocks ? kBiasMaxBlocks : nb;
  float* partials = reinterpret_cast<float*>(workspace);
  hipLaunchKernelGGL(k_bias_grad_partial, dim3((unsigned)nb), dim3(kThreads), 0, st, (const _Float16*)dy, rows, c / 8, partials);
  LFD_CHECK_LAUNCH();
  hipLaunchKernelGGL(k_bias_grad_final, dim3(c), dim3(64), 0, st, partials, (int)nb, c, inv_scale, dbias);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

}  // extern "C"
