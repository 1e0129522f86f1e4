// csrc/precise_pyramid.hip -- the pyramid arithmetic of the 'fp32_storage' precision mode in its fp32-tensor form
// (lfd_amd/engine_sibling_p32.py): what an FPN / SimpleFPN neck and an FCOSHead do between the convolutions of
// csrc/precise.hip, on dense fp32 NHWC tensors -- the fp32 twins of csrc/sibling.hip:
//   * top-down (or bottom-up) merge `lateral[i-1] += nn.Upsample(size, mode='nearest')(lateral[i])` (fpn.py:127-135,
//     simple_fpn.py:141-157) for the laterals whose conv does not carry the merge in its epilogue
//     (lfd_p32_conv2d_merge_nhwc_f32, csrc/precise.hip: same index expression, same fp32 add, same bits);
//   * nn.ReLU(inplace=True) in front of an extra level and the 'pooling' extra level nn.MaxPool2d(3, 2, 1)
//     (fpn.py:66-79,136-152, simple_fpn.py:84-99,158-172);
//   * `scales[i](conv).float().exp()` of FCOSHead's regression output (fcos_head.py:129-154): the conv and the Scale are
//     the epilogue of lfd_p32_conv2d_nhwc_f32, which writes the level's rows of the level-concatenated [N,P,4] tensor; expf
//     runs in place on those rows.
// All HBM-bound streaming kernels: one float4 per lane and step, grid-stride loops, 64-bit element counts.
#include "common.h"

namespace {

// dst[n,y,x,:] += src[n, sy(y), sx(x), :]; source index = min(floorf(dst_index * float(in)/out), in-1) as ATen's
// upsample_nearest2d computes it for nn.Upsample(size=...) (the rule of csrc/sibling.hip k_upsample_add)
__global__ __launch_bounds__(256) void k_p32_upsample_add(float* dst, const float* src, int N, int H, int W, int h, int w,
                                                          int c4, float sy, float sx) {
  const int64_t total = (int64_t)N * H * W * c4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int q = (int)(i % c4);
    int64_t t = i / c4;
    const int x = (int)(t % W);
    t /= W;
    const int y = (int)(t % H);
    const int n = (int)(t / H);
    int yy = (int)floorf((float)y * sy), xx = (int)floorf((float)x * sx);
    yy = yy < h - 1 ? yy : h - 1;
    xx = xx < w - 1 ? xx : w - 1;
    float4 a = reinterpret_cast<const float4*>(dst)[i];
    const float4 b = reinterpret_cast<const float4*>(src)[(((int64_t)n * h + yy) * w + xx) * c4 + q];
    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
    reinterpret_cast<float4*>(dst)[i] = a;
  }
}

__global__ __launch_bounds__(256) void k_p32_relu(float* x, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    float4 v = reinterpret_cast<float4*>(x)[i];
    v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f);   // the conv epilogue's ReLU
    reinterpret_cast<float4*>(x)[i] = v;
  }
}

// F.max_pool2d(x, 3, 2, 1): the padding never wins (-inf), a NaN in the window does (ATen: `val > max || isnan(val)`)
__device__ __forceinline__ float pool_max(float m, float v) { return (v > m || v != v) ? v : m; }

__global__ __launch_bounds__(256) void k_p32_maxpool3s2(const float* in, float* out, int N, int H, int W, int OH, int OW,
                                                        int c4) {
  const int64_t total = (int64_t)N * OH * OW * c4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int q = (int)(i % c4);
    int64_t t = i / c4;
    const int ox = (int)(t % OW);
    t /= OW;
    const int oy = (int)(t % OH);
    const int n = (int)(t / OH);
    float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    for (int dy = 0; dy < 3; ++dy) {
      const int y = oy * 2 - 1 + dy;
      if (y < 0 || y >= H) continue;
      for (int dx = 0; dx < 3; ++dx) {
        const int x = ox * 2 - 1 + dx;
        if (x < 0 || x >= W) continue;
        const float4 v = reinterpret_cast<const float4*>(in)[(((int64_t)n * H + y) * W + x) * c4 + q];
        m.x = pool_max(m.x, v.x); m.y = pool_max(m.y, v.y); m.z = pool_max(m.z, v.z); m.w = pool_max(m.w, v.w);
      }
    }
    reinterpret_cast<float4*>(out)[i] = m;
  }
}

// out[img * image_stride + (row0 + r) * c + j] = expf(same), r < rows, j < c: one level's rows of every image
__global__ __launch_bounds__(256) void k_p32_exp_rows(float* out, int N, int64_t image_stride, int64_t row0, int64_t rows,
                                                      int c4) {
  const int64_t per = rows * c4, total = (int64_t)N * per;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i / per, k = i - n * per;
    float4* p = reinterpret_cast<float4*>(out + n * image_stride + row0 * c4 * 4) + k;
    float4 v = *p;
    v.x = expf(v.x); v.y = expf(v.y); v.z = expf(v.z); v.w = expf(v.w);     // expf, not the fast intrinsic
    *p = v;
  }
}

inline unsigned grid_for(int64_t total) {
  int64_t b = (total + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

}  // namespace

extern "C" {

int lfd_p32_upsample_nearest_add_f32(float* dst, const float* src, int32_t n, int32_t H, int32_t W, int32_t h, int32_t w,
                                     int32_t c, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!dst || !src || dst == src || n < 1 || H < 1 || W < 1 || h < 1 || w < 1 || c < 4) return LFD_ERR_INVALID_ARGUMENT;
  if (h > H || w > W || !lfd_aligned16(dst) || !lfd_aligned16(src)) return LFD_ERR_INVALID_ARGUMENT;
  if (c % 4) return LFD_ERR_UNSUPPORTED;
  const int64_t total = (int64_t)n * H * W * (c / 4);
  hipLaunchKernelGGL(k_p32_upsample_add, dim3(grid_for(total)), dim3(256), 0, st, dst, src, n, H, W, h, w, c / 4,
                     (float)h / (float)H, (float)w / (float)W);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

int lfd_p32_relu_f32(float* x, int64_t count, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!x || count < 0 || !lfd_aligned16(x)) return LFD_ERR_INVALID_ARGUMENT;
  if (count % 4) return LFD_ERR_UNSUPPORTED;
  if (count == 0) return LFD_OK;
  hipLaunchKernelGGL(k_p32_relu, dim3(grid_for(count / 4)), dim3(256), 0, st, x, count / 4);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

int lfd_p32_maxpool3x3s2_f32(const float* in, float* out, int32_t n, int32_t h, int32_t w, int32_t c, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!in || !out || in == out || n < 1 || h < 1 || w < 1 || c < 4 || !lfd_aligned16(in) || !lfd_aligned16(out))
    return LFD_ERR_INVALID_ARGUMENT;
  if (c % 4) return LFD_ERR_UNSUPPORTED;
  const int oh = (h + 2 - 3) / 2 + 1, ow = (w + 2 - 3) / 2 + 1;
  const int64_t total = (int64_t)n * oh * ow * (c / 4);
  hipLaunchKernelGGL(k_p32_maxpool3s2, dim3(grid_for(total)), dim3(256), 0, st, in, out, n, h, w, oh, ow, c / 4);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

int lfd_p32_exp_rows_f32(float* out, int32_t n, int64_t image_stride, int64_t row0, int64_t rows, int32_t c,
                         lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!out || n < 1 || row0 < 0 || rows < 0 || c < 4 || !lfd_aligned16(out)) return LFD_ERR_INVALID_ARGUMENT;
  if ((row0 + rows) * c > image_stride) return LFD_ERR_INVALID_ARGUMENT;       // the slice lies inside one image
  if (c % 4 || image_stride % 4) return LFD_ERR_UNSUPPORTED;
  if (rows == 0) return LFD_OK;
  const int64_t total = (int64_t)n * rows * (c / 4);
  hipLaunchKernelGGL(k_p32_exp_rows, dim3(grid_for(total)), dim3(256), 0, st, out, n, image_stride, row0, rows, c / 4);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

}  // extern "C"
