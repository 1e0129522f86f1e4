// csrc/stem7.hip -- the torchvision-style ResNet's first layer: conv7x7 stride 2 pad 3 (3 -> 64) + BatchNorm (folded on
// the host) + ReLU on a frame (reference lfd/model/backbone/resnet.py:366-370, :470-473).  The 3x3 s2 max-pool that follows
// stays lfd_maxpool3x3s2_nhwc_f16 (csrc/sibling.hip).
//
// K = 7 * 7 * 3 = 147 taps, zero-padded to ten k-steps of v_mfma_f32_32x32x16_f16 (160), fp32 accumulation.  As in k_stem
// (csrc/stem.hip) the im2col is done from an LDS copy of the raw 3-channel tile: a filter row of an output pixel is 21
// contiguous halfs e = 3 * kx + c there.  k-slot order (the packed filter has the same, engine_resnet.pack_stem7_weight):
//   k-step s = 0..6, half h:  filter row s, e = 8 h .. 8 h + 7                     (one 16-byte run per lane)
//   k-step s = 7..9, half h:  the 35 left-over taps i = 8 (2 (s - 7) + h) + j  ->  filter row i / 5, e = 16 + i % 5;  i >= 35: 0
// The 64 x 160 filter (20 KB) is stationary in registers: a wave owns 32 output channels, 10 fragments = 40 VGPRs.
//
// Persistent grid over (image, tile of 4 x 32 output pixels); the NEXT tile's raw fetch is issued before the current tile's
// MFMAs (unconditional loads from clamped addresses + select).  The output (the kernel is write-bound: 64 channels per
// pixel against 3 read) leaves through LDS as whole 128-byte pixel lines, 16 bytes per lane.
//
// Frame formats: NCHW fp32, NHWC fp16, NHWC uint8 with the reference's simple_normalize (x/255-0.5)/0.5 on the load -- the
// expression of k_stem's load_px.
#include "common.h"

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

enum { IN_NCHW_F32 = 0, IN_NHWC_F16 = 1, IN_NHWC_U8 = 2 };
enum { KSTEPS = 10, MAX_WGS = 512 };        // 2 resident workgroups per CU (VGPR-bound: 2 waves per SIMD) on 256 CUs

struct Stem7Args {
  const void* in;
  _Float16* out;       // [N,OH,OW,64]
  const half8* w;      // [2][KSTEPS][64] fragments
  const float* b;      // [64]
  int N, H, W, OH, OW;
  int tiles_x, tiles_y;
};

template <int FMT>
__device__ __forceinline__ _Float16 load_px(const void* in, int n, int H, int W, int gy, int gx, int c) {
  if (FMT == IN_NCHW_F32) {
    return (_Float16) reinterpret_cast<const float*>(in)[(((size_t)n * 3 + c) * H + gy) * W + gx];
  } else if (FMT == IN_NHWC_F16) {
    return reinterpret_cast<const _Float16*>(in)[(((size_t)n * H + gy) * W + gx) * 3 + c];
  } else {
    const float v = (float)reinterpret_cast<const uint8_t*>(in)[(((size_t)n * H + gy) * W + gx) * 3 + c];
    return (_Float16)((v / 255.f - 0.5f) / 0.5f);
  }
}

// 4 waves: ct = wave % 2 (32 output channels), pg = wave / 2; each wave: 2 output rows x 32 px x 32 ch.
template <int FMT>
__global__ __launch_bounds__(256) void k_stem7(Stem7Args a) {
  constexpr int C = 64, PG = 2, PT = 2, TW = 32, TH = PG * PT;
  constexpr int IH = 2 * TH + 5, IW = 2 * TW + 5;       // 13 x 69 raw pixels
  constexpr int RS = ((IW * 3 + 1) / 2) * 2;            // halfs per LDS input row (even): 208
  constexpr int OUT_HALFS = TH * TW * C;
  constexpr int IN_HALFS = OUT_HALFS > IH * RS + 8 ? OUT_HALFS : IH * RS + 8;
  constexpr int MCPP = C / 8, MPIXB = C * 2, MPPR = 16 / MCPP;
  __shared__ __attribute__((aligned(16))) _Float16 s_in[IN_HALFS];      // the raw tile, then the output tile

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int ct = wave & 1, pg = wave >> 1;
  const int h = lane >> 5, pix = lane & 31;
  const int tiles_per_img = a.tiles_x * a.tiles_y;
  const int ntiles = a.N * tiles_per_img;
  constexpr int NE = IH * IW * 3;
  constexpr int NIT = (NE + 255) / 256;

  half8 wr[KSTEPS];
#pragma unroll
  for (int s = 0; s < KSTEPS; ++s) wr[s] = a.w[(ct * KSTEPS + s) * 64 + lane];

  _Float16 rv[NIT];
  auto fetch = [&](int t) {
    const int n = t / tiles_per_img;
    const int tr = t - n * tiles_per_img;
    const int ty0 = tr / a.tiles_x, tx0 = tr - ty0 * a.tiles_x;
    const int gy0 = ty0 * TH * 2 - 3, gx0 = tx0 * TW * 2 - 3;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = it * 256 + threadIdx.x;
      const int iy = i / (IW * 3), e = i - iy * (IW * 3);
      const int ix = e / 3, c = e - ix * 3;
      const int gy = gy0 + iy, gx = gx0 + ix;
      const bool ok = i < NE && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
      const int cy = gy < 0 ? 0 : (gy >= a.H ? a.H - 1 : gy), cx = gx < 0 ? 0 : (gx >= a.W ? a.W - 1 : gx);
      const _Float16 v = load_px<FMT>(a.in, n, a.H, a.W, cy, cx, c);
      rv[it] = ok ? v : (_Float16)0.f;
    }
  };

  int t = blockIdx.x;
  if (t < ntiles) fetch(t);
  for (; t < ntiles; t += gridDim.x) {
    const int n = t / tiles_per_img;
    const int tr = t - n * tiles_per_img;
    const int ty0 = tr / a.tiles_x, tx0 = tr - ty0 * a.tiles_x;
    __syncthreads();   // the previous tile's output lines have left s_in
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = it * 256 + threadIdx.x;
      const int iy = i / (IW * 3), e = i - iy * (IW * 3);
      if (i < NE) s_in[iy * RS + e] = rv[it];
    }
    __syncthreads();
    if (t + (int)gridDim.x < ntiles) fetch(t + gridDim.x);

    f32x16 acc[PT];
    {
      const float* bp = a.b + ct * 32 + 4 * h;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 b4 = *reinterpret_cast<const float4*>(bp + 8 * g);
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) {
          acc[pt][4 * g + 0] = b4.x; acc[pt][4 * g + 1] = b4.y; acc[pt][4 * g + 2] = b4.z; acc[pt][4 * g + 3] = b4.w;
        }
      }
    }
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      const int oy = pg * PT + pt;
      const _Float16* base = s_in + (2 * oy) * RS + 6 * pix;     // raw pixel (2 oy, 2 pix) channel 0: filter tap (0, 0)
#pragma unroll
      for (int s = 0; s < 7; ++s) {
        union { half8 v; uint32_t u[4]; } f;
        const uint32_t* p = reinterpret_cast<const uint32_t*>(base + s * RS + 8 * h);
        f.u[0] = p[0]; f.u[1] = p[1]; f.u[2] = p[2]; f.u[3] = p[3];
        acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wr[s], f.v, acc[pt], 0, 0, 0);
      }
#pragma unroll
      for (int s = 7; s < KSTEPS; ++s) {
        half8 f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int i = 8 * (2 * (s - 7) + h) + j;               // < 48
          const int ic = i < 35 ? i : 34;
          const int r = ic / 5;
          const _Float16 v = base[r * RS + 16 + (ic - 5 * r)];
          f[j] = i < 35 ? v : (_Float16)0.f;
        }
        acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wr[s], f, acc[pt], 0, 0, 0);
      }
    }

    // ---- epilogue: ReLU -> fp16 -> LDS (swizzled [pixel][64]) -> whole-line 16-byte stores, ragged tiles guarded
    __syncthreads();   // every wave has read its taps: the raw tile's storage takes the output tile
    char* s_out = reinterpret_cast<char*>(s_in);
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      const int pb = (pg * PT + pt) * 32 + pix;
      const int fm = (pb / MPPR) % MCPP;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        uint2 v;
        v.x = lfd_cvt_pk_max(acc[pt][4 * g + 0], acc[pt][4 * g + 1], LFD_PK_RELU);
        v.y = lfd_cvt_pk_max(acc[pt][4 * g + 2], acc[pt][4 * g + 3], LFD_PK_RELU);
        *reinterpret_cast<uint2*>(s_out + pb * MPIXB + (((ct * 4 + g) ^ fm) * 16) + 8 * h) = v;
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < TH * TW * MCPP; i += 256) {
      const int pb = i / MCPP, c = i - pb * MCPP;
      const int oy = ty0 * TH + pb / TW, ox = tx0 * TW + (pb % TW);
      if (oy < a.OH && ox < a.OW) {
        const int fm = (pb / MPPR) % MCPP;
        const uint4 v = *reinterpret_cast<const uint4*>(s_out + pb * MPIXB + ((c ^ fm) * 16));
        *reinterpret_cast<uint4*>(a.out + (((size_t)n * a.OH + oy) * a.OW + ox) * C + c * 8) = v;
      }
    }
  }  // persistent tile loop
}

template <int FMT>
int launch_stem7(Stem7Args a, hipStream_t st) {
  constexpr int TH = 4, TW = 32;
  a.tiles_x = (a.OW + TW - 1) / TW;
  a.tiles_y = (a.OH + TH - 1) / TH;
  const long long ntiles = (long long)a.N * a.tiles_x * a.tiles_y;
  if (ntiles > 0x7fffffffLL - MAX_WGS) return LFD_ERR_UNSUPPORTED;      // the tile loop adds the grid size to an int index
  const unsigned blocks = ntiles < MAX_WGS ? (unsigned)ntiles : (unsigned)MAX_WGS;
  hipLaunchKernelGGL((k_stem7<FMT>), dim3(blocks), dim3(256), 0, st, a);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

}  // namespace

extern "C" {

size_t lfd_stem7_packed_weight_halfs(void) { return (size_t)2 * KSTEPS * 64 * 8; }

int lfd_stem7_conv_f16(const void* in, int32_t in_format, int32_t n, int32_t h, int32_t w, const void* w_packed,
                       const float* bias, void* out, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!in || !w_packed || !bias || !out || n < 1 || h < 1 || w < 1) return LFD_ERR_INVALID_ARGUMENT;
  if (in_format < 0 || in_format > 2) return LFD_ERR_INVALID_ARGUMENT;
  if (!lfd_aligned16(out) || !lfd_aligned16(w_packed) || !lfd_aligned16(bias)) return LFD_ERR_INVALID_ARGUMENT;
  Stem7Args a{};
  a.in = in; a.out = (_Float16*)out; a.w = (const half8*)w_packed; a.b = bias;
  a.N = n; a.H = h; a.W = w; a.OH = (h + 6 - 7) / 2 + 1; a.OW = (w + 6 - 7) / 2 + 1;
  switch (in_format) {
    case IN_NCHW_F32: return launch_stem7<IN_NCHW_F32>(a, st);
    case IN_NHWC_F16: return launch_stem7<IN_NHWC_F16>(a, st);
    default: return launch_stem7<IN_NHWC_U8>(a, st);
  }
}

}  // extern "C"
