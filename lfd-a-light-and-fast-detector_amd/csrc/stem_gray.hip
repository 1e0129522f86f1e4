// csrc/stem_gray.hip -- first stem unit of a one-channel (grayscale) model: conv3x3 stride 2 (Cin = 1) + BN + ReLU, optionally
// chained in the same kernel with the following conv1x1 + BN + ReLU (reference lfd/model/backbone/lfd_resnet.py:356-374 'fast'
// stem, :376-395 first half of the 'faster' stem, with input_channels = 1).
//
// One kernel source, two output forms:
//   PLANES = false: fp16 NHWC [N,OH,OW,C], the layout and numerics of lfd_stem_conv_f16 (csrc/stem.hip): frame values rounded
//                   to fp16 on the load, one MFMA per k-step, the C-channel intermediate rounded to fp16 before the 1x1;
//   PLANES = true:  hi/lo planes (the 'fp32_storage' mode, layout of lfd_pl_stem_pair): weights split into hi + 2^-11 lo, frame
//                   values split on the load (fp16 frames are exact in hi, their lo MFMA is skipped), three MFMAs per k-step
//                   into two fp32 accumulator sets, the fp32 intermediate split into planes before the 1x1.
//
// For one channel NCHW and NHWC are the same bytes, so every frame format reads one [N,H,W] plane: fp32 (the reference's
// tensor API), fp16, uint8 with simple_normalize (x/255 - 0.5)/0.5 in fp32 on the load (augmentation_pipeline.py:31-36).
// K is the 9 taps of one channel: ONE 16-wide k-step of v_mfma_f32_32x32x16_f16 (k = 3 ky + kx; lane half 0 holds k = 0..7,
// half 1 holds k = 8 and seven zero slots), where the RGB kernels need two (K = 27 -> 32).
//
// Tiles: a 3-channel LDS row is 6 B per input pixel, a gray one 2 B, so the tile is twice as wide as csrc/stem.hip's: 64 output
// columns x (4 / NCT) rows, each wave one output row of one 32-channel slab as two 32-pixel MFMA tiles.  The frame patch
// (2 TH + 1 rows x 129 columns) is fetched into registers for the next tile while the current one computes; the output goes
// through a swizzled LDS staging tile to 16-byte coalesced stores (the unit is bound by its output writes).
#include "common.h"

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

enum { IN_F32 = 0, IN_F16 = 1, IN_U8 = 2 };
constexpr float kLo = 2048.f, kInvLo = 1.f / 2048.f;

struct GrayArgs {
  const void* in;      // [N,H,W] in FMT
  _Float16* out;       // [N,OH,OW,C] (PLANES: hi plane; lo plane out_plane halfs behind it)
  long out_plane;
  const half8* w1;     // [C/32][64] packed 3x3 taps (engine.pack_stem_gray_weight); PLANES: [2][C/32][64]
  long w1_plane;
  const float* b1;     // [C]
  const half8* w2;     // TAIL: [C/32][C/16][64] packed 1x1 fragments (ops.pack_conv_weight); PLANES: [2][...]
  long w2_plane;
  const float* b2;     // [C]
  int N, H, W, OH, OW;
  int tiles_x, tiles_y;
};

template <int FMT>
__device__ __forceinline__ uint32_t load_raw(const void* in, size_t i) {
  if (FMT == IN_F32) return reinterpret_cast<const uint32_t*>(in)[i];
  if (FMT == IN_F16) return reinterpret_cast<const uint16_t*>(in)[i];
  return reinterpret_cast<const uint8_t*>(in)[i];
}

template <int FMT>
__device__ __forceinline__ float raw_value(uint32_t raw) {
  if (FMT == IN_F32) return __uint_as_float(raw);
  if (FMT == IN_F16) return (float)__builtin_bit_cast(_Float16, (unsigned short)raw);
  return ((float)raw / 255.f - 0.5f) / 0.5f;
}

// y -> (hi, lo) fp16 with hi = RNE(y), lo = RNE(2^11 (y - hi)): the split of every plane kernel (planes_impl.h split2)
__device__ __forceinline__ void split1(float y, _Float16& hi, _Float16& lo) {
  hi = (_Float16)y;
  lo = (_Float16)((y - (float)hi) * kLo);
}

template <int NCT, int FMT, bool TAIL, bool PLANES>
__global__ __launch_bounds__(256) void k_stem_gray(GrayArgs a) {
  constexpr bool HASLO = PLANES && FMT != IN_F16;
  constexpr int NPL = PLANES ? 2 : 1;                 // planes of the intermediate / staging tile
  constexpr int C = NCT * 32;
  constexpr int TH = 4 / NCT, TW = 64, PT = TW / 32;
  constexpr int IH = 2 * TH + 1, IW = 2 * TW + 1;
  constexpr int RS = IW + 1;                          // halfs per LDS input row
  constexpr int MCPP = C / 8, MPIXB = C * 2, MPPR = 16 / MCPP;
  constexpr int MID_PLANE = TH * TW * MPIXB;
  constexpr int NE = IH * IW;
  constexpr int NIT = (NE + 255) / 256;
  __shared__ __attribute__((aligned(16))) _Float16 s_in[HASLO ? 2 : 1][IH * RS];
  __shared__ __attribute__((aligned(16))) char s_mid[NPL * MID_PLANE];

  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int ct = wave % NCT, oy = wave / NCT;         // this wave's channel slab and tile row
  const int h = lane >> 5, pix = lane & 31;
  const int tiles_per_img = a.tiles_x * a.tiles_y;
  const int ntiles = a.N * tiles_per_img;

  const half8 w1h = a.w1[ct * 64 + lane];
  const half8 w1l = PLANES ? a.w1[a.w1_plane + ct * 64 + lane] : w1h;
  half8 w2h[TAIL ? C / 16 : 1], w2l[(TAIL && PLANES) ? C / 16 : 1];
  if (TAIL) {
#pragma unroll
    for (int q = 0; q < C / 16; ++q) {
      w2h[q] = a.w2[(ct * (C / 16) + q) * 64 + lane];
      if (PLANES) w2l[q] = a.w2[a.w2_plane + (ct * (C / 16) + q) * 64 + lane];
    }
  }

  // raw frame patch in registers: unconditional loads from clamped addresses, the in-image bit kept aside (a branch around a
  // load makes the compiler wait for each element separately); issued one tile ahead
  uint32_t rv[NIT];
  uint32_t rok = 0;
  auto fetch = [&](int t) {
    const int n = t / tiles_per_img;
    const int tr = t - n * tiles_per_img;
    const int ty0 = tr / a.tiles_x, tx0 = tr - ty0 * a.tiles_x;
    const int gy0 = ty0 * TH * 2 - 1, gx0 = tx0 * TW * 2 - 1;
    rok = 0;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = it * 256 + (int)threadIdx.x;
      const int iy = i / IW, ix = i - iy * IW;
      const int gy = gy0 + iy, gx = gx0 + ix;
      const bool ok = i < NE && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
      const int cy = gy < 0 ? 0 : (gy >= a.H ? a.H - 1 : gy), cx = gx < 0 ? 0 : (gx >= a.W ? a.W - 1 : gx);
      rv[it] = load_raw<FMT>(a.in, ((size_t)n * a.H + cy) * a.W + cx);
      rok |= ok ? (1u << it) : 0u;
    }
  };

  auto bias_init = [&](f32x16& m, const float* bias) {
    const float* bp = bias + ct * 32 + 4 * h;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const float4 b4 = *reinterpret_cast<const float4*>(bp + 8 * g);
      m[4 * g + 0] = b4.x; m[4 * g + 1] = b4.y; m[4 * g + 2] = b4.z; m[4 * g + 3] = b4.w;
    }
  };
  // accumulator tile pt -> ReLU -> fp16 (PLANES: hi / lo) into the swizzled [pixel][C] tile (channel 8 g + 4 h + e of the slab)
  auto to_lds = [&](const f32x16& m, const f32x16& c, int pt) {
    const int pb = oy * TW + pt * 32 + pix;
    const int fm = (pb / MPPR) % MCPP;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int o = pb * MPIXB + (((ct * 4 + g) ^ fm) * 16) + 8 * h;
      if constexpr (PLANES) {
        union { _Float16 e[4]; uint2 u; } vh, vl;
#pragma unroll
        for (int e = 0; e < 4; ++e) split1(fmaxf(fmaf(c[4 * g + e], kInvLo, m[4 * g + e]), 0.f), vh.e[e], vl.e[e]);
        *reinterpret_cast<uint2*>(s_mid + o) = vh.u;
        *reinterpret_cast<uint2*>(s_mid + MID_PLANE + o) = vl.u;
      } else {
        uint2 v;
        v.x = lfd_cvt_pk_max(m[4 * g + 0], m[4 * g + 1], LFD_PK_RELU);
        v.y = lfd_cvt_pk_max(m[4 * g + 2], m[4 * g + 3], LFD_PK_RELU);
        *reinterpret_cast<uint2*>(s_mid + o) = v;
      }
    }
  };
  // im2col fragment of output column 32 pt + pix (tile-local) from an LDS frame plane
  auto gather = [&](const _Float16* plane, int pt) {
    const _Float16* b = plane + (2 * oy) * RS + 2 * (pt * 32 + pix);
    const _Float16 z = (_Float16)0.f;
    half8 f;
    f[0] = b[h ? 2 * RS + 2 : 0];
    f[1] = h ? z : b[1];
    f[2] = h ? z : b[2];
    f[3] = h ? z : b[RS];
    f[4] = h ? z : b[RS + 1];
    f[5] = h ? z : b[RS + 2];
    f[6] = h ? z : b[2 * RS];
    f[7] = h ? z : b[2 * RS + 1];
    return f;
  };

  int t = blockIdx.x;
  if (t < ntiles) fetch(t);
  for (; t < ntiles; t += gridDim.x) {
    const int n = t / tiles_per_img;
    const int tr = t - n * tiles_per_img;
    const int ty0 = tr / a.tiles_x, tx0 = tr - ty0 * a.tiles_x;
    __syncthreads();   // the previous tile's readers of s_in / s_mid are done
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = it * 256 + (int)threadIdx.x;
      if (i < NE) {
        const int iy = i / IW, ix = i - iy * IW;
        const float v = ((rok >> it) & 1u) ? raw_value<FMT>(rv[it]) : 0.f;
        if constexpr (HASLO) {
          _Float16 hi, lo;
          split1(v, hi, lo);
          s_in[0][iy * RS + ix] = hi;
          s_in[1][iy * RS + ix] = lo;
        } else {
          s_in[0][iy * RS + ix] = (_Float16)v;
        }
      }
    }
    __syncthreads();
    if (t + (int)gridDim.x < ntiles) fetch(t + gridDim.x);

    f32x16 accm[PT], accc[PT];
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
      bias_init(accm[pt], a.b1);
      const half8 xh = gather(s_in[0], pt);
      accm[pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w1h, xh, accm[pt], 0, 0, 0);
      if constexpr (PLANES) {
#pragma unroll
        for (int r = 0; r < 16; ++r) accc[pt][r] = 0.f;
        accc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w1l, xh, accc[pt], 0, 0, 0);
        if constexpr (HASLO) {
          const half8 xl = gather(s_in[1], pt);
          accc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w1h, xl, accc[pt], 0, 0, 0);
        }
      }
    }

    if constexpr (TAIL) {
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) to_lds(accm[pt], accc[pt], pt);
      __syncthreads();
#pragma unroll
      for (int pt = 0; pt < PT; ++pt) {
        bias_init(accm[pt], a.b2);
        if constexpr (PLANES) {
#pragma unroll
          for (int r = 0; r < 16; ++r) accc[pt][r] = 0.f;
        }
        const int pb = oy * TW + pt * 32 + pix;
        const int fm = (pb / MPPR) % MCPP;
#pragma unroll
        for (int q = 0; q < C / 16; ++q) {
          const int o = pb * MPIXB + (((2 * q + h) ^ fm) * 16);
          const half8 xh = *reinterpret_cast<const half8*>(s_mid + o);
          accm[pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w2h[q], xh, accm[pt], 0, 0, 0);
          if constexpr (PLANES) {
            const half8 xl = *reinterpret_cast<const half8*>(s_mid + MID_PLANE + o);
            accc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w2h[q], xl, accc[pt], 0, 0, 0);
            accc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(w2l[q], xh, accc[pt], 0, 0, 0);
          }
        }
      }
      __syncthreads();   // every wave finished reading s_mid: it becomes the staging tile
    }
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) to_lds(accm[pt], accc[pt], pt);
    __syncthreads();
    for (int i = threadIdx.x; i < TH * TW * MCPP; i += 256) {
      const int pb = i / MCPP, c = i - pb * MCPP;
      const int oyg = ty0 * TH + pb / TW, oxg = tx0 * TW + pb % TW;
      if (oyg < a.OH && oxg < a.OW) {
        const int fm = (pb / MPPR) % MCPP;
        const int o = pb * MPIXB + ((c ^ fm) * 16);
        _Float16* dst = a.out + (((size_t)n * a.OH + oyg) * a.OW + oxg) * C + c * 8;
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(s_mid + o);
        if (PLANES) *reinterpret_cast<uint4*>(dst + a.out_plane) = *reinterpret_cast<const uint4*>(s_mid + MID_PLANE + o);
      }
    }
  }  // persistent tile loop
}

template <int NCT, int FMT, bool TAIL, bool PLANES>
int launch_gray(GrayArgs a, hipStream_t st) {
  constexpr int TH = 4 / NCT, TW = 64;
  a.tiles_x = (a.OW + TW - 1) / TW;
  a.tiles_y = (a.OH + TH - 1) / TH;
  const long long ntiles = (long long)a.N * a.tiles_x * a.tiles_y;
  if (ntiles > 0x7fffffffLL) return LFD_ERR_UNSUPPORTED;
  const unsigned blocks = ntiles < 2048 ? (unsigned)ntiles : 2048u;   // 8 resident workgroups per CU
  hipLaunchKernelGGL((k_stem_gray<NCT, FMT, TAIL, PLANES>), dim3(blocks), dim3(256), 0, st, a);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

template <bool PLANES>
int dispatch_gray(int fmt, int channels, bool tail, const GrayArgs& a, hipStream_t st) {
#define LFD_GRAY_CASE(NCT, FMT)                                                                                     \
  return tail ? launch_gray<NCT, FMT, true, PLANES>(a, st) : launch_gray<NCT, FMT, false, PLANES>(a, st)
  if (channels == 64) {
    switch (fmt) {
      case IN_F32: LFD_GRAY_CASE(2, IN_F32);
      case IN_F16: LFD_GRAY_CASE(2, IN_F16);
      case IN_U8: LFD_GRAY_CASE(2, IN_U8);
      default: return LFD_ERR_INVALID_ARGUMENT;
    }
  }
  switch (fmt) {
    case IN_F32: LFD_GRAY_CASE(1, IN_F32);
    case IN_F16: LFD_GRAY_CASE(1, IN_F16);
    case IN_U8: LFD_GRAY_CASE(1, IN_U8);
    default: return LFD_ERR_INVALID_ARGUMENT;
  }
#undef LFD_GRAY_CASE
}

int check_gray_args(const void* in, int32_t in_format, int32_t n, int32_t h, int32_t w, int32_t channels, const void* w1,
                    const float* b1, const void* w2, const float* b2, const void* out) {
  if (!in || !w1 || !b1 || !out || n < 1 || h < 1 || w < 1) return LFD_ERR_INVALID_ARGUMENT;
  if ((w2 != nullptr) != (b2 != nullptr)) return LFD_ERR_INVALID_ARGUMENT;
  if (in_format < IN_F32 || in_format > IN_U8) return LFD_ERR_INVALID_ARGUMENT;
  if (!lfd_aligned16(out) || !lfd_aligned16(b1) || (b2 && !lfd_aligned16(b2))) return LFD_ERR_INVALID_ARGUMENT;
  if (channels != 32 && channels != 64) return LFD_ERR_UNSUPPORTED;
  return LFD_OK;
}

}  // namespace

extern "C" {

int lfd_stem_gray_f16(const void* in, int32_t in_format, int32_t n, int32_t h, int32_t w, int32_t channels,
                      const void* w1_packed, const float* b1, const void* w2_packed, const float* b2, void* out,
                      lfd_stream_t stream) {
  const int s = check_gray_args(in, in_format, n, h, w, channels, w1_packed, b1, w2_packed, b2, out);
  if (s != LFD_OK) return s;
  GrayArgs a{};
  a.in = in; a.out = (_Float16*)out;
  a.w1 = (const half8*)w1_packed; a.b1 = b1; a.w2 = (const half8*)w2_packed; a.b2 = b2;
  a.N = n; a.H = h; a.W = w; a.OH = (h + 2 - 3) / 2 + 1; a.OW = (w + 2 - 3) / 2 + 1;
  return dispatch_gray<false>(in_format, channels, w2_packed != nullptr, a, reinterpret_cast<hipStream_t>(stream));
}

int lfd_pl_stem_gray_pair(const void* in, int32_t in_format, int32_t n, int32_t h, int32_t w, int32_t channels,
                          const void* w1_packed, const float* b1, const void* w2_packed, const float* b2, void* out,
                          int64_t out_plane_halfs, lfd_stream_t stream) {
  const int s = check_gray_args(in, in_format, n, h, w, channels, w1_packed, b1, w2_packed, b2, out);
  if (s != LFD_OK) return s;
  if (out_plane_halfs & 7) return LFD_ERR_INVALID_ARGUMENT;
  const long oh = (h + 2 - 3) / 2 + 1, ow = (w + 2 - 3) / 2 + 1;
  if (out_plane_halfs < (long long)n * oh * ow * channels) return LFD_ERR_INVALID_ARGUMENT;   // the planes may not overlap
  GrayArgs a{};
  a.in = in; a.out = (_Float16*)out; a.out_plane = out_plane_halfs;
  a.w1 = (const half8*)w1_packed; a.w1_plane = (long)(channels / 32) * 64; a.b1 = b1;
  a.w2 = (const half8*)w2_packed; a.w2_plane = (long)(channels / 32) * (channels / 16) * 64; a.b2 = b2;
  a.N = n; a.H = h; a.W = w; a.OH = (int)oh; a.OW = (int)ow;
  return dispatch_gray<true>(in_format, channels, w2_packed != nullptr, a, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
