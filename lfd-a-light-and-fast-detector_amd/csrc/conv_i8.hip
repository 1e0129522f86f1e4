// csrc/conv_i8.hip -- the INT8 deployment mode's kernels: NHWC int8 conv of the residual stages with the
// requantising epilogue, and the fp16 -> int8 quantise step behind the stem.  Replaces what the reference gets from TensorRT's
// INT8 engine (lfd/deployment/tensorrt/build_engine.py:22-126: INT8Calibrator + BuilderFlag.INT8).
//
// lfd_conv2d_nhwc_i8: ks 1 | 3, stride 1 | 2, pad ks / 2, cin and cout in {64, 128}; v_mfma_i32_32x32x32_i8, exact i32
// accumulation (|acc| <= 9 * 128 * 127^2 < 2^31), so no summation order has to be fixed.
//   * A = filter (MFMA rows = output channels), B = input pixels (MFMA columns = pixels).  A k-step is 32 input channels of one
//     tap: lane (h = lane >> 5, r = lane & 31) holds the 16 bytes "channels 32 q + 16 h + 0..15" of filter row r (A) and of
//     pixel r (B).  Both operands use the SAME (h, byte) -> channel assignment, and the instruction pairs byte j of lane half h
//     of A with byte j of lane half h of B, so the sum covers each of the 32 channels once whatever k index the hardware gives
//     a (h, j) slot; the exact tests (asymmetric full-range operands) are the check of that pairing.
//   * C/D map (the f16 32x32 one): register g of lane (h, p) is MFMA row (g & 3) + 8 (g >> 2) + 4 h of pixel p.  The packed
//     filter (ops.pack_conv_weight_i8) puts output channel 32 slab + 16 h + g on that row, so a lane ends with 16 consecutive
//     channels of its pixel: one 16-byte store of int8, two of fp16, four float4 loads of each constant.
//   * a workgroup (4 waves) owns TH x 16 output pixels -- stride 1: 8 rows = four MFMA tiles of 2 rows, wave w is tile w and
//     every 32-channel slab of cout; stride 2: 4 rows = two tiles, wave w is tile w & 1 and half the slabs -- and stages the
//     input halo once through LDS (a pixel is cin bytes + 16 of bank spread); a 1x1 stride-2 conv stages only the pixels it
//     reads.  One 16-byte LDS read is a lane's k-fragment.  The halo of a workgroup's next tile travels from memory into
//     registers while the current one is contracted.  The filter never enters LDS: where a wave's fragments fit in 160
//     registers (every 1x1 layer, 64 -> 64 3x3, the 3x3 stride-2 layers from 64 channels) they are read once per workgroup
//     and stay; the other layers read them per tile in k-step order (<= 144 KB per layer, cache resident).
//   * workgroups walk (image, tile) with stride gridDim.x (at most CI8_MAX_WORKGROUPS); ragged tiles are guarded on the store,
//     halo pixels outside the image are loads from a clamped address plus a select.
// Epilogue: v = fmaf(acc, mult[co], biasq[co]); with res: v = fmaf(q_res, res_mult, v); with relu: v = max(v, 0);
// out_i8 = clamp(rint(v), -127, 127) (round half even); out_f16 (a tap) = half(v * out_scale), the un-requantised value, with
// this v evaluated in float64 (see the epilogue).
// Addressing: the image base is a 64-bit scalar, offsets inside an image are 32-bit (h * w * 128 < 2^31 is checked).
#include "common.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int CI8_MAX_WORKGROUPS = 1024;
constexpr int Q8_MAX_WORKGROUPS = 1024;

struct CI8Args {
  const int8_t* in;       // [N,H,W,cin]
  const i32x4* w;         // packed [cout/32][ks*ks*cin/32][64 lanes]
  const float* mult;      // [cout]
  const float* biasq;     // [cout]
  const int8_t* res;      // [N,OH,OW,cout] or NULL
  int8_t* out_i8;         // [N,OH,OW,cout]
  _Float16* out_f16;      // [N,OH,OW,cout] or NULL
  float res_mult, out_scale;
  int N, H, W, OH, OW, relu;
  int tiles_x, tiles_y, ntiles;
};

template <int CIN, int COUT, int KS, int S>
struct CI8Cfg {
  static constexpr int TH = S == 1 ? 8 : 4, TW = 16;    // output tile; MFMA tile pt = rows 2 pt, 2 pt + 1
  static constexpr int PT = TH / 2;                      // MFMA pixel tiles per workgroup
  static constexpr int CGN = 4 / PT;                     // channel groups (waves per pixel tile)
  static constexpr int NSLAB = COUT / 32 / CGN;          // 32-channel slabs per wave
  static constexpr int PAD = KS / 2;
  static constexpr int LS = KS == 1 ? 1 : S;             // stride between output pixels inside the LDS tile
  static constexpr int IH = (TH - 1) * LS + KS, IW = (TW - 1) * LS + KS;
  static constexpr int NPIX = IH * IW;
  static constexpr int PITCH = CIN + 16;                 // bytes per LDS pixel
  static constexpr int PIECES = NPIX * (CIN / 16);       // 16-byte pieces of the halo
  static constexpr int NIT = (PIECES + 255) / 256;
  static constexpr int NQ = CIN / 32;                    // k-steps per tap
  static constexpr int NT = KS * KS;
  static constexpr int LDS_BYTES = NPIX * PITCH;
  static_assert(LDS_BYTES <= 64 * 1024, "static LDS");
  static_assert(NSLAB >= 1, "a wave owns at least one slab");
  static constexpr bool STAT = NT * NSLAB * NQ * 4 <= 160;   // registers of a wave's whole filter
};

template <int CIN, int COUT, int KS, int S>
__global__ __launch_bounds__(256) void k_conv_i8(const CI8Args a) {
  using C = CI8Cfg<CIN, COUT, KS, S>;
  __shared__ __attribute__((aligned(16))) char smem[C::LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, p = lane & 31, kh = lane >> 5;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pt = wv % C::PT, cg = wv / C::PT;
  const int slab0 = cg * C::NSLAB;
  const i32x4* wl = a.w + (size_t)slab0 * C::NT * C::NQ * 64 + lane;
  // LDS byte of lane (kh, p)'s fragment of tap (0, 0), k-step 0
  const int lbase = (((2 * pt + (p >> 4)) * C::LS) * C::IW + (p & 15) * C::LS) * C::PITCH + kh * 16;

  // filter fragments stationary in registers where they fit (every 1x1 layer, 64 -> 64 3x3, the 3x3 stride-2 layers from 64
  // channels): read once per workgroup, not once per tile
  i32x4 ws[C::STAT ? C::NT : 1][C::NSLAB][C::NQ];
  if (C::STAT) {
#pragma unroll
    for (int tp = 0; tp < C::NT; ++tp)
#pragma unroll
      for (int s = 0; s < C::NSLAB; ++s)
#pragma unroll
        for (int q = 0; q < C::NQ; ++q) ws[C::STAT ? tp : 0][s][q] = wl[(size_t)((s * C::NT + tp) * C::NQ + q) * 64];
  }

  // halo of tile t: memory -> registers (unconditional load from a clamped address + select)
  auto load_halo = [&](int t, uint4 (&v)[C::NIT]) {
    const int tx = t % a.tiles_x;
    const int tq = t / a.tiles_x;
    const int ty = tq % a.tiles_y, n = tq / a.tiles_y;
    const int8_t* in_img = a.in + (size_t)n * a.H * a.W * CIN;
#pragma unroll
    for (int it = 0; it < C::NIT; ++it) {
      const int i = tid + 256 * it;
      const int pix = i / (CIN / 16), ck = i % (CIN / 16);
      const int iy = pix / C::IW, ix = pix - iy * C::IW;
      const int gy = KS == 1 ? (ty * C::TH + iy) * S : ty * C::TH * S - C::PAD + iy;
      const int gx = KS == 1 ? (tx * C::TW + ix) * S : tx * C::TW * S - C::PAD + ix;
      const bool ok = i < C::PIECES && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
      v[it] = *reinterpret_cast<const uint4*>(in_img + (ok ? (gy * a.W + gx) * CIN + ck * 16 : 0));
      if (!ok) v[it] = make_uint4(0u, 0u, 0u, 0u);
    }
  };

  uint4 v[C::NIT];
  if ((int)blockIdx.x < a.ntiles) load_halo(blockIdx.x, v);
  for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const int tx = t % a.tiles_x;
    const int tq = t / a.tiles_x;
    const int ty = tq % a.tiles_y, n = tq / a.tiles_y;

    __syncthreads();            // every wave is done reading the previous tile
#pragma unroll
    for (int it = 0; it < C::NIT; ++it) {
      const int i = tid + 256 * it;
      if (i < C::PIECES) *reinterpret_cast<uint4*>(smem + (i / (CIN / 16)) * C::PITCH + (i % (CIN / 16)) * 16) = v[it];
    }
    __syncthreads();
    if (t + (int)gridDim.x < a.ntiles) load_halo(t + gridDim.x, v);     // the next tile travels while this one is contracted

    i32x16 acc[C::NSLAB];
#pragma unroll
    for (int s = 0; s < C::NSLAB; ++s)
#pragma unroll
      for (int g = 0; g < 16; ++g) acc[s][g] = 0;

    auto contract = [&](int tp, const i32x4 (&w)[C::NSLAB][C::NQ]) {
      const int dy = tp / KS, dx = tp - dy * KS;
#pragma unroll
      for (int q = 0; q < C::NQ; ++q) {
        const i32x4 b = *reinterpret_cast<const i32x4*>(smem + lbase + (dy * C::IW + dx) * C::PITCH + q * 32);
#pragma unroll
        for (int s = 0; s < C::NSLAB; ++s) acc[s] = __builtin_amdgcn_mfma_i32_32x32x32_i8(w[s][q], b, acc[s], 0, 0, 0);
      }
    };
    if constexpr (C::STAT) {
#pragma unroll
      for (int tp = 0; tp < C::NT; ++tp) contract(tp, ws[tp]);
    } else {
      // the filter of one tap at a time, the next tap's fragments on their way while this one is contracted
      auto load_tap = [&](int tp, i32x4 (&w)[C::NSLAB][C::NQ]) {
#pragma unroll
        for (int s = 0; s < C::NSLAB; ++s)
#pragma unroll
          for (int q = 0; q < C::NQ; ++q) w[s][q] = wl[(size_t)((s * C::NT + tp) * C::NQ + q) * 64];
      };
      static_assert(C::STAT || C::NT % 2 == 1, "the tap loop below runs pairs and one last tap");
      i32x4 w1[C::NSLAB][C::NQ];
      load_tap(0, ws[0]);
#pragma unroll 1
      for (int tp = 0; tp + 1 < C::NT; tp += 2) {
        load_tap(tp + 1, w1);
        contract(tp, ws[0]);
        load_tap(tp + 2, ws[0]);
        contract(tp + 1, w1);
      }
      contract(C::NT - 1, ws[0]);
    }

    // ---- epilogue: register g of lane (kh, p) = channel 32 slab + 16 kh + g of pixel p
    const int oy = ty * C::TH + 2 * pt + (p >> 4), ox = tx * C::TW + (p & 15);
    const bool ook = oy < a.OH && ox < a.OW;
    const size_t opix = ((size_t)n * a.OH * a.OW + (size_t)((ook ? oy : 0) * a.OW + (ook ? ox : 0))) * COUT;
#pragma unroll
    for (int s = 0; s < C::NSLAB; ++s) {
      const int c0 = (slab0 + s) * 32 + 16 * kh;
      float vv[16], mm[16], bb[16];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float4 m4 = *reinterpret_cast<const float4*>(a.mult + c0 + 4 * j);
        const float4 b4 = *reinterpret_cast<const float4*>(a.biasq + c0 + 4 * j);
        mm[4 * j + 0] = m4.x; mm[4 * j + 1] = m4.y; mm[4 * j + 2] = m4.z; mm[4 * j + 3] = m4.w;
        bb[4 * j + 0] = b4.x; bb[4 * j + 1] = b4.y; bb[4 * j + 2] = b4.z; bb[4 * j + 3] = b4.w;
      }
#pragma unroll
      for (int g = 0; g < 16; ++g) vv[g] = __builtin_fmaf((float)acc[s][g], mm[g], bb[g]);
      union { uint4 u; int8_t b[16]; } r;
      r.u = make_uint4(0u, 0u, 0u, 0u);
      if (a.res) {              // (wave-uniform)
        r.u = *reinterpret_cast<const uint4*>(a.res + opix + c0);
#pragma unroll
        for (int g = 0; g < 16; ++g) vv[g] = __builtin_fmaf((float)r.b[g], a.res_mult, vv[g]);
      }
      if (a.relu) {
#pragma unroll
        for (int g = 0; g < 16; ++g) vv[g] = vv[g] > 0.f ? vv[g] : 0.f;
      }
      union { uint4 u; int8_t b[16]; } o;
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        float r = __builtin_rintf(vv[g]);
        r = r > 127.f ? 127.f : r;
        r = r < -127.f ? -127.f : r;
        o.b[g] = (int8_t)(int)r;
      }
      if (ook) *reinterpret_cast<uint4*>(a.out_i8 + opix + c0) = o.u;
      if (a.out_f16) {          // (wave-uniform) a pyramid tap: the un-requantised value for the fp16 head.  Evaluated in
        // float64 and rounded once: the fp32 chain's first rounding (<= 2^-25 |acc mult + biasq|) survives a cancelling
        // residual add and would exceed one fp16 ulp of a small result (measured: 1.25 ulp)
        union { uint4 u[2]; _Float16 h[16]; } f;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          double dv = __builtin_fma((double)acc[s][g], (double)mm[g], (double)bb[g]);
          if (a.res) dv = __builtin_fma((double)r.b[g], (double)a.res_mult, dv);
          if (a.relu) dv = dv > 0.0 ? dv : 0.0;
          f.h[g] = (_Float16)(float)(dv * (double)a.out_scale);
        }
        if (ook) {
          *reinterpret_cast<uint4*>(a.out_f16 + opix + c0) = f.u[0];
          *reinterpret_cast<uint4*>(a.out_f16 + opix + c0 + 8) = f.u[1];
        }
      }
    }
  }
}

template <int CIN, int COUT, int KS, int S>
int launch_i8(CI8Args& a, hipStream_t st) {
  using C = CI8Cfg<CIN, COUT, KS, S>;
  a.tiles_x = (a.OW + C::TW - 1) / C::TW;
  a.tiles_y = (a.OH + C::TH - 1) / C::TH;
  const long tiles = (long)a.tiles_x * a.tiles_y * a.N;
  if (tiles > 0x7fffffffL) return LFD_ERR_UNSUPPORTED;
  a.ntiles = (int)tiles;
  const int blocks = a.ntiles < CI8_MAX_WORKGROUPS ? a.ntiles : CI8_MAX_WORKGROUPS;
  hipLaunchKernelGGL((k_conv_i8<CIN, COUT, KS, S>), dim3((unsigned)blocks), dim3(256), 0, st, a);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

template <int CIN, int COUT>
int launch_i8_ks(CI8Args& a, int ks, int stride, hipStream_t st) {
  if (ks == 3) return stride == 1 ? launch_i8<CIN, COUT, 3, 1>(a, st) : launch_i8<CIN, COUT, 3, 2>(a, st);
  return stride == 1 ? launch_i8<CIN, COUT, 1, 1>(a, st) : launch_i8<CIN, COUT, 1, 2>(a, st);
}

// q = clamp(rint((float)x * inv_scale), -127, 127): 16 values per thread and trip, the last count % 16 one by one
__global__ __launch_bounds__(256) void k_quantize_f16_i8(const _Float16* __restrict__ in, int8_t* __restrict__ out, long count,
                                                         float inv_scale) {
  const long nvec = count >> 4;
  const long step = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += step) {
    const uint4 lo = *reinterpret_cast<const uint4*>(in + i * 16);
    const uint4 hi = *reinterpret_cast<const uint4*>(in + i * 16 + 8);
    *reinterpret_cast<uint4*>(out + i * 16) = lfd_quant16_f16_i8(lo, hi, inv_scale);
  }
  const long tail = (nvec << 4) + (long)blockIdx.x * 256 + threadIdx.x;     // (count & 15 <= 15 elements: block 0 covers them)
  if (tail < count) {
    float r = __builtin_rintf((float)in[tail] * inv_scale);
    r = r > 127.f ? 127.f : r;
    r = r < -127.f ? -127.f : r;
    out[tail] = (int8_t)(int)r;
  }
}

// the same step into a wider pixel: out [pixels][cout] = q(in [pixels][cin]) in channels < cin, 0 above (a 32-channel stem in
// front of stages that run padded to 64); one thread per 16 output channels of a pixel
__global__ __launch_bounds__(256) void k_quantize_pad_f16_i8(const _Float16* __restrict__ in, int8_t* __restrict__ out, long pixels,
                                                             int cin, int cout, float inv_scale) {
  const int per = cout >> 4;
  const long total = pixels * per;
  const long step = (long)gridDim.x * 256;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
    const long pix = i / per;
    const int c0 = (int)(i - pix * per) << 4;
    const bool real = c0 < cin;
    const _Float16* src = in + (real ? pix * cin + c0 : 0);
    uint4 q = lfd_quant16_f16_i8(*reinterpret_cast<const uint4*>(src), *reinterpret_cast<const uint4*>(src + 8), inv_scale);
    if (!real) q = make_uint4(0u, 0u, 0u, 0u);
    *reinterpret_cast<uint4*>(out + pix * cout + c0) = q;
  }
}

}  // namespace

extern "C" int lfd_conv2d_nhwc_i8_supported(int32_t cin, int32_t cout, int32_t ks, int32_t stride) {
  if ((cin != 64 && cin != 128) || (cout != 64 && cout != 128)) return LFD_ERR_UNSUPPORTED;
  if ((ks != 1 && ks != 3) || (stride != 1 && stride != 2)) return LFD_ERR_UNSUPPORTED;
  return LFD_OK;
}

extern "C" int lfd_conv2d_nhwc_i8(const lfd_conv_desc_t* d, const void* in, const void* w_packed, const float* mult,
                                  const float* biasq, const void* res, float res_mult, void* out_i8, void* out_f16,
                                  float out_scale, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!d || !in || !w_packed || !mult || !biasq || !out_i8) return LFD_ERR_INVALID_ARGUMENT;
  if (d->n < 1 || d->h < 1 || d->w < 1 || d->tail_cout != 0) return LFD_ERR_INVALID_ARGUMENT;
  const int rc = lfd_conv2d_nhwc_i8_supported(d->cin, d->cout, d->ks, d->stride);
  if (rc != LFD_OK) return rc;
  if (!lfd_aligned16(in) || !lfd_aligned16(w_packed) || !lfd_aligned16(mult) || !lfd_aligned16(biasq) || !lfd_aligned16(res) ||
      !lfd_aligned16(out_i8) || !lfd_aligned16(out_f16))
    return LFD_ERR_INVALID_ARGUMENT;
  if (in == out_i8 || res == out_i8) return LFD_ERR_INVALID_ARGUMENT;
  if ((long)d->h * d->w * 128 > 0x7fffffffL) return LFD_ERR_UNSUPPORTED;     // 32-bit offsets inside an image
  CI8Args a{};
  a.in = (const int8_t*)in; a.w = (const i32x4*)w_packed; a.mult = mult; a.biasq = biasq; a.res = (const int8_t*)res;
  a.out_i8 = (int8_t*)out_i8; a.out_f16 = (_Float16*)out_f16; a.res_mult = res_mult; a.out_scale = out_scale;
  a.N = d->n; a.H = d->h; a.W = d->w; a.relu = d->relu ? 1 : 0;
  const int pad = d->ks / 2;
  a.OH = (d->h + 2 * pad - d->ks) / d->stride + 1;
  a.OW = (d->w + 2 * pad - d->ks) / d->stride + 1;
  if (d->cin == 64) return d->cout == 64 ? launch_i8_ks<64, 64>(a, d->ks, d->stride, st) : launch_i8_ks<64, 128>(a, d->ks, d->stride, st);
  return d->cout == 64 ? launch_i8_ks<128, 64>(a, d->ks, d->stride, st) : launch_i8_ks<128, 128>(a, d->ks, d->stride, st);
}

extern "C" int lfd_quantize_nhwc_f16_i8(const void* in, void* out, int64_t count, float inv_scale, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!in || !out || count < 1) return LFD_ERR_INVALID_ARGUMENT;
  if (!lfd_aligned16(in) || !lfd_aligned16(out)) return LFD_ERR_INVALID_ARGUMENT;
  long blocks = ((count >> 4) + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > Q8_MAX_WORKGROUPS ? Q8_MAX_WORKGROUPS : blocks);
  hipLaunchKernelGGL(k_quantize_f16_i8, dim3((unsigned)blocks), dim3(256), 0, st, (const _Float16*)in, (int8_t*)out, (long)count,
                     inv_scale);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

extern "C" int lfd_quantize_pad_nhwc_f16_i8(const void* in, void* out, int64_t pixels, int32_t cin, int32_t cout, float inv_scale,
                                            lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!in || !out || pixels < 1) return LFD_ERR_INVALID_ARGUMENT;
  if (!lfd_aligned16(in) || !lfd_aligned16(out)) return LFD_ERR_INVALID_ARGUMENT;
  if (cin < 16 || cin % 16 || cout % 16 || cout < cin || cout > 128) return LFD_ERR_UNSUPPORTED;
  long blocks = (pixels * (cout >> 4) + 255) / 256;
  blocks = blocks > Q8_MAX_WORKGROUPS ? Q8_MAX_WORKGROUPS : blocks;
  hipLaunchKernelGGL(k_quantize_pad_f16_i8, dim3((unsigned)blocks), dim3(256), 0, st, (const _Float16*)in, (int8_t*)out, (long)pixels,
                     cin, cout, inv_scale);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}
