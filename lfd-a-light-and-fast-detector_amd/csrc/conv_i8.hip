// csrc/conv_i8.hip -- the INT8 deployment mode's layer kernels: NHWC int8 conv of the residual stages with the
// requantising epilogue, the stage-entry pair of two such convs from one staged tile, and the fp16 -> int8 quantise step behind
// the stem.  Replaces what the reference gets from TensorRT's INT8 engine (lfd/deployment/tensorrt/build_engine.py:22-126:
// INT8Calibrator + BuilderFlag.INT8).  The lane map, the LDS pixel pitch, the tile walk and the epilogue: csrc/i8_impl.h.
//
// lfd_conv2d_nhwc_i8: ks 1 | 3, stride 1 | 2, pad ks / 2, cin and cout in {64, 128}.
//   * a workgroup (4 waves) owns TH x 16 output pixels -- stride 1: 8 rows = four MFMA tiles of 2 rows, wave w is tile w and
//     every 32-channel slab of cout; stride 2: 4 rows = two tiles, wave w is tile w & 1 and half the slabs -- and stages the
//     input halo once through LDS; a 1x1 stride-2 conv stages only the pixels it reads.  The halo of a workgroup's next tile
//     travels from memory into registers while the current one is contracted.  The filter never enters LDS: where a wave's
//     fragments fit in 160 registers (every 1x1 layer, 64 -> 64 3x3, the 3x3 stride-2 layers from 64 channels) they are read
//     once per workgroup and stay; the other layers read them per tile in k-step order (<= 144 KB per layer, cache resident).
//   * workgroups walk (image, tile) with stride gridDim.x (at most CI8_MAX_WORKGROUPS).
//   * res, relu and out_f16 (a pyramid tap) are wave-uniform runtime flags of the epilogue.
// lfd_conv2d_downsample_nhwc_i8 (the PAIR instances): the 3x3 stride-2 conv (ReLU) and the 1x1 stride-2 identity branch (no ReLU)
// of an entry block from ONE staged input tile: the 1x1 reads the 3x3's centre tap.  The same kernel with the 1x1 filter always
// stationary, a second accumulator set and a second epilogue; no residual, no tap.  One exception: the 64 -> 128 pair is slower
// that way and keeps its own kernel, k_down_i8 (below the quantise kernels, where the reason stands).
#include <type_traits>
#include "i8_impl.h"

namespace {

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
// the stage-entry pair: out_i8 is the 3x3 (ReLU); res, out_f16 and relu are not read
struct CI8PairArgs : CI8Args {
  const i32x4* wd;        // 1x1: packed [cout/32][cin/32][64 lanes]
  const float* multd;
  const float* biasqd;
  int8_t* ds_out_i8;      // [N,OH,OW,cout]: the 1x1, no ReLU
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

template <int CIN, int COUT, int KS, int S, class Args>
__global__ __launch_bounds__(256) void k_conv_i8(const Args a) {
  using C = CI8Cfg<CIN, COUT, KS, S>;
  constexpr bool PAIR = std::is_same<Args, CI8PairArgs>::value;
  static_assert(!PAIR || (KS == 3 && S == 2), "the identity branch reads the centre tap of a 3x3 stride-2 tile");
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
  i32x4 wd[C::NSLAB][C::NQ];          // the pair's 1x1 filter: always stationary
  if constexpr (PAIR) {
#pragma unroll
    for (int s = 0; s < C::NSLAB; ++s)
#pragma unroll
      for (int q = 0; q < C::NQ; ++q) wd[s][q] = a.wd[(size_t)((slab0 + s) * C::NQ + q) * 64 + lane];
  }

  // halo of tile t: memory -> registers
  auto load_halo = [&](int t, I8Piece<> (&v)[C::NIT]) {
    const I8Tile tl = i8_tile_of(t, a.tiles_x, a.tiles_y);
    if constexpr (KS == 1 && S == 2) {
      // the four 1x1 stride-2 instances stage only the pixels they read, every second one, and keep this written-out copy of
      // i8_halo_load (keep it in step): through the shared loader with a stride, in either arithmetic form, the 64 -> 64
      // instance measured 1.0 .. 2.1 % slower at 270 x 480, batch 8, and three of the four take 2 more registers
      const int8_t* in_img = a.in + (size_t)tl.n * a.H * a.W * CIN;
#pragma unroll
      for (int it = 0; it < C::NIT; ++it) {
        const int i = tid + 256 * it;
        const int pix = i >> I8_LG<CIN>, ck = i & (CIN / 16 - 1);
        const int iy = pix / C::IW, ix = pix - iy * C::IW;
        const int gy = (tl.ty * C::TH + iy) * S, gx = (tl.tx * C::TW + ix) * S;
        const bool ok = i < C::PIECES && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
        v[it].u[0] = *reinterpret_cast<const uint4*>(in_img + (ok ? (gy * a.W + gx) * CIN + ck * 16 : 0));
        if (!ok) v[it].u[0] = make_uint4(0u, 0u, 0u, 0u);
      }
    } else {
      i8_halo_load<CIN, C::IW, C::PIECES, C::PAD, 256, C::NIT>(v, a.in + (size_t)tl.n * a.H * a.W * CIN, tid, 0,
                                                               tl.ty * C::TH * C::LS, tl.tx * C::TW * C::LS, a.H, a.W);
    }
  };

  I8Piece<> v[C::NIT];
  if ((int)blockIdx.x < a.ntiles) load_halo(blockIdx.x, v);
  for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const I8Tile tl = i8_tile_of(t, a.tiles_x, a.tiles_y);

    __syncthreads();            // every wave is done reading the previous tile
    i8_halo_store<CIN, C::PIECES, 256, C::NIT>(smem, v, tid, 0);
    __syncthreads();
    if (t + (int)gridDim.x < a.ntiles) load_halo(t + gridDim.x, v);     // the next tile travels while this one is contracted

    i32x16 acc[C::NSLAB], accd[PAIR ? C::NSLAB : 1];
#pragma unroll
    for (int s = 0; s < C::NSLAB; ++s)
#pragma unroll
      for (int g = 0; g < 16; ++g) {
        acc[s][g] = 0;
        if constexpr (PAIR) accd[s][g] = 0;
      }

    if constexpr (PAIR) {       // the identity branch: the centre tap's pixels against the 1x1 filter
#pragma unroll
      for (int q = 0; q < C::NQ; ++q) {
        const i32x4 b = *reinterpret_cast<const i32x4*>(smem + lbase + (C::IW + 1) * C::PITCH + q * 32);
#pragma unroll
        for (int s = 0; s < C::NSLAB; ++s) accd[s] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wd[s][q], b, accd[s], 0, 0, 0);
      }
    }

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
    const bool has_res = PAIR ? false : a.res != nullptr, relu = PAIR ? true : a.relu != 0;      // (wave-uniform)
    bool ook;
    const size_t opix = i8_out_pixel<COUT>(tl.n, tl.ty * C::TH + 2 * pt + (p >> 4), tl.tx * C::TW + (p & 15), a.OH, a.OW, ook);
#pragma unroll
    for (int s = 0; s < C::NSLAB; ++s) {
      const int c0 = (slab0 + s) * 32 + 16 * kh;
      float vv[16], mm[16], bb[16];
      load16f(a.mult + c0, mm);
      load16f(a.biasq + c0, bb);
#pragma unroll
      for (int g = 0; g < 16; ++g) vv[g] = i8_affine(acc[s][g], mm[g], bb[g]);
      I8x16 r;
      r.u = make_uint4(0u, 0u, 0u, 0u);
      if (has_res) {
        r.u = *reinterpret_cast<const uint4*>(a.res + opix + c0);
#pragma unroll
        for (int g = 0; g < 16; ++g) vv[g] = i8_residual(vv[g], r.b[g], a.res_mult);
      }
      if (relu) {
#pragma unroll
        for (int g = 0; g < 16; ++g) vv[g] = i8_relu(vv[g]);
      }
      const uint4 o = i8_requant16(vv);
      if (ook) *reinterpret_cast<uint4*>(a.out_i8 + opix + c0) = o;
      if (!PAIR && a.out_f16) {          // (wave-uniform) a pyramid tap
        F16x16 f;
#pragma unroll
        for (int g = 0; g < 16; ++g) f.h[g] = i8_tap(acc[s][g], mm[g], bb[g], has_res, r.b[g], a.res_mult, relu, a.out_scale);
        if (ook) {
          *reinterpret_cast<uint4*>(a.out_f16 + opix + c0) = f.u[0];
          *reinterpret_cast<uint4*>(a.out_f16 + opix + c0 + 8) = f.u[1];
        }
      }
      if constexpr (PAIR) {       // the identity branch: no residual, no ReLU
        load16f(a.multd + c0, mm);
        load16f(a.biasqd + c0, bb);
#pragma unroll
        for (int g = 0; g < 16; ++g) vv[g] = i8_affine(accd[s][g], mm[g], bb[g]);
        const uint4 od = i8_requant16(vv);
        if (ook) *reinterpret_cast<uint4*>(a.ds_out_i8 + opix + c0) = od;
      }
    }
  }
}

template <int CIN, int COUT, int KS, int S, class Args>
int launch_i8(Args& a, hipStream_t st) {
  using C = CI8Cfg<CIN, COUT, KS, S>;
  const int blocks = i8_tile_grid(a, a.N, a.OH, a.OW, C::TH, C::TW, CI8_MAX_WORKGROUPS);
  if (!blocks) return LFD_ERR_UNSUPPORTED;
  hipLaunchKernelGGL((k_conv_i8<CIN, COUT, KS, S, Args>), dim3((unsigned)blocks), dim3(256), 0, st, a);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

template <int CIN, int COUT>
int launch_i8_ks(CI8Args& a, int ks, int stride, hipStream_t st) {
  if (ks == 3) return stride == 1 ? launch_i8<CIN, COUT, 3, 1>(a, st) : launch_i8<CIN, COUT, 3, 2>(a, st);
  return stride == 1 ? launch_i8<CIN, COUT, 1, 1>(a, st) : launch_i8<CIN, COUT, 1, 2>(a, st);
}

// q = lfd_requant_i8((float)x * inv_scale): 16 values per thread and trip, the last count % 16 one by one
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
    out[tail] = lfd_requant_i8((float)in[tail] * inv_scale);
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

// ------------------------------------------------------------------------------------- the 64 -> 128 pair: its own kernel
// k_conv_i8<64, 128, 3, 2, CI8PairArgs> compiles to 256 VGPRs + 85 AGPRs where this kernel has 256 + 83 and measured 2.2 .. 3.6 %
// slower at batch 8, whatever the halo loader and the order of its epilogue, so this one instance keeps the
// separate kernel and its own argument layout: the text k_conv_i8 was merged from, on CI8Cfg<64, 128, 3, 2> and the shared tile
// walk, epilogue steps and requantisation, and compiled to the same instructions as before the merge.  Its halo load and LDS slot
// are copies of i8_impl.h's i8_halo_load / i8_halo_slot (with the shared slot its code already changes): keep them in step.
struct DI8Args {
  const int8_t* in;        // [N,H,W,cin]
  const i32x4* w;          // 3x3: packed [cout/32][9*cin/32][64 lanes]
  const float* mult;
  const float* biasq;
  const i32x4* wd;         // 1x1: packed [cout/32][cin/32][64 lanes]
  const float* multd;
  const float* biasqd;
  int8_t* out_i8;          // [N,OH,OW,cout]: the 3x3, ReLU
  int8_t* ds_out_i8;       // [N,OH,OW,cout]: the 1x1, no ReLU
  int N, H, W, OH, OW;
  int tiles_x, tiles_y, ntiles;
};

template <int CIN, int COUT>
__global__ __launch_bounds__(256) void k_down_i8(const DI8Args a) {
  using C = CI8Cfg<CIN, COUT, 3, 2>;
  __shared__ __attribute__((aligned(16))) char smem[C::LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, p = lane & 31, kh = lane >> 5;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int pt = wv & 1, cg = wv >> 1;
  const int slab0 = cg * C::NSLAB;
  const i32x4* wl = a.w + (size_t)slab0 * 9 * C::NQ * 64 + lane;
  const int lbase = (((2 * pt + (p >> 4)) * 2) * C::IW + (p & 15) * 2) * C::PITCH + kh * 16;

  i32x4 ws[C::STAT ? 9 : 1][C::NSLAB][C::NQ];
  if (C::STAT) {
#pragma unroll
    for (int tp = 0; tp < 9; ++tp)
#pragma unroll
      for (int s = 0; s < C::NSLAB; ++s)
#pragma unroll
        for (int q = 0; q < C::NQ; ++q) ws[C::STAT ? tp : 0][s][q] = wl[(size_t)((s * 9 + tp) * C::NQ + q) * 64];
  }
  i32x4 wd[C::NSLAB][C::NQ];          // the 1x1 filter: always stationary
#pragma unroll
  for (int s = 0; s < C::NSLAB; ++s)
#pragma unroll
    for (int q = 0; q < C::NQ; ++q) wd[s][q] = a.wd[(size_t)((slab0 + s) * C::NQ + q) * 64 + lane];

  auto load_halo = [&](int t, uint4 (&v)[C::NIT]) {
    const I8Tile tl = i8_tile_of(t, a.tiles_x, a.tiles_y);
    const int tx = tl.tx, ty = tl.ty, n = tl.n;
    const int8_t* in_img = a.in + (size_t)n * a.H * a.W * CIN;
#pragma unroll
    for (int it = 0; it < C::NIT; ++it) {
      const int i = tid + 256 * it;
      const int pix = i / (CIN / 16), ck = i % (CIN / 16);
      const int iy = pix / C::IW, ix = pix - iy * C::IW;
      const int gy = ty * C::TH * 2 - 1 + iy;
      const int gx = tx * C::TW * 2 - 1 + ix;
      const bool ok = i < C::PIECES && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
      v[it] = *reinterpret_cast<const uint4*>(in_img + (ok ? (gy * a.W + gx) * CIN + ck * 16 : 0));
      if (!ok) v[it] = make_uint4(0u, 0u, 0u, 0u);
    }
  };

  uint4 v[C::NIT];
  if ((int)blockIdx.x < a.ntiles) load_halo(blockIdx.x, v);
  for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const I8Tile tl = i8_tile_of(t, a.tiles_x, a.tiles_y);
    const int tx = tl.tx, ty = tl.ty, n = tl.n;

    __syncthreads();            // every wave is done reading the previous tile
#pragma unroll
    for (int it = 0; it < C::NIT; ++it) {
      const int i = tid + 256 * it;
      if (i < C::PIECES) *reinterpret_cast<uint4*>(smem + (i / (CIN / 16)) * C::PITCH + (i % (CIN / 16)) * 16) = v[it];
    }
    __syncthreads();
    if (t + (int)gridDim.x < a.ntiles) load_halo(t + gridDim.x, v);     // the next tile travels while this one is contracted

    i32x16 acc[C::NSLAB], accd[C::NSLAB];
#pragma unroll
    for (int s = 0; s < C::NSLAB; ++s)
#pragma unroll
      for (int g = 0; g < 16; ++g) { acc[s][g] = 0; accd[s][g] = 0; }

    // the identity branch: the centre tap's pixels against the 1x1 filter
#pragma unroll
    for (int q = 0; q < C::NQ; ++q) {
      const i32x4 b = *reinterpret_cast<const i32x4*>(smem + lbase + (C::IW + 1) * C::PITCH + q * 32);
#pragma unroll
      for (int s = 0; s < C::NSLAB; ++s) accd[s] = __builtin_amdgcn_mfma_i32_32x32x32_i8(wd[s][q], b, accd[s], 0, 0, 0);
    }

    auto contract = [&](int tp, const i32x4 (&w)[C::NSLAB][C::NQ]) {
      const int dy = tp / 3, dx = tp - dy * 3;
#pragma unroll
      for (int q = 0; q < C::NQ; ++q) {
        const i32x4 b = *reinterpret_cast<const i32x4*>(smem + lbase + (dy * C::IW + dx) * C::PITCH + q * 32);
#pragma unroll
        for (int s = 0; s < C::NSLAB; ++s) acc[s] = __builtin_amdgcn_mfma_i32_32x32x32_i8(w[s][q], b, acc[s], 0, 0, 0);
      }
    };
    if constexpr (C::STAT) {
#pragma unroll
      for (int tp = 0; tp < 9; ++tp) contract(tp, ws[tp]);
    } else {
      // the filter of one tap at a time, the next tap's fragments on their way while this one is contracted
      auto load_tap = [&](int tp, i32x4 (&w)[C::NSLAB][C::NQ]) {
#pragma unroll
        for (int s = 0; s < C::NSLAB; ++s)
#pragma unroll
          for (int q = 0; q < C::NQ; ++q) w[s][q] = wl[(size_t)((s * 9 + tp) * C::NQ + q) * 64];
      };
      i32x4 w1[C::NSLAB][C::NQ];
      load_tap(0, ws[0]);
#pragma unroll 1
      for (int tp = 0; tp + 1 < 9; tp += 2) {
        load_tap(tp + 1, w1);
        contract(tp, ws[0]);
        load_tap(tp + 2, ws[0]);
        contract(tp + 1, w1);
      }
      contract(8, ws[0]);
    }

    // ---- epilogues (lfd_conv2d_nhwc_i8's without residual): register g of lane (kh, p) = channel 32 slab + 16 kh + g
    const int oy = ty * C::TH + 2 * pt + (p >> 4), ox = tx * C::TW + (p & 15);
    const bool ook = oy < a.OH && ox < a.OW;
    const size_t opix = ((size_t)n * a.OH * a.OW + (size_t)((ook ? oy : 0) * a.OW + (ook ? ox : 0))) * COUT;
#pragma unroll
    for (int s = 0; s < C::NSLAB; ++s) {
      const int c0 = (slab0 + s) * 32 + 16 * kh;
      float vv[16], mm[16], bb[16];
      load16f(a.mult + c0, mm);
      load16f(a.biasq + c0, bb);
#pragma unroll
      for (int g = 0; g < 16; ++g) vv[g] = i8_relu(i8_affine(acc[s][g], mm[g], bb[g]));
      const uint4 o = i8_requant16(vv);
      if (ook) *reinterpret_cast<uint4*>(a.out_i8 + opix + c0) = o;
      load16f(a.multd + c0, mm);
      load16f(a.biasqd + c0, bb);
#pragma unroll
      for (int g = 0; g < 16; ++g) vv[g] = i8_affine(accd[s][g], mm[g], bb[g]);
      const uint4 od = i8_requant16(vv);
      if (ook) *reinterpret_cast<uint4*>(a.ds_out_i8 + opix + c0) = od;
    }
  }
}

int launch_down_64_128(const CI8PairArgs& p, hipStream_t st) {
  DI8Args a{p.in, p.w, p.mult, p.biasq, p.wd, p.multd, p.biasqd, p.out_i8, p.ds_out_i8, p.N, p.H, p.W, p.OH, p.OW, 0, 0, 0};
  using C = CI8Cfg<64, 128, 3, 2>;
  const int blocks = i8_tile_grid(a, a.N, a.OH, a.OW, C::TH, C::TW, CI8_MAX_WORKGROUPS);
  if (!blocks) return LFD_ERR_UNSUPPORTED;
  hipLaunchKernelGGL((k_down_i8<64, 128>), dim3((unsigned)blocks), dim3(256), 0, st, a);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
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

extern "C" int lfd_conv2d_downsample_nhwc_i8_supported(int32_t cin, int32_t cout) {
  if ((cin == 64 && (cout == 64 || cout == 128)) || (cin == 128 && cout == 128)) return LFD_OK;
  return LFD_ERR_UNSUPPORTED;
}

extern "C" int lfd_conv2d_downsample_nhwc_i8(int32_t n, int32_t h, int32_t w, int32_t cin, int32_t cout, const void* in,
                                             const void* w_packed, const float* mult, const float* biasq,
                                             const void* ds_w_packed, const float* ds_mult, const float* ds_biasq, void* out_i8,
                                             void* ds_out_i8, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!in || !w_packed || !mult || !biasq || !ds_w_packed || !ds_mult || !ds_biasq || !out_i8 || !ds_out_i8)
    return LFD_ERR_INVALID_ARGUMENT;
  if (n < 1 || h < 1 || w < 1) return LFD_ERR_INVALID_ARGUMENT;
  const int rc = lfd_conv2d_downsample_nhwc_i8_supported(cin, cout);
  if (rc != LFD_OK) return rc;
  if (!lfd_aligned16(in) || !lfd_aligned16(w_packed) || !lfd_aligned16(mult) || !lfd_aligned16(biasq) ||
      !lfd_aligned16(ds_w_packed) || !lfd_aligned16(ds_mult) || !lfd_aligned16(ds_biasq) || !lfd_aligned16(out_i8) ||
      !lfd_aligned16(ds_out_i8))
    return LFD_ERR_INVALID_ARGUMENT;
  if (in == out_i8 || in == ds_out_i8 || out_i8 == ds_out_i8) return LFD_ERR_INVALID_ARGUMENT;
  if ((long)h * w * 128 > 0x7fffffffL) return LFD_ERR_UNSUPPORTED;           // 32-bit offsets inside an image
  CI8PairArgs a{};
  a.in = (const int8_t*)in; a.w = (const i32x4*)w_packed; a.mult = mult; a.biasq = biasq;
  a.wd = (const i32x4*)ds_w_packed; a.multd = ds_mult; a.biasqd = ds_biasq;
  a.out_i8 = (int8_t*)out_i8; a.ds_out_i8 = (int8_t*)ds_out_i8;
  a.N = n; a.H = h; a.W = w; a.relu = 1;
  a.OH = (h - 1) / 2 + 1;
  a.OW = (w - 1) / 2 + 1;
  if (cin == 64) return cout == 64 ? launch_i8<64, 64, 3, 2>(a, st) : launch_down_64_128(a, st);
  return launch_i8<128, 128, 3, 2>(a, st);
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
