// csrc/block_i8.hip -- the INT8 deployment mode's fused launches: a whole 64-channel residual block, and the two
// stride-2 convs that open a stage-entry block.  Both compute exactly what the layer-by-layer launches of csrc/conv_i8.hip
// compute -- the i32 sums are exact in any order and the epilogues below are conv_i8.hip's expressions -- so the results are
// required to agree in every bit (tests/test_gpu_block_i8_exact.py).
//
// lfd_block_i8_fused: y = ReLU(conv2(ReLU(conv1(x))) + x), both convs 3x3 stride 1 pad 1, 64 -> 64, the int8 tensors and
// constants of two lfd_conv2d_nhwc_i8 calls.  The cut is csrc/block.hip's (PRODUCER / CONSUMER wave specialisation):
//   * one 512-thread workgroup per CU, persistent, walking (image, tile) with stride gridDim.x (<= BI8_MAX_WORKGROUPS).  Waves
//     0-3 are conv1 producers, waves 4-7 conv2 consumers; wave w and wave w + 4 share a SIMD, so each matrix pipe serves one
//     producer and one consumer and the one's loads, epilogue and stores run under the other's MFMAs.
//   * both filters are stationary: a wave owns one 32-channel slab of ONE conv, 18 k-steps of 16 bytes per lane = 72 VGPRs,
//     read once per workgroup in the ops.pack_conv_weight_i8 order (nothing is repacked).  The lane's 16 mult / biasq values
//     are re-read per tile (cache-hot): the registers go to the filter.
//   * per 8 x 16 output tile the producers contract the 12 x 20 input halo (LDS, 80-byte pixels as in conv_i8.hip) into the
//     10 x 18 mid tile: 180 pixels numbered linearly over six 32-pixel MFMA tiles, three per producer pixel group (93.75 % of
//     the slots useful, recompute factor (192 + 128) / 256 = 1.25).  The mid tile is int8 in LDS only, 80-byte pixels, one
//     16-byte write per lane; mid pixels outside the image are conv2's zero padding and are written as 0, not as conv1
//     evaluated there.  Input halo pixels outside the image are 0 (load from a clamped address + select).
//   * software pipeline, ONE barrier per step: in step s the producers contract tile s from in[s & 1] into mid[s & 1] while
//     the halo of tile s + 1 travels through their registers into in[(s + 1) & 1], and the consumers contract tile s - 1 from
//     mid[(s - 1) & 1], add the identity (a 16-byte load of x per lane, cache-hot: the producers just pulled those lines),
//     requantise and store.  Ragged tiles are guarded on the store.
//   * v_mfma_i32_32x32x32_i8 with A = filter, B = pixels and the lane map of conv_i8.hip: a lane ends with 16 consecutive
//     channels of its pixel.
//   * LDS: 2 x 19200 (input) + 2 x 14400 (mid) = 67200 bytes, dynamic.  hipcc reports 232 VGPRs, no AGPRs, no scratch.
//
// lfd_conv2d_downsample_nhwc_i8: the 3x3 stride-2 conv (ReLU) and the 1x1 stride-2 identity branch (no ReLU) of an entry block
// from ONE staged input tile: the 1x1 reads the 3x3's centre tap.  conv_i8.hip's stride-2 cut (4 x 16 output tile, 4 waves =
// 2 pixel tiles x 2 channel groups), the 1x1 filter always stationary, a second accumulator set and a second epilogue.
#include "common.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

constexpr int BI8_MAX_WORKGROUPS = 256;     // one 512-thread workgroup per CU
constexpr int DI8_MAX_WORKGROUPS = 1024;

// clamp(rint(v), -127, 127) of 16 values -> 16 bytes (conv_i8.hip's expression)
__device__ __forceinline__ uint4 requant16(const float (&vv)[16]) {
  union { uint4 u; int8_t b[16]; } o;
#pragma unroll
  for (int g = 0; g < 16; ++g) {
    float r = __builtin_rintf(vv[g]);
    r = r > 127.f ? 127.f : r;
    r = r < -127.f ? -127.f : r;
    o.b[g] = (int8_t)(int)r;
  }
  return o.u;
}

__device__ __forceinline__ void load16f(const float* src, float (&dst)[16]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float4 f = *reinterpret_cast<const float4*>(src + 4 * j);
    dst[4 * j + 0] = f.x; dst[4 * j + 1] = f.y; dst[4 * j + 2] = f.z; dst[4 * j + 3] = f.w;
  }
}

// ------------------------------------------------------------------------------------------------ fused residual block
struct BI8Args {
  const int8_t* in;        // [N,H,W,64]
  const i32x4* w1;         // packed [2][18][64 lanes]
  const float* mult1;      // [64]
  const float* biasq1;
  const i32x4* w2;
  const float* mult2;
  const float* biasq2;
  int8_t* out_i8;          // [N,H,W,64]
  _Float16* out_f16;       // [N,H,W,64] or NULL
  float res_mult, out_scale;
  int N, H, W;
  int tiles_x, tiles_y, ntiles;
};

struct BI8 {
  static constexpr int TH = 8, TW = 16;                 // output tile
  static constexpr int MH = TH + 2, MW = TW + 2;        // mid tile (conv1's output with conv2's halo)
  static constexpr int MPIX = MH * MW;                  // 180
  static constexpr int IH = TH + 4, IW = TW + 4;        // input halo tile
  static constexpr int IPIX = IH * IW;                  // 240
  static constexpr int PITCH = 64 + 16;                 // bytes per LDS pixel (16 of bank spread), input and mid
  static constexpr int IN_BYTES = IPIX * PITCH;         // 19200
  static constexpr int MID_BYTES = MPIX * PITCH;        // 14400
  static constexpr int PIECES = IPIX * 4;               // 16-byte pieces of the input halo
  static constexpr int NIT = (PIECES + 255) / 256;      // per producer thread
  static constexpr int NK = 18;                         // k-steps of a 3x3x64 contraction
  static constexpr int OFF_IN = 0;
  static constexpr int OFF_MID = 2 * IN_BYTES;
  static constexpr int LDS_BYTES = OFF_MID + 2 * MID_BYTES;      // 67200
};
static_assert(BI8::LDS_BYTES <= 160 * 1024, "LDS capacity");

__global__ __launch_bounds__(512) void k_block_i8(const BI8Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool prod = wv < 4;
  const int ct = wv & 1, pg = (wv >> 1) & 1;            // channel slab, pixel group of this wave within its role
  const int grid = gridDim.x;
  const int my = (a.ntiles - (int)blockIdx.x + grid - 1) / grid;       // tiles of this workgroup (>= 1: grid <= ntiles)

  // stationary: the wave's filter slab and the lane's epilogue constants, of conv1 (producers) or conv2 (consumers)
  i32x4 ws[BI8::NK];
  {
    const i32x4* wl = (prod ? a.w1 : a.w2) + (size_t)ct * BI8::NK * 64 + lane;
#pragma unroll
    for (int k = 0; k < BI8::NK; ++k) ws[k] = wl[(size_t)k * 64];
  }
  const float* mult = prod ? a.mult1 : a.mult2;         // re-read per tile (cache-hot): 32 registers the filter needs
  const float* biasq = prod ? a.biasq1 : a.biasq2;

  // input halo of tile t: memory -> registers (producer threads, tid < 256) -> LDS
  auto load_halo = [&](int tid, int t, uint4 (&v)[BI8::NIT]) {
    const int tx = t % a.tiles_x;
    const int tq = t / a.tiles_x;
    const int ty = tq % a.tiles_y, n = tq / a.tiles_y;
    const int8_t* in_img = a.in + (size_t)n * a.H * a.W * 64;
#pragma unroll
    for (int it = 0; it < BI8::NIT; ++it) {
      const int i = tid + 256 * it;
      const int pix = i >> 2, ck = i & 3;
      const int iy = pix / BI8::IW, ix = pix - iy * BI8::IW;
      const int gy = ty * BI8::TH - 2 + iy, gx = tx * BI8::TW - 2 + ix;
      const bool ok = i < BI8::PIECES && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
      v[it] = *reinterpret_cast<const uint4*>(in_img + (ok ? (gy * a.W + gx) * 64 + ck * 16 : 0));
      if (!ok) v[it] = make_uint4(0u, 0u, 0u, 0u);
    }
  };
  auto store_halo = [&](int tid, int buf, const uint4 (&v)[BI8::NIT]) {
    char* dst = smem + BI8::OFF_IN + buf * BI8::IN_BYTES;
#pragma unroll
    for (int it = 0; it < BI8::NIT; ++it) {
      const int i = tid + 256 * it;
      if (i < BI8::PIECES) *reinterpret_cast<uint4*>(dst + (i >> 2) * BI8::PITCH + (i & 3) * 16) = v[it];
    }
  };

  uint4 hv[BI8::NIT];
  if (prod) {
    load_halo(tid, blockIdx.x, hv);
    store_halo(tid, 0, hv);
  }

  for (int s = 0; s <= my; ++s) {
    __syncthreads();      // in[s & 1] and mid[(s - 1) & 1] are complete; mid[s & 1] and in[(s + 1) & 1] are free
    // the per-lane geometry below is recomputed per tile (a few VALU instructions) instead of being hoisted out of the loop
    // into registers the stationary filter needs
    int tl = threadIdx.x;
    asm volatile("" : "+v"(tl));
    const int p = tl & 31, kh = (tl >> 5) & 1;
    const int c0 = 32 * ct + 16 * kh;                   // the lane's 16 output channels
    if (prod) {
      if (s < my) {
        // -------------------------------------------------------------------------------------- producer: conv1 of tile s
        const int t = (int)blockIdx.x + s * grid;
        const int tx = t % a.tiles_x;
        const int ty = (t / a.tiles_x) % a.tiles_y;
        const bool more = s + 1 < my;
        if (more) load_halo(tl, t + grid, hv);              // travels while this tile is contracted
        const char* in_t = smem + BI8::OFF_IN + (s & 1) * BI8::IN_BYTES;
        char* mid_t = smem + BI8::OFF_MID + (s & 1) * BI8::MID_BYTES;

        // mid pixel m = (3 pg + pt) * 32 + p, linear over 10 x 18; mid (row, col) = input tile (row + dy, col + dx)
        int pbase[3], mrow[3], mcol[3];
        bool mval[3];
#pragma unroll
        for (int pt = 0; pt < 3; ++pt) {
          const int m = (pg * 3 + pt) * 32 + p;
          mval[pt] = m < BI8::MPIX;
          const int mc = mval[pt] ? m : BI8::MPIX - 1;
          mrow[pt] = mc / BI8::MW;
          mcol[pt] = mc - mrow[pt] * BI8::MW;
          pbase[pt] = (mrow[pt] * BI8::IW + mcol[pt]) * BI8::PITCH + kh * 16;
        }
        // one MFMA tile at a time (16 accumulator registers live): the epilogue of one runs under the MFMAs of the next
        // epilogue: mid = clamp(rint(max(fmaf(acc, mult1, biasq1), 0))); 0 outside the image (conv2's padding)
        float mm[16], bb[16];
        load16f(mult + c0, mm);
        load16f(biasq + c0, bb);
#pragma unroll
        for (int pt = 0; pt < 3; ++pt) {
          i32x16 acc;
#pragma unroll
          for (int g = 0; g < 16; ++g) acc[g] = 0;
#pragma unroll
          for (int k = 0; k < BI8::NK; ++k) {
            const int tp = k >> 1, q = k & 1, dy = tp / 3, dx = tp - dy * 3;
            const i32x4 b = *reinterpret_cast<const i32x4*>(in_t + pbase[pt] + (dy * BI8::IW + dx) * BI8::PITCH + q * 32);
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(ws[k], b, acc, 0, 0, 0);
          }
          float vv[16];
#pragma unroll
          for (int g = 0; g < 16; ++g) {
            vv[g] = __builtin_fmaf((float)acc[g], mm[g], bb[g]);
            vv[g] = vv[g] > 0.f ? vv[g] : 0.f;
          }
          uint4 o = requant16(vv);
          const int gy = ty * BI8::TH - 1 + mrow[pt], gx = tx * BI8::TW - 1 + mcol[pt];
          if (gy < 0 || gy >= a.H || gx < 0 || gx >= a.W) o = make_uint4(0u, 0u, 0u, 0u);
          if (mval[pt]) *reinterpret_cast<uint4*>(mid_t + ((pg * 3 + pt) * 32 + p) * BI8::PITCH + c0) = o;
        }
        if (more) store_halo(tl, (s + 1) & 1, hv);
      }
    } else if (s >= 1) {
      // ---------------------------------------------------------------------------------------- consumer: conv2 of tile s - 1
      const int t = (int)blockIdx.x + (s - 1) * grid;
      const int tx = t % a.tiles_x;
      const int tq = t / a.tiles_x;
      const int ty = tq % a.tiles_y, n = tq / a.tiles_y;
      const char* mid_t = smem + BI8::OFF_MID + ((s - 1) & 1) * BI8::MID_BYTES;

      // MFMA pixel tile 2 pg + j = output rows 2 (2 pg + j), + 1 of the tile; out (y, x) reads mid (y + dy, x + dx)
      int cbase[2];
      size_t opix[2];
      bool ook[2];
      union { uint4 u; int8_t b[16]; } r[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int ly = 2 * (2 * pg + j) + (p >> 4), lx = p & 15;
        cbase[j] = (ly * BI8::MW + lx) * BI8::PITCH + kh * 16;
        const int oy = ty * BI8::TH + ly, ox = tx * BI8::TW + lx;
        ook[j] = oy < a.H && ox < a.W;
        opix[j] = ((size_t)n * a.H * a.W + (size_t)((ook[j] ? oy : 0) * a.W + (ook[j] ? ox : 0))) * 64 + c0;
        r[j].u = *reinterpret_cast<const uint4*>(a.in + opix[j]);        // the identity, on its way under the MFMAs
      }
      i32x16 acc[2];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[j][g] = 0;
#pragma unroll
      for (int tp = 0; tp < 9; ++tp) {
        const int dy = tp / 3, dx = tp - dy * 3;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            const i32x4 b = *reinterpret_cast<const i32x4*>(mid_t + cbase[j] + (dy * BI8::MW + dx) * BI8::PITCH + q * 32);
            acc[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(ws[tp * 2 + q], b, acc[j], 0, 0, 0);
          }
        }
      }
      // epilogue: lfd_conv2d_nhwc_i8's with a residual and ReLU
      float mm[16], bb[16];
      load16f(mult + c0, mm);
      load16f(biasq + c0, bb);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float vv[16];
#pragma unroll
        for (int g = 0; g < 16; ++g) {
          vv[g] = __builtin_fmaf((float)acc[j][g], mm[g], bb[g]);
          vv[g] = __builtin_fmaf((float)r[j].b[g], a.res_mult, vv[g]);
          vv[g] = vv[g] > 0.f ? vv[g] : 0.f;
        }
        const uint4 o = requant16(vv);
        if (ook[j]) *reinterpret_cast<uint4*>(a.out_i8 + opix[j]) = o;
        if (a.out_f16) {        // (wave-uniform) a pyramid tap: evaluated in float64 and rounded once, as conv_i8.hip does
          union { uint4 u[2]; _Float16 h[16]; } f;
#pragma unroll
          for (int g = 0; g < 16; ++g) {
            double dv = __builtin_fma((double)acc[j][g], (double)mm[g], (double)bb[g]);
            dv = __builtin_fma((double)r[j].b[g], (double)a.res_mult, dv);
            dv = dv > 0.0 ? dv : 0.0;
            f.h[g] = (_Float16)(float)(dv * (double)a.out_scale);
          }
          if (ook[j]) {
            *reinterpret_cast<uint4*>(a.out_f16 + opix[j]) = f.u[0];
            *reinterpret_cast<uint4*>(a.out_f16 + opix[j] + 8) = f.u[1];
          }
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ stage-entry pair
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
struct DI8Cfg {
  static constexpr int TH = 4, TW = 16;                 // output tile; MFMA tile pt = rows 2 pt, 2 pt + 1
  static constexpr int NSLAB = COUT / 32 / 2;           // 32-channel slabs per wave (two channel groups)
  static constexpr int IH = (TH - 1) * 2 + 3, IW = (TW - 1) * 2 + 3;
  static constexpr int NPIX = IH * IW;
  static constexpr int PITCH = CIN + 16;
  static constexpr int PIECES = NPIX * (CIN / 16);
  static constexpr int NIT = (PIECES + 255) / 256;
  static constexpr int NQ = CIN / 32;
  static constexpr int LDS_BYTES = NPIX * PITCH;
  static_assert(LDS_BYTES <= 64 * 1024, "static LDS");
  static constexpr bool STAT = 9 * NSLAB * NQ * 4 <= 160;    // registers of a wave's whole 3x3 filter
};

template <int CIN, int COUT>
__global__ __launch_bounds__(256) void k_down_i8(const DI8Args a) {
  using C = DI8Cfg<CIN, COUT>;
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
    const int tx = t % a.tiles_x;
    const int tq = t / a.tiles_x;
    const int ty = tq % a.tiles_y, n = tq / a.tiles_y;
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
      for (int g = 0; g < 16; ++g) {
        vv[g] = __builtin_fmaf((float)acc[s][g], mm[g], bb[g]);
        vv[g] = vv[g] > 0.f ? vv[g] : 0.f;
      }
      const uint4 o = requant16(vv);
      if (ook) *reinterpret_cast<uint4*>(a.out_i8 + opix + c0) = o;
      load16f(a.multd + c0, mm);
      load16f(a.biasqd + c0, bb);
#pragma unroll
      for (int g = 0; g < 16; ++g) vv[g] = __builtin_fmaf((float)accd[s][g], mm[g], bb[g]);
      const uint4 od = requant16(vv);
      if (ook) *reinterpret_cast<uint4*>(a.ds_out_i8 + opix + c0) = od;
    }
  }
}

template <int CIN, int COUT>
int launch_down_i8(DI8Args& a, hipStream_t st) {
  using C = DI8Cfg<CIN, COUT>;
  a.tiles_x = (a.OW + C::TW - 1) / C::TW;
  a.tiles_y = (a.OH + C::TH - 1) / C::TH;
  const long tiles = (long)a.tiles_x * a.tiles_y * a.N;
  if (tiles > 0x7fffffffL - DI8_MAX_WORKGROUPS) return LFD_ERR_UNSUPPORTED;
  a.ntiles = (int)tiles;
  const int blocks = a.ntiles < DI8_MAX_WORKGROUPS ? a.ntiles : DI8_MAX_WORKGROUPS;
  hipLaunchKernelGGL((k_down_i8<CIN, COUT>), dim3((unsigned)blocks), dim3(256), 0, st, a);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

}  // namespace

extern "C" int lfd_block_i8_fused(int32_t n, int32_t h, int32_t w, const void* in, const void* w1_packed, const float* mult1,
                                  const float* biasq1, const void* w2_packed, const float* mult2, const float* biasq2,
                                  float res_mult, void* out_i8, void* out_f16, float out_scale, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!in || !w1_packed || !mult1 || !biasq1 || !w2_packed || !mult2 || !biasq2 || !out_i8) return LFD_ERR_INVALID_ARGUMENT;
  if (n < 1 || h < 1 || w < 1) return LFD_ERR_INVALID_ARGUMENT;
  if (!lfd_aligned16(in) || !lfd_aligned16(w1_packed) || !lfd_aligned16(mult1) || !lfd_aligned16(biasq1) ||
      !lfd_aligned16(w2_packed) || !lfd_aligned16(mult2) || !lfd_aligned16(biasq2) || !lfd_aligned16(out_i8) ||
      !lfd_aligned16(out_f16))
    return LFD_ERR_INVALID_ARGUMENT;
  if (in == out_i8) return LFD_ERR_INVALID_ARGUMENT;
  if ((long)h * w * 128 > 0x7fffffffL) return LFD_ERR_UNSUPPORTED;           // 32-bit offsets inside an image
  BI8Args a{};
  a.in = (const int8_t*)in; a.w1 = (const i32x4*)w1_packed; a.mult1 = mult1; a.biasq1 = biasq1;
  a.w2 = (const i32x4*)w2_packed; a.mult2 = mult2; a.biasq2 = biasq2;
  a.out_i8 = (int8_t*)out_i8; a.out_f16 = (_Float16*)out_f16; a.res_mult = res_mult; a.out_scale = out_scale;
  a.N = n; a.H = h; a.W = w;
  a.tiles_x = (w + BI8::TW - 1) / BI8::TW;
  a.tiles_y = (h + BI8::TH - 1) / BI8::TH;
  const long tiles = (long)a.tiles_x * a.tiles_y * n;
  if (tiles > 0x7fffffffL - BI8_MAX_WORKGROUPS) return LFD_ERR_UNSUPPORTED;
  a.ntiles = (int)tiles;
  static unsigned long long attr_set = 0;       // bit = device ordinal
  const int dev = lfd_device_ordinal();
  if (LFD_ONCE_PER_DEVICE(attr_set, dev)) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_block_i8), hipFuncAttributeMaxDynamicSharedMemorySize,
                            BI8::LDS_BYTES) != hipSuccess)
      return LFD_ERR_LAUNCH_FAILED;
    LFD_DONE_ON_DEVICE(attr_set, dev);
  }
  const int blocks = a.ntiles < BI8_MAX_WORKGROUPS ? a.ntiles : BI8_MAX_WORKGROUPS;
  hipLaunchKernelGGL(k_block_i8, dim3((unsigned)blocks), dim3(512), BI8::LDS_BYTES, st, a);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
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
  DI8Args a{};
  a.in = (const int8_t*)in; a.w = (const i32x4*)w_packed; a.mult = mult; a.biasq = biasq;
  a.wd = (const i32x4*)ds_w_packed; a.multd = ds_mult; a.biasqd = ds_biasq;
  a.out_i8 = (int8_t*)out_i8; a.ds_out_i8 = (int8_t*)ds_out_i8;
  a.N = n; a.H = h; a.W = w;
  a.OH = (h - 1) / 2 + 1;
  a.OW = (w - 1) / 2 + 1;
  if (cin == 64) return cout == 64 ? launch_down_i8<64, 64>(a, st) : launch_down_i8<64, 128>(a, st);
  return launch_down_i8<128, 128>(a, st);
}
