// csrc/block_i8.hip -- the INT8 deployment mode's one-launch 64-channel residual block.  It computes exactly what the
// layer-by-layer launches of csrc/conv_i8.hip compute -- the i32 sums are exact in any order and the epilogues are the same
// functions of csrc/i8_impl.h, which also states the lane map and the LDS pixel pitch -- so the results are required to agree in
// every bit (tests/test_gpu_block_i8_exact.py).  (The stage-entry pair lfd_conv2d_downsample_nhwc_i8 is an instance of
// csrc/conv_i8.hip's kernel.)
//
// lfd_block_i8_fused: y = ReLU(conv2(ReLU(conv1(x))) + x), both convs 3x3 stride 1 pad 1, 64 -> 64, the int8 tensors and
// constants of two lfd_conv2d_nhwc_i8 calls.  The cut is csrc/block.hip's (PRODUCER / CONSUMER wave specialisation):
//   * one 512-thread workgroup per CU, persistent, walking (image, tile) with stride gridDim.x (<= BI8_MAX_WORKGROUPS).  Waves
//     0-3 are conv1 producers, waves 4-7 conv2 consumers; wave w and wave w + 4 share a SIMD, so each matrix pipe serves one
//     producer and one consumer and the one's loads, epilogue and stores run under the other's MFMAs.
//   * both filters are stationary: a wave owns one 32-channel slab of ONE conv, 18 k-steps of 16 bytes per lane = 72 VGPRs,
//     read once per workgroup in the ops.pack_conv_weight_i8 order (nothing is repacked).  The lane's 16 mult / biasq values
//     are re-read per tile (cache-hot): the registers go to the filter.
//   * per 8 x 16 output tile the producers contract the 12 x 20 input halo (LDS) into the 10 x 18 mid tile: 180 pixels numbered
//     linearly over six 32-pixel MFMA tiles, three per producer pixel group (93.75 % of the slots useful, recompute factor
//     (192 + 128) / 256 = 1.25).  The mid tile is int8 in LDS only, one 16-byte write per lane; mid pixels outside the image
//     are conv2's zero padding and are written as 0, not as conv1 evaluated there.
//   * software pipeline, ONE barrier per step: in step s the producers contract tile s from in[s & 1] into mid[s & 1] while
//     the halo of tile s + 1 travels through their registers into in[(s + 1) & 1], and the consumers contract tile s - 1 from
//     mid[(s - 1) & 1], add the identity (a 16-byte load of x per lane, cache-hot: the producers just pulled those lines),
//     requantise and store.
//   * LDS: 2 x 19200 (input) + 2 x 14400 (mid) = 67200 bytes, dynamic.  hipcc reports 232 VGPRs, no AGPRs, no scratch.
#include "i8_impl.h"

namespace {

constexpr int BI8_MAX_WORKGROUPS = 256;     // one 512-thread workgroup per CU

struct BI8 : BlockI8Cfg<64> {
  static constexpr int OFF_IN = 0;
  static constexpr int OFF_MID = 2 * IN_BYTES;
  static constexpr int LDS_BYTES = OFF_MID + 2 * MID_BYTES;      // 67200
};
static_assert(BI8::LDS_BYTES <= 160 * 1024, "LDS capacity");

__global__ __launch_bounds__(512) void k_block_i8(const BlockI8Args a) {
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
  auto load_halo = [&](int tid, int t, I8Piece<> (&v)[BI8::NIT]) {
    const I8Tile tl = i8_tile_of(t, a.tiles_x, a.tiles_y);
    i8_halo_load<64, BI8::IW, BI8::PIECES, 2, 256, BI8::NIT>(v, a.in + (size_t)tl.n * a.H * a.W * 64, tid, 0, tl.ty * BI8::TH,
                                                             tl.tx * BI8::TW, a.H, a.W);
  };
  auto store_halo = [&](int tid, int buf, const I8Piece<> (&v)[BI8::NIT]) {
    i8_halo_store<64, BI8::PIECES, 256, BI8::NIT>(smem + BI8::OFF_IN + buf * BI8::IN_BYTES, v, tid, 0);
  };

  I8Piece<> hv[BI8::NIT];
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
        const I8Tile ti = i8_tile_of(t, a.tiles_x, a.tiles_y);
        const bool more = s + 1 < my;
        if (more) load_halo(tl, t + grid, hv);              // travels while this tile is contracted
        const char* in_t = smem + BI8::OFF_IN + (s & 1) * BI8::IN_BYTES;
        char* mid_t = smem + BI8::OFF_MID + (s & 1) * BI8::MID_BYTES;

        // mid pixel m = (3 pg + pt) * 32 + p
        int pbase[3], mrow[3], mcol[3];
        bool mval[3];
#pragma unroll
        for (int pt = 0; pt < 3; ++pt) i8_block_mid_pixel<BI8>((pg * 3 + pt) * 32 + p, kh, pbase[pt], mrow[pt], mcol[pt], mval[pt]);
        // one MFMA tile at a time (16 accumulator registers live): the epilogue of one runs under the MFMAs of the next
        // epilogue: mid = requantised ReLU(conv1); 0 outside the image (conv2's padding)
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
          for (int g = 0; g < 16; ++g) vv[g] = i8_relu(i8_affine(acc[g], mm[g], bb[g]));
          uint4 o = i8_requant16(vv);
          const int gy = ti.ty * BI8::TH - 1 + mrow[pt], gx = ti.tx * BI8::TW - 1 + mcol[pt];
          if (gy < 0 || gy >= a.H || gx < 0 || gx >= a.W) o = make_uint4(0u, 0u, 0u, 0u);
          if (mval[pt]) *reinterpret_cast<uint4*>(mid_t + ((pg * 3 + pt) * 32 + p) * BI8::PITCH + c0) = o;
        }
        if (more) store_halo(tl, (s + 1) & 1, hv);
      }
    } else if (s >= 1) {
      // ---------------------------------------------------------------------------------------- consumer: conv2 of tile s - 1
      const I8Tile ti = i8_tile_of((int)blockIdx.x + (s - 1) * grid, a.tiles_x, a.tiles_y);
      const char* mid_t = smem + BI8::OFF_MID + ((s - 1) & 1) * BI8::MID_BYTES;

      // MFMA pixel tile 2 pg + j = output rows 2 (2 pg + j), + 1 of the tile
      int cbase[2];
      size_t opix[2];
      bool ook[2];
      I8x16 r[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        i8_block_out_pixel<BI8>(a, ti, 2 * (2 * pg + j) + (p >> 4), p & 15, kh, c0, cbase[j], opix[j], ook[j]);
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
        for (int g = 0; g < 16; ++g) vv[g] = i8_relu(i8_residual(i8_affine(acc[j][g], mm[g], bb[g]), r[j].b[g], a.res_mult));
        const uint4 o = i8_requant16(vv);
        if (ook[j]) *reinterpret_cast<uint4*>(a.out_i8 + opix[j]) = o;
        if (a.out_f16) {        // (wave-uniform) a pyramid tap
          F16x16 f;
#pragma unroll
          for (int g = 0; g < 16; ++g) f.h[g] = i8_tap(acc[j][g], mm[g], bb[g], true, r[j].b[g], a.res_mult, true, a.out_scale);
          if (ook[j]) {
            *reinterpret_cast<uint4*>(a.out_f16 + opix[j]) = f.u[0];
            *reinterpret_cast<uint4*>(a.out_f16 + opix[j] + 8) = f.u[1];
          }
        }
      }
    }
  }
}

}  // namespace

extern "C" int lfd_block_i8_fused(int32_t n, int32_t h, int32_t w, const void* in, const void* w1_packed, const float* mult1,
                                  const float* biasq1, const void* w2_packed, const float* mult2, const float* biasq2,
                                  float res_mult, void* out_i8, void* out_f16, float out_scale, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  BlockI8Args a{};
  int blocks = 0;
  const int rc = i8_block_args<BI8>(a, blocks, BI8_MAX_WORKGROUPS, n, h, w, in, w1_packed, mult1, biasq1, w2_packed, mult2, biasq2,
                                    res_mult, out_i8, out_f16, out_scale);
  if (rc != LFD_OK) return rc;
  static unsigned long long attr_set = 0;       // bit = device ordinal
  const int dev = lfd_device_ordinal();
  if (LFD_ONCE_PER_DEVICE(attr_set, dev)) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_block_i8), hipFuncAttributeMaxDynamicSharedMemorySize,
                            BI8::LDS_BYTES) != hipSuccess)
      return LFD_ERR_LAUNCH_FAILED;
    LFD_DONE_ON_DEVICE(attr_set, dev);
  }
  hipLaunchKernelGGL(k_block_i8, dim3((unsigned)blocks), dim3(512), BI8::LDS_BYTES, st, a);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}
