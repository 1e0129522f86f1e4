// csrc/block128_i8.hip -- the INT8 deployment mode's one-launch 128-channel residual block (the block128 option):
//   y = ReLU(conv2(ReLU(conv1(x))) + x), both convs 3x3 stride 1 pad 1, 128 -> 128, the int8 tensors and constants of the two
// lfd_conv2d_nhwc_i8 calls it replaces.  The i32 sums are exact in any order and the epilogue steps are the functions of
// csrc/i8_impl.h that conv_i8.hip calls (the compare / select requantisation included), so the results are required to agree in every bit
// (tests/test_gpu_block128_i8_exact.py).
//
// One filter is 147456 bytes: neither fits LDS next to a tile, and a producer / consumer cut like csrc/block_i8.hip's would leave
// a wave 112 registers beside its 144-register slab.  The cut here is ONE WAVE PER SIMD with both filters stationary:
//   * one 256-thread workgroup per CU, persistent, walking (image, tile) with stride gridDim.x (<= B128I8_MAX_WORKGROUPS).  Wave
//     w owns output channels 32 w .. 32 w + 31 of BOTH convs: 2 x 36 k-steps of 16 bytes per lane = 288 registers, read once per
//     workgroup in the ops.pack_conv_weight_i8 order (nothing is repacked).  240 of them (conv1's slab and NK2A k-steps of
//     conv2's) are pinned to AGPRs, which an MFMA reads as its A operand directly (keep_in_agpr below: left alone the compiler
//     copies them to VGPRs in front of every MFMA and spills); the other 48 are VGPRs.  Every wave contracts every pixel of the
//     tile against its slab.
//   * per 8 x 16 output tile: the 12 x 20 input halo (LDS, 144-byte pixels: 128 channels + 16 of bank spread) is contracted
//     into the 10 x 18 mid tile, 180 pixels numbered linearly over six 32-pixel MFMA tiles (93.75 % of the slots useful), two
//     MFMA tiles at a time (two independent accumulator chains).  The mid tile is int8 in LDS only, 144-byte pixels, one
//     16-byte write per lane; mid pixels outside the image are conv2's zero padding and are written as 0, not as conv1
//     evaluated there.  Input halo pixels outside the image are 0 (load from a clamped address + select).  A barrier, then
//     conv2 contracts the mid tile into the four MFMA tiles (2 rows x 16) of the output, again two at a time, adds the identity
//     (the halo tile in LDS holds it), requantises and stores.  Ragged tiles are guarded on the store.
//   * the contraction is software-pipelined by hand (contract2): stages of two k-steps, the four LDS reads of the next stage in
//     front of the four MFMAs of this one.  One wave per SIMD has nobody to hide an LDS read behind.
//   * two barriers per tile.  The halo of the workgroup's next tile travels from memory in two halves of four 16-byte pieces
//     per thread, one under each conv, into the other input buffer; the mid buffer is single (conv1 of the next tile writes it
//     behind the next barrier).
//   * v_mfma_i32_32x32x32_i8 with A = filter, B = pixels and the lane map of csrc/i8_impl.h: a lane ends with 16 consecutive
//     channels of its pixel.
//   * LDS: 2 x 34560 (input) + 25920 (mid) = 95040 bytes, dynamic.  hipcc reports 192 VGPRs + 240 AGPRs without the tap and
//     256 + 254 with it (the float64 tap epilogue), no scratch in either; 1 wave per SIMD.
#include "i8_impl.h"

namespace {

constexpr int B128I8_MAX_WORKGROUPS = 256;  // one 256-thread workgroup per CU, one wave per SIMD

// an MFMA's A operand may be an AGPR: this pins a filter fragment to the accumulator half of the unified register file where it
// is used, so that the allocator keeps it there across the tile loop instead of copying it to a VGPR in front of every MFMA
__device__ __forceinline__ void keep_in_agpr(i32x4& w) { asm("" : "+a"(w)); }

struct B128I8 : BlockI8Cfg<128> {
  static constexpr int NITH = NIT / 2;                  // the halo's 8 pieces per thread travel in two halves of 4
  static constexpr int NK2A = 24;                       // k-steps of conv2's slab held in AGPRs next to all of conv1's (240 of 256)
  static constexpr int MPAIRS = (MPIX + 63) / 64;       // pairs of MFMA pixel tiles of the mid tile: 3
  static constexpr int OPAIRS = TH / 4;                 // of the output tile: 2
  static constexpr int OFF_IN = 0;
  static constexpr int OFF_MID = 2 * IN_BYTES;
  static constexpr int LDS_BYTES = OFF_MID + MID_BYTES;           // 95040
};
static_assert(B128I8::LDS_BYTES <= 160 * 1024, "LDS capacity");
static_assert(B128I8::TH % 4 == 0 && B128I8::TW == 16, "an MFMA pixel tile is 2 rows of 16; conv2 runs them in pairs");

// One contraction on two accumulator chains: acc[j] += filter slab x pixels of MFMA pixel tile j, j = 0, 1, over the 36
// k-steps of a 3x3x128 window.  base + pb[j]: the lane's fragment of tap (0, 0), k-step 0 of its pixel in an LDS tile of ROWW
// pixels per row.  Software pipeline in stages of two k-steps (four 16-byte LDS reads, four MFMAs): the reads of stage st + 1 are
// issued in front of the MFMAs of stage st; the scheduling barriers keep that order (left alone, the compiler issues each read
// right in front of the MFMA that waits for it).  The first NA k-steps of the slab are pinned to AGPRs.
template <int ROWW, int NA>
__device__ __forceinline__ void contract2(const char* base, const int (&pb)[2], i32x4 (&w)[B128I8::NK], i32x16 (&acc)[2]) {
  using B = B128I8;
  constexpr int NST = B::NK / 2;
  static_assert(NST % 2 == 0, "the stage loop runs pairs");
  auto ld = [&](int st, i32x4 (&b)[2][2]) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int k = 2 * st + kk, tp = k / B::NQ, q = k - tp * B::NQ, dy = tp / 3, dx = tp - dy * 3;
#pragma unroll
      for (int j = 0; j < 2; ++j)
        b[j][kk] = *reinterpret_cast<const i32x4*>(base + pb[j] + (dy * ROWW + dx) * B::PITCH + q * 32);
    }
  };
  auto mm = [&](int st, const i32x4 (&b)[2][2]) {
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      const int k = 2 * st + kk;
      if (k < NA) keep_in_agpr(w[k]);
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[j] = __builtin_amdgcn_mfma_i32_32x32x32_i8(w[k], b[j][kk], acc[j], 0, 0, 0);
    }
  };
  i32x4 b0[2][2], b1[2][2];
  ld(0, b0);
#pragma unroll
  for (int st = 0; st < NST; st += 2) {
    ld(st + 1, b1);
    __builtin_amdgcn_sched_barrier(0);
    mm(st, b0);
    __builtin_amdgcn_sched_barrier(0);
    if (st + 2 < NST) ld(st + 2, b0);
    __builtin_amdgcn_sched_barrier(0);
    mm(st + 1, b1);
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <bool TAP>
__global__ __launch_bounds__(256) void k_block128_i8(const BlockI8Args a) {
  using B = B128I8;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, p = lane & 31, kh = lane >> 5;
  const int ct = __builtin_amdgcn_readfirstlane(tid >> 6);            // the wave's 32-channel slab of both convs
  const int c0 = 32 * ct + 16 * kh;                                   // the lane's 16 output channels
  const int grid = gridDim.x;
  const int my = (a.ntiles - (int)blockIdx.x + grid - 1) / grid;      // tiles of this workgroup (>= 1: grid <= ntiles)

  // half `part` of the input halo of tile t: memory -> registers -> LDS
  auto load_halo = [&](int t, int part, I8Piece<> (&v)[B::NITH]) {
    const I8Tile tl = i8_tile_of(t, a.tiles_x, a.tiles_y);
    i8_halo_load<B::C, B::IW, B::PIECES, 2, 256, B::NITH>(v, a.in + (size_t)tl.n * a.H * a.W * B::C, tid, part * B::NITH,
                                                             tl.ty * B::TH, tl.tx * B::TW, a.H, a.W);
  };
  auto store_halo = [&](int buf, int part, const I8Piece<> (&v)[B::NITH]) {
    i8_halo_store<B::C, B::PIECES, 256, B::NITH>(smem + B::OFF_IN + buf * B::IN_BYTES, v, tid, part * B::NITH);
  };

  I8Piece<> hv[B::NITH];
  load_halo(blockIdx.x, 0, hv);
  store_halo(0, 0, hv);
  load_halo(blockIdx.x, 1, hv);

  // stationary: the wave's slab of both filters, fetched in chunks of CHUNK k-steps so that no more than that many fragments
  // are on their way through VGPRs at a time
  i32x4 w1s[B::NK], w2s[B::NK];
  {
    constexpr int CHUNK = 4;
    static_assert(B::NK % CHUNK == 0 && B::NK2A % CHUNK == 0, "whole chunks");
    const i32x4* wl1 = a.w1 + (size_t)ct * B::NK * 64 + lane;
    const i32x4* wl2 = a.w2 + (size_t)ct * B::NK * 64 + lane;
#pragma unroll
    for (int k0 = 0; k0 < B::NK; k0 += CHUNK) {
#pragma unroll
      for (int k = k0; k < k0 + CHUNK; ++k) w1s[k] = wl1[(size_t)k * 64];
#pragma unroll
      for (int k = k0; k < k0 + CHUNK; ++k) keep_in_agpr(w1s[k]);
    }
#pragma unroll
    for (int k0 = 0; k0 < B::NK; k0 += CHUNK) {
#pragma unroll
      for (int k = k0; k < k0 + CHUNK; ++k) w2s[k] = wl2[(size_t)k * 64];
      if (k0 < B::NK2A) {
#pragma unroll
        for (int k = k0; k < k0 + CHUNK; ++k) keep_in_agpr(w2s[k]);
      }
    }
  }
  store_halo(0, 1, hv);

  char* const mid_t = smem + B::OFF_MID;
  for (int s = 0; s < my; ++s) {
    __syncthreads();      // in[s & 1] is complete; every wave is done reading mid (conv2 of tile s - 1)
    const int t = (int)blockIdx.x + s * grid;
    const I8Tile ti = i8_tile_of(t, a.tiles_x, a.tiles_y);
    const bool more = s + 1 < my;
    // the halo of the next tile travels in two halves, one under each conv, into in[(s + 1) & 1]: that buffer was last read in
    // step s - 1, before the barrier above
    if (more) load_halo(t + grid, 0, hv);
    const char* in_t = smem + B::OFF_IN + (s & 1) * B::IN_BYTES;

    // ------------------------------------------------------------------------------------------ conv1: input halo -> mid
    // mid pixel m = (2 pp + j) * 32 + p
#pragma unroll 1
    for (int pp = 0; pp < B::MPAIRS; ++pp) {
      int pbase[2], mrow[2], mcol[2];
      bool mval[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) i8_block_mid_pixel<B>((2 * pp + j) * 32 + p, kh, pbase[j], mrow[j], mcol[j], mval[j]);
      i32x16 acc[2];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[j][g] = 0;
      contract2<B::IW, B::NK>(in_t, pbase, w1s, acc);
      // epilogue: mid = requantised ReLU(conv1); 0 outside the image (conv2's padding)
      float mm[16], bb[16];
      load16f(a.mult1 + c0, mm);
      load16f(a.biasq1 + c0, bb);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        float vv[16];
#pragma unroll
        for (int g = 0; g < 16; ++g) vv[g] = i8_relu(i8_affine(acc[j][g], mm[g], bb[g]));
        uint4 o = i8_requant16(vv);
        const int gy = ti.ty * B::TH - 1 + mrow[j], gx = ti.tx * B::TW - 1 + mcol[j];
        if (gy < 0 || gy >= a.H || gx < 0 || gx >= a.W) o = make_uint4(0u, 0u, 0u, 0u);
        if (mval[j]) *reinterpret_cast<uint4*>(mid_t + ((2 * pp + j) * 32 + p) * B::PITCH + c0) = o;
      }
    }
    if (more) {
      store_halo((s + 1) & 1, 0, hv);
      load_halo(t + grid, 1, hv);
    }
    __syncthreads();      // mid is complete

    // ------------------------------------------------------------------------------------------ conv2: mid -> output
    // MFMA pixel tile 2 pp + j = output rows 2 (2 pp + j), + 1 of the tile
#pragma unroll 1
    for (int pp = 0; pp < B::OPAIRS; ++pp) {
      int cbase[2];
      size_t opix[2];
      bool ook[2];
      I8x16 r[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) i8_block_out_pixel<B>(a, ti, 2 * (2 * pp + j) + (p >> 4), p & 15, kh, c0, cbase[j], opix[j], ook[j]);
      i32x16 acc[2];
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[j][g] = 0;
      contract2<B::MW, B::NK2A>(mid_t, cbase, w2s, acc);
      // epilogue: lfd_conv2d_nhwc_i8's with a residual and ReLU; the identity is the centre of the input halo tile
      float mm[16], bb[16];
      load16f(a.mult2 + c0, mm);
      load16f(a.biasq2 + c0, bb);
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int ly = 2 * (2 * pp + j) + (p >> 4), lx = p & 15;
        r[j].u = *reinterpret_cast<const uint4*>(in_t + ((ly + 2) * B::IW + lx + 2) * B::PITCH + c0);
        float vv[16];
#pragma unroll
        for (int g = 0; g < 16; ++g) vv[g] = i8_relu(i8_residual(i8_affine(acc[j][g], mm[g], bb[g]), r[j].b[g], a.res_mult));
        const uint4 o = i8_requant16(vv);
        if (ook[j]) *reinterpret_cast<uint4*>(a.out_i8 + opix[j]) = o;
        if (TAP) {              // a pyramid tap
          F16x16 f;
#pragma unroll
          for (int g = 0; g < 16; ++g) {
            f.h[g] = i8_tap(acc[j][g], mm[g], bb[g], true, r[j].b[g], a.res_mult, true, a.out_scale);
            if ((g & 3) == 3) __builtin_amdgcn_sched_barrier(0);      // four elements' float64 temporaries at a time
          }
          if (ook[j]) {
            *reinterpret_cast<uint4*>(a.out_f16 + opix[j]) = f.u[0];
            *reinterpret_cast<uint4*>(a.out_f16 + opix[j] + 8) = f.u[1];
          }
        }
      }
    }
    if (more) store_halo((s + 1) & 1, 1, hv);
  }
}

template <bool TAP>
int launch_block128_i8(const BlockI8Args& a, int blocks, hipStream_t st) {
  static unsigned long long attr_set = 0;       // bit = device ordinal
  const int dev = lfd_device_ordinal();
  if (LFD_ONCE_PER_DEVICE(attr_set, dev)) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_block128_i8<TAP>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            B128I8::LDS_BYTES) != hipSuccess)
      return LFD_ERR_LAUNCH_FAILED;
    LFD_DONE_ON_DEVICE(attr_set, dev);
  }
  hipLaunchKernelGGL(k_block128_i8<TAP>, dim3((unsigned)blocks), dim3(256), B128I8::LDS_BYTES, st, a);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

}  // namespace

extern "C" int lfd_block128_i8_fused(int32_t n, int32_t h, int32_t w, const void* in, const void* w1_packed, const float* mult1,
                                     const float* biasq1, const void* w2_packed, const float* mult2, const float* biasq2,
                                     float res_mult, void* out_i8, void* out_f16, float out_scale, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  BlockI8Args a{};
  int blocks = 0;
  const int rc = i8_block_args<B128I8>(a, blocks, B128I8_MAX_WORKGROUPS, n, h, w, in, w1_packed, mult1, biasq1, w2_packed, mult2,
                                       biasq2, res_mult, out_i8, out_f16, out_scale);
  if (rc != LFD_OK) return rc;
  return out_f16 ? launch_block128_i8<true>(a, blocks, st) : launch_block128_i8<false>(a, blocks, st);
}
