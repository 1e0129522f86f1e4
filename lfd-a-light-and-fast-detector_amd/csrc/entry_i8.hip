// csrc/entry_i8.hip -- the INT8 deployment mode's one-launch 64-channel stage-entry block (the fused='full' route):
//   xq  = the int8 input (format 0), or clamp(rint((float)x * in_inv_scale)) of the fp16 stem map on its way into LDS (format 1)
//   y1  = ReLU(conv1(xq)), 3x3 stride 2 pad 1          id = downsample(xq), 1x1 stride 2, no ReLU
//   out = ReLU(conv2(y1) + id), 3x3 stride 1 pad 1
// all three convs 64 -> 64 (padded) channels, the operands of lfd_conv2d_downsample_nhwc_i8 + lfd_conv2d_nhwc_i8 (and of the
// quantise launch in front of them).  The i32 sums are exact in any order and the epilogue steps are the functions of
// csrc/i8_impl.h that conv_i8.hip calls (the lane map and the LDS pixel pitch are stated there too), so the launch is required
// to equal the launches it replaces in every bit (tests/test_gpu_entry_i8_exact.py).
//
// The cut is csrc/block_i8.hip's producer / consumer one, with a 4 x 16 output tile so that every LDS buffer can be doubled:
//   * one 512-thread workgroup per CU, persistent, walking (image, tile) with stride gridDim.x (<= EI8_MAX_WORKGROUPS).  Waves
//     0-3 are producers (conv1 and the 1x1), waves 4-7 consumers (conv2 and the output stores); wave w and wave w + 4 share a
//     SIMD.
//   * filters are stationary: a producer wave owns one 32-channel slab of conv1 (72 VGPRs) and of the 1x1 (8 VGPRs), a consumer
//     wave one slab of conv2 (72 VGPRs), read once per workgroup in the ops.pack_conv_weight_i8 order.
//   * per output tile the y1 tile is 6 x 18 (conv2's halo) = 108 pixels, numbered linearly over four 32-pixel MFMA tiles, two
//     per producer pixel group, and the input halo is 13 x 37 pixels (80-byte LDS pixels).  y1 pixels outside
//     the oh x ow map are conv2's zero padding and are written as 0; input pixels outside the image are 0.
//   * the 1x1 reads conv1's centre tap.  Producer wave w computes exactly the (pixel tile, channel slab) of id that consumer
//     wave w + 4 adds, in the same lane layout, so id crosses as one 16-byte LDS slot per (wave, lane).
//   * software pipeline, ONE barrier per step: in step s the producers contract tile s from in[s & 1] into y1[s & 1] and
//     id[s & 1] and the consumers contract tile s - 1 from y1[(s - 1) & 1], requantise and store it, while the halo of tile
//     s + 1 travels through the registers of all 512 threads (4 pieces of 16 channels each), is converted (format 1) and is
//     written to in[(s + 1) & 1] at the end of the step.  The producers last read in[(s + 1) & 1] and the consumers last read
//     y1 / id[s & 1] in step s - 1: both before this step's barrier.
//   * LDS: 2 x 38480 (input) + 2 x 8640 (y1) + 2 x 4096 (id) = 102432 bytes, dynamic.  hipcc reports 166 VGPRs (format 0) and
//     219 VGPRs (format 1), no AGPRs, no scratch.
#include "i8_impl.h"

namespace {

constexpr int EI8_MAX_WORKGROUPS = 256;     // one 512-thread workgroup per CU

struct EI8Args {
  const void* in;          // FMT 0: int8 [N,H,W,64]; FMT 1: fp16 [N,H,W,cin]
  const i32x4* w1;         // conv1, packed [2][18][64 lanes]
  const float* mult1;
  const float* biasq1;
  const i32x4* wd;         // 1x1, packed [2][2][64 lanes]
  const float* multd;
  const float* biasqd;
  const i32x4* w2;         // conv2, packed [2][18][64 lanes]
  const float* mult2;
  const float* biasq2;
  int8_t* out_i8;          // [N,OH,OW,64]
  float res_mult, in_inv_scale;
  int N, H, W, OH, OW, cin;
  int tiles_x, tiles_y, ntiles;
};

struct EI8 {
  static constexpr int TH = 4, TW = 16;                 // output tile; MFMA pixel tile pg = rows 2 pg, 2 pg + 1
  static constexpr int MH = TH + 2, MW = TW + 2;        // y1 tile (conv1's output with conv2's halo)
  static constexpr int MPIX = MH * MW;                  // 108
  static constexpr int IH = (MH - 1) * 2 + 3, IW = (MW - 1) * 2 + 3;       // input halo tile, 13 x 37
  static constexpr int IPIX = IH * IW;                  // 481
  static constexpr int PITCH = 64 + 16;                 // bytes per LDS pixel (16 of bank spread), input and y1
  static constexpr int IN_BYTES = IPIX * PITCH;         // 38480
  static constexpr int MID_BYTES = MPIX * PITCH;        // 8640
  static constexpr int ID_BYTES = 4 * 64 * 16;          // one 16-byte slot per (producer wave, lane)
  static constexpr int PIECES = IPIX * 4;               // 16-channel pieces of the input halo
  static constexpr int NIT = (PIECES + 511) / 512;      // per thread: 4
  static constexpr int NK = 18;                         // k-steps of a 3x3x64 contraction
  static constexpr int OFF_IN = 0;
  static constexpr int OFF_MID = 2 * IN_BYTES;
  static constexpr int OFF_ID = OFF_MID + 2 * MID_BYTES;
  static constexpr int LDS_BYTES = OFF_ID + 2 * ID_BYTES;        // 102432
};
static_assert(EI8::LDS_BYTES <= 160 * 1024, "LDS capacity");
static_assert(EI8::MPIX <= 4 * 32, "y1 tile over four MFMA pixel tiles");

template <int FMT>
__global__ __launch_bounds__(512) void k_entry_i8(const EI8Args a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool prod = wv < 4;
  const int ct = wv & 1, pg = (wv >> 1) & 1;            // channel slab, pixel group of this wave within its role
  const int grid = gridDim.x;
  const int my = (a.ntiles - (int)blockIdx.x + grid - 1) / grid;       // tiles of this workgroup (>= 1: grid <= ntiles)

  // stationary: the wave's filter slab of conv1 (producers) or conv2 (consumers), and the producers' 1x1 slab
  i32x4 ws[EI8::NK];
  {
    const i32x4* wl = (prod ? a.w1 : a.w2) + (size_t)ct * EI8::NK * 64 + lane;
#pragma unroll
    for (int k = 0; k < EI8::NK; ++k) ws[k] = wl[(size_t)k * 64];
  }
  i32x4 wd[2];
#pragma unroll
  for (int q = 0; q < 2; ++q) wd[q] = a.wd[(size_t)(ct * 2 + q) * 64 + lane];      // (the consumers never use theirs)

  // input halo of tile t: memory -> registers (all 512 threads) -> LDS.  The load is i8_impl.h's i8_halo_load with an element size
  // and a runtime channel count (chunks at or above a.cin are 0), and stands here as this kernel's own copy: called through the
  // shared template -- in every shape tried, the element size and the narrow check as template arguments included -- hipcc
  // evaluates the bounds checks in another order and the kernel's assembly changes, and this kernel is required to stay the
  // parent's instruction for instruction (profiles/i8_impl_isa_equality.txt).  The LDS slot is the shared i8_halo_slot.
  auto load_halo = [&](int tid, int t, I8Piece<FMT + 1> (&v)[EI8::NIT]) {
    const I8Tile tl = i8_tile_of(t, a.tiles_x, a.tiles_y);
    const int esz = FMT == 0 ? 1 : 2;
    const char* in_img = (const char*)a.in + (size_t)tl.n * a.H * a.W * a.cin * esz;
#pragma unroll
    for (int it = 0; it < EI8::NIT; ++it) {
      const int i = tid + 512 * it;
      const int pix = i >> 2, ck = i & 3;
      const int iy = pix / EI8::IW, ix = pix - iy * EI8::IW;
      const int gy = tl.ty * EI8::TH * 2 - 3 + iy, gx = tl.tx * EI8::TW * 2 - 3 + ix;
      const bool ok = i < EI8::PIECES && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W && ck * 16 < a.cin;
      const char* src = in_img + (ok ? ((gy * a.W + gx) * a.cin + ck * 16) * esz : 0);     // < h * w * 128 < 2^31
      v[it].u[0] = *reinterpret_cast<const uint4*>(src);
      if (FMT == 1) v[it].u[FMT] = *reinterpret_cast<const uint4*>(src + (ok ? 16 : 0));
      if (!ok) {
        v[it].u[0] = make_uint4(0u, 0u, 0u, 0u);         // 0 stays 0 through the quantisation below
        if (FMT == 1) v[it].u[FMT] = make_uint4(0u, 0u, 0u, 0u);
      }
    }
  };
  auto store_halo = [&](int tid, int buf, const I8Piece<FMT + 1> (&v)[EI8::NIT]) {
    char* dst = smem + EI8::OFF_IN + buf * EI8::IN_BYTES;
#pragma unroll
    for (int it = 0; it < EI8::NIT; ++it) {
      const int i = tid + 512 * it;
      uint4 o;
      if (FMT == 0) {
        o = v[it].u[0];
      } else {
        // lfd_quantize_nhwc_f16_i8's value: one fp32 multiply, round half even, clamp
        union { uint4 u[2]; _Float16 h[16]; } x;
        x.u[0] = v[it].u[0];
        x.u[1] = v[it].u[FMT];
        float p[16];
#pragma unroll
        for (int g = 0; g < 16; ++g) p[g] = (float)x.h[g] * a.in_inv_scale;
        o = i8_requant16_fast<-127>(p);
      }
      if (i < EI8::PIECES) *reinterpret_cast<uint4*>(dst + i8_halo_slot<64>(i)) = o;
    }
  };

  I8Piece<FMT + 1> hv[EI8::NIT];
  load_halo(tid, blockIdx.x, hv);
  store_halo(tid, 0, hv);

  for (int s = 0; s <= my; ++s) {
    __syncthreads();      // in[s & 1], y1 / id[(s - 1) & 1] are complete; y1 / id[s & 1] and in[(s + 1) & 1] are free
    // the per-lane geometry below is recomputed per tile (a few VALU instructions) instead of being hoisted out of the loop
    // into registers the stationary filter needs
    int tl = threadIdx.x;
    asm volatile("" : "+v"(tl));
    const int p = tl & 31, kh = (tl >> 5) & 1;
    const int c0 = 32 * ct + 16 * kh;                   // the lane's 16 output channels
    const int ly = 2 * pg + (p >> 4), lx = p & 15;      // the lane's pixel of output MFMA tile pg (1x1 and conv2)
    const bool more = s + 1 < my;
    if (more) load_halo(tl, (int)blockIdx.x + (s + 1) * grid, hv);        // travels while this step's tiles are contracted
    if (prod) {
      if (s < my) {
        // -------------------------------------------------------------------------------- producer: conv1 and 1x1 of tile s
        const I8Tile ti = i8_tile_of((int)blockIdx.x + s * grid, a.tiles_x, a.tiles_y);
        const char* in_t = smem + EI8::OFF_IN + (s & 1) * EI8::IN_BYTES;
        char* mid_t = smem + EI8::OFF_MID + (s & 1) * EI8::MID_BYTES;
        char* id_t = smem + EI8::OFF_ID + (s & 1) * EI8::ID_BYTES;

        // the identity branch: output (ly, lx) = y1 tile (ly + 1, lx + 1), whose centre tap is halo (2 ly + 3, 2 lx + 3)
        {
          i32x16 accd;
#pragma unroll
          for (int g = 0; g < 16; ++g) accd[g] = 0;
          const int dbase = ((2 * ly + 3) * EI8::IW + 2 * lx + 3) * EI8::PITCH + kh * 16;
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const i32x4 b = *reinterpret_cast<const i32x4*>(in_t + dbase + q * 32);
            accd = __builtin_amdgcn_mfma_i32_32x32x32_i8(wd[q], b, accd, 0, 0, 0);
          }
          float vv[16], mm[16], bb[16];
          load16f(a.multd + c0, mm);
          load16f(a.biasqd + c0, bb);
#pragma unroll
          for (int g = 0; g < 16; ++g) vv[g] = i8_affine(accd[g], mm[g], bb[g]);
          *reinterpret_cast<uint4*>(id_t + (tl & 255) * 16) = i8_requant16_fast<-127>(vv);
        }

        // y1 pixel m = (2 pg + pt) * 32 + p, linear over 6 x 18; y1 (row, col), tap (dy, dx) = halo (2 row + dy, 2 col + dx)
        float mm[16], bb[16];
        load16f(a.mult1 + c0, mm);
        load16f(a.biasq1 + c0, bb);
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {
          const int m = (pg * 2 + pt) * 32 + p;
          const bool mval = m < EI8::MPIX;
          const int mc = mval ? m : EI8::MPIX - 1;
          const int mrow = mc / EI8::MW, mcol = mc - mrow * EI8::MW;
          const int pbase = (2 * mrow * EI8::IW + 2 * mcol) * EI8::PITCH + kh * 16;
          i32x16 acc;
#pragma unroll
          for (int g = 0; g < 16; ++g) acc[g] = 0;
#pragma unroll
          for (int k = 0; k < EI8::NK; ++k) {
            const int tp = k >> 1, q = k & 1, dy = tp / 3, dx = tp - dy * 3;
            const i32x4 b = *reinterpret_cast<const i32x4*>(in_t + pbase + (dy * EI8::IW + dx) * EI8::PITCH + q * 32);
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(ws[k], b, acc, 0, 0, 0);
          }
          // epilogue: y1 = clamp(rint(max(fmaf(acc, mult1, biasq1), 0))); 0 outside the oh x ow map (conv2's padding)
          float vv[16];
#pragma unroll
          for (int g = 0; g < 16; ++g) vv[g] = i8_affine(acc[g], mm[g], bb[g]);
          uint4 o = i8_requant16_fast<0>(vv);            // ReLU in the clamp
          const int gy = ti.ty * EI8::TH - 1 + mrow, gx = ti.tx * EI8::TW - 1 + mcol;
          if (gy < 0 || gy >= a.OH || gx < 0 || gx >= a.OW) o = make_uint4(0u, 0u, 0u, 0u);
          if (mval) *reinterpret_cast<uint4*>(mid_t + m * EI8::PITCH + c0) = o;
        }
      }
    } else {
      // ---------------------------------------------------------------------------- consumer: conv2 + store of tile s - 1
      if (s >= 1) {
        const I8Tile ti = i8_tile_of((int)blockIdx.x + (s - 1) * grid, a.tiles_x, a.tiles_y);
        const char* mid_t = smem + EI8::OFF_MID + ((s - 1) & 1) * EI8::MID_BYTES;
        const char* id_t = smem + EI8::OFF_ID + ((s - 1) & 1) * EI8::ID_BYTES;

        // out (ly, lx) reads y1 tile (ly + dy, lx + dx)
        const int cbase = (ly * EI8::MW + lx) * EI8::PITCH + kh * 16;
        i32x16 acc;
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[g] = 0;
#pragma unroll
        for (int k = 0; k < EI8::NK; ++k) {
          const int tp = k >> 1, q = k & 1, dy = tp / 3, dx = tp - dy * 3;
          const i32x4 b = *reinterpret_cast<const i32x4*>(mid_t + cbase + (dy * EI8::MW + dx) * EI8::PITCH + q * 32);
          acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(ws[k], b, acc, 0, 0, 0);
        }
        // epilogue: lfd_conv2d_nhwc_i8's with a residual and ReLU; the identity is producer wave wv - 4's slot of this lane
        I8x16 r;
        r.u = *reinterpret_cast<const uint4*>(id_t + (tl & 255) * 16);
        float vv[16], mm[16], bb[16];
        load16f(a.mult2 + c0, mm);
        load16f(a.biasq2 + c0, bb);
#pragma unroll
        for (int g = 0; g < 16; ++g) vv[g] = i8_residual(i8_affine(acc[g], mm[g], bb[g]), r.b[g], a.res_mult);
        const uint4 o = i8_requant16_fast<0>(vv);        // ReLU in the clamp
        const int oy = ti.ty * EI8::TH + ly, ox = ti.tx * EI8::TW + lx;
        if (oy < a.OH && ox < a.OW)
          *reinterpret_cast<uint4*>(a.out_i8 + ((size_t)ti.n * a.OH * a.OW + (size_t)(oy * a.OW + ox)) * 64 + c0) = o;
      }
    }
    if (more) store_halo(tl, (s + 1) & 1, hv);
  }
}

template <int FMT>
int launch_entry_i8(const EI8Args& a, int blocks, hipStream_t st) {
  static unsigned long long attr_set = 0;       // bit = device ordinal
  const int dev = lfd_device_ordinal();
  if (LFD_ONCE_PER_DEVICE(attr_set, dev)) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&k_entry_i8<FMT>), hipFuncAttributeMaxDynamicSharedMemorySize,
                            EI8::LDS_BYTES) != hipSuccess)
      return LFD_ERR_LAUNCH_FAILED;
    LFD_DONE_ON_DEVICE(attr_set, dev);
  }
  hipLaunchKernelGGL(k_entry_i8<FMT>, dim3((unsigned)blocks), dim3(512), EI8::LDS_BYTES, st, a);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

}  // namespace

extern "C" int lfd_entry_i8_fused_supported(int32_t in_format, int32_t in_channels) {
  if (in_format == 0 && in_channels == 64) return LFD_OK;
  if (in_format == 1 && (in_channels == 32 || in_channels == 48 || in_channels == 64)) return LFD_OK;
  return LFD_ERR_UNSUPPORTED;
}

extern "C" int lfd_entry_i8_fused(int32_t n, int32_t h, int32_t w, int32_t in_format, int32_t in_channels, const void* in,
                                  float in_inv_scale, const void* w1_packed, const float* mult1, const float* biasq1,
                                  const void* ds_w_packed, const float* ds_mult, const float* ds_biasq, const void* w2_packed,
                                  const float* mult2, const float* biasq2, float res_mult, void* out_i8, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!in || !w1_packed || !mult1 || !biasq1 || !ds_w_packed || !ds_mult || !ds_biasq || !w2_packed || !mult2 || !biasq2 || !out_i8)
    return LFD_ERR_INVALID_ARGUMENT;
  if (n < 1 || h < 1 || w < 1) return LFD_ERR_INVALID_ARGUMENT;
  const int rc = lfd_entry_i8_fused_supported(in_format, in_channels);
  if (rc != LFD_OK) return rc;
  if (!lfd_aligned16(in) || !lfd_aligned16(w1_packed) || !lfd_aligned16(mult1) || !lfd_aligned16(biasq1) ||
      !lfd_aligned16(ds_w_packed) || !lfd_aligned16(ds_mult) || !lfd_aligned16(ds_biasq) || !lfd_aligned16(w2_packed) ||
      !lfd_aligned16(mult2) || !lfd_aligned16(biasq2) || !lfd_aligned16(out_i8))
    return LFD_ERR_INVALID_ARGUMENT;
  if (in == out_i8) return LFD_ERR_INVALID_ARGUMENT;
  if ((long)h * w * 128 > 0x7fffffffL) return LFD_ERR_UNSUPPORTED;           // 32-bit offsets inside an image
  EI8Args a{};
  a.in = in; a.w1 = (const i32x4*)w1_packed; a.mult1 = mult1; a.biasq1 = biasq1;
  a.wd = (const i32x4*)ds_w_packed; a.multd = ds_mult; a.biasqd = ds_biasq;
  a.w2 = (const i32x4*)w2_packed; a.mult2 = mult2; a.biasq2 = biasq2;
  a.out_i8 = (int8_t*)out_i8; a.res_mult = res_mult; a.in_inv_scale = in_inv_scale;
  a.N = n; a.H = h; a.W = w; a.cin = in_channels;
  a.OH = (h - 1) / 2 + 1;
  a.OW = (w - 1) / 2 + 1;
  const int blocks = i8_tile_grid(a, n, a.OH, a.OW, EI8::TH, EI8::TW, EI8_MAX_WORKGROUPS);
  if (!blocks) return LFD_ERR_UNSUPPORTED;
  return in_format == 0 ? launch_entry_i8<0>(a, blocks, st) : launch_entry_i8<1>(a, blocks, st);
}
