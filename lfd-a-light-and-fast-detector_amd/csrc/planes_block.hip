// csrc/planes_block.hip -- k_pl_blk64: one residual block of the planes mode per launch (lfd_resnet.py:96-154, FasterBlock
// without a downsample branch):  m = split(ReLU(conv3x3(x) + b1)),  y = split(ReLU(conv3x3(m) + b2 + x)),  64 -> 64 -> 64.
//
// The two-launch form runs k_pl_c3p twice; the intermediate m goes to HBM as two fp16 planes and comes straight back.  Here a
// workgroup owns a STRIP of 30 output columns (32 mid columns = one MFMA pixel tile, 34 input columns) and walks down a
// segment of R rows, one row per step, with one barrier per step (the scheme of block_rows.hip):
//   * input ring (NIN rows of hi | lo, 144-byte pixel pitch) filled by LDS-DMA five steps ahead of its first use; the
//     identity of output row ol is input row ol + 2 of the same ring;
//   * mid ring (NMID rows of hi | lo): the split m, the rounding point of the two-launch path;
//   * the contraction index of each conv is split as in k_pl_c3p (KA = 18): wave pair (A, B) per 32-channel slab and conv.
//     A = bias + k-steps [0, 18) (+ the two identity k-steps in conv2), B = k-steps [18, 36); A hands main + 2^-11 corr of
//     its part to B through LDS, B adds it, ReLUs, splits -- one step later, behind the next barrier.
//     waves 0, 1: conv1 A (slab 0, 1) + the DMA;  2, 3: conv1 B + the mid epilogue;
//     waves 4, 5: conv2 B + the stores;           6, 7: conv2 A + the identity.
//     (waves w and w + 4 share a SIMD: each SIMD holds one wave of each conv, 144 filter registers per wave.)
// Step j: conv1 contracts mid row j (its B finishes mid row j - 1), conv2 contracts output row j - 4 (its B finishes row
// j - 5); T = R + 5 steps.  Every MFMA, sum and rounding is the one k_pl_c3p<false> then k_pl_c3p<true> performs for the
// element: the result is bit-identical to the two launches (tests/test_gpu_planes_block.py).
// Ring safety (tests/test_planes_block_schedule.py model-checks it): input row il is DMA'd at the end of step
// il - 5 and last read (identity) in step il + 2, so NIN >= 8; mid row ml is written in step ml + 1 and read in steps
// ml + 2 .. ml + 4, so NMID >= 4.
#include "planes_impl.h"

namespace pl {
namespace {

struct BlkArgs {
  const _Float16* in;     // hi plane [N,H,W,64]; lo plane in_plane halfs behind it
  long in_plane;
  _Float16* out;          // hi plane [N,H,W,64]; lo plane out_plane halfs behind it
  long out_plane;
  const half8* w1;        // packed [2][2 slabs][36][64] (lfd_pl_conv2d order)
  const float* b1;
  const half8* w2;
  const float* b2;
  const _Float16* zeros;  // 4 KB line: [0, 2048) zero
  int N, H, W;
  int strips, segs, SH, nwork;
};

struct PB {
  static constexpr int TW = 30, IW = 34;
  static constexpr int PIXB = 144;                       // 128 + 16: lane-linear DMA of 7 pixels x 9 chunks
  static constexpr int NDMA = 5;                         // instructions per row and plane
  static constexpr int IN_PLANE = IW * PIXB + 256;       // (+ slack behind the last DMA window)
  static constexpr int IN_SLOT = 2 * IN_PLANE;
  static constexpr int NIN = 8;
  static constexpr int MID_PLANE = IW * PIXB;            // conv2's lanes 30, 31 read two columns past the 32 mid columns
  static constexpr int MID_SLOT = 2 * MID_PLANE;
  static constexpr int NMID = 4;
  static constexpr int NK = 36, KA = 18, KB = NK - KA;
  static constexpr int LEAD = 5;                         // row il is issued at the end of step il - LEAD
  static constexpr int XCH = 64 * 16 * 4;                // one slab's hand-off: 64 lanes x 16 floats
  static constexpr int OFF_IN = 0;
  static constexpr int OFF_MID = OFF_IN + NIN * IN_SLOT;
  static constexpr int OFF_X1 = OFF_MID + NMID * MID_SLOT;       // [2 steps][2 slabs]
  static constexpr int OFF_X2 = OFF_X1 + 4 * XCH;
  static constexpr int OFF_BIAS = OFF_X2 + 4 * XCH;
  static constexpr int LDS_BYTES = OFF_BIAS + 2 * 64 * 4;
};
static_assert(pl::PB::LDS_BYTES <= 160 * 1024, "LDS capacity");
static_assert(pl::PB::NIN >= pl::PB::LEAD + 3 && pl::PB::NMID >= 4, "ring depths (see the header)");

struct PSeg { int n, oy0, ox0, R; };

// the DMA of one plane of input row il (gy = oy0 - 2 + il): 5 instructions, lane L carries chunk L % 9 of pixel 7 i + L / 9
// (chunk 8 and lane 63 masked off); rows / columns outside the image come from the zero line
__device__ __forceinline__ void pb_issue_row(const BlkArgs& a, char* smem, const PSeg& sg, int plane, int il, int slot) {
  const int ol = threadIdx.x & 63;
  const int px = (ol * 57) >> 9;                         // ol / 9
  const int ck = ol - 9 * px;
  const bool lane_on = ck < 8 && ol < 63;
  const int gy = sg.oy0 - 2 + il;
  const bool rv = gy >= 0 && gy < a.H && il < sg.R + 4;
  const char* rowp = reinterpret_cast<const char*>(a.in + (size_t)plane * a.in_plane) +
                     ((long)sg.n * a.H + (rv ? gy : 0)) * (long)a.W * 128;
  const char* zp = reinterpret_cast<const char*>(a.zeros) + (ck & 7) * 16;
  char* lrow = smem + pl::PB::OFF_IN + slot * pl::PB::IN_SLOT + plane * pl::PB::IN_PLANE;
#pragma unroll
  for (int i = 0; i < pl::PB::NDMA; ++i) {
    const int col = 7 * i + px;
    const int gx = sg.ox0 - 2 + col;
    const bool ok = rv && gx >= 0 && gx < a.W;
    const char* src = ok ? rowp + (long)gx * 128 + (ck & 7) * 16 : zp;
    if (lane_on && col < pl::PB::IW) dma16(src, lrow + i * 1008);
  }
}

__device__ __forceinline__ half8 pb_identity_fragment(int pix, int h, int qq) {
  int j0 = pix - 16 * qq - 8 * h;
  asm volatile("" : "+v"(j0));
  union { half8 v; uint32_t u[4]; } f;
#pragma unroll
  for (int r = 0; r < 4; ++r) f.u[r] = (j0 == 2 * r) ? 0x3c00u : ((j0 == 2 * r + 1) ? 0x3c000000u : 0u);
  return f.v;
}

// one conv of the block, one role: CONV2 = 0 (conv1, reads the input ring) | 1 (conv2, reads the mid ring); B = 0 (bias + k-steps
// [0, 18) (+ identity), hand-off) | 1 (k-steps [18, 36) + the epilogue of the previous row)
template <bool CONV2, bool B>
__device__ __forceinline__ void pb_role(const BlkArgs& a, char* smem, int ct, const PSeg& sg) {
  const int lane = threadIdx.x & 63;
  const int h = lane >> 5, pix = lane & 31;
  constexpr int K0 = B ? pl::PB::KA : 0;
  constexpr int KN = B ? pl::PB::KB : pl::PB::KA;
  constexpr int PD = 2;
  constexpr bool DMA = !CONV2 && !B;
  const int T = sg.R + 5;
  // conv1 contracts row j (mid), conv2 row j - 4 (output)
  const int row_lag = CONV2 ? 4 : 0;
  const int nrows = CONV2 ? sg.R : sg.R + 2;

  if (DMA) {
    for (int il = 0; il < pl::PB::LEAD; ++il) pb_issue_row(a, smem, sg, ct, il, il);
  }
  half8 wh[KN], wl[KN];
  {
    const half8* wsrc = (CONV2 ? a.w2 : a.w1) + (size_t)(ct * pl::PB::NK + K0) * 64 + lane;
    constexpr long WPL = 2L * pl::PB::NK * 64;
#pragma unroll
    for (int k = 0; k < KN; ++k) {
      wh[k] = wsrc[(size_t)k * 64];
      wl[k] = wsrc[WPL + (size_t)k * 64];
    }
  }
  const float* sbias = reinterpret_cast<const float*>(smem + pl::PB::OFF_BIAS) + (CONV2 ? 64 : 0);
  float* xch = reinterpret_cast<float*>(smem + (CONV2 ? pl::PB::OFF_X2 : pl::PB::OFF_X1)) + ct * (pl::PB::XCH / 4) + lane * 4;
  const int RING = CONV2 ? pl::PB::NMID : pl::PB::NIN;
  const int SLOT = CONV2 ? pl::PB::MID_SLOT : pl::PB::IN_SLOT;
  const int PLANE = CONV2 ? pl::PB::MID_PLANE : pl::PB::IN_PLANE;
  const char* ring = smem + (CONV2 ? pl::PB::OFF_MID : pl::PB::OFF_IN) + pix * pl::PB::PIXB + h * 16;

  float yp[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) yp[r] = 0.f;

  block_barrier();                     // biases visible
  for (int j = 0; j < T; ++j) {
    if (DMA) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * pl::PB::NDMA) : "memory");   // row j + 2 landed
    block_barrier();
    const int r0 = j - row_lag;        // the row this wave contracts in step j
    // ---- B: the epilogue of row r0 - 1 (contracted in step j - 1; A's part was handed off before this barrier)
    if constexpr (B) {
      const int re = r0 - 1;
      if (re >= 0 && re < nrows) {
        const float* xr = xch + ((j - 1) & 1) * (pl::PB::XCH / 2);
        float y[16];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4 pa = *reinterpret_cast<const float4*>(xr + g * 256);
          y[4 * g + 0] = fmaxf(yp[4 * g + 0] + pa.x, 0.f);
          y[4 * g + 1] = fmaxf(yp[4 * g + 1] + pa.y, 0.f);
          y[4 * g + 2] = fmaxf(yp[4 * g + 2] + pa.z, 0.f);
          y[4 * g + 3] = fmaxf(yp[4 * g + 3] + pa.w, 0.f);
        }
        if constexpr (!CONV2) {
          // mid row re = image row oy0 - 1 + re; pixels outside the image are conv2's zero padding
          const int my = sg.oy0 - 1 + re, mx = sg.ox0 - 1 + pix;
          const bool inimg = my >= 0 && my < a.H && mx >= 0 && mx < a.W;
          char* mid = smem + pl::PB::OFF_MID + (re % pl::PB::NMID) * pl::PB::MID_SLOT + pix * pl::PB::PIXB + ct * 64 + h * 8;
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            uint2 vh, vl;
            split2(y[4 * g + 0], y[4 * g + 1], vh.x, vl.x);
            split2(y[4 * g + 2], y[4 * g + 3], vh.y, vl.y);
            if (!inimg) { vh = uint2{0u, 0u}; vl = uint2{0u, 0u}; }
            *reinterpret_cast<uint2*>(mid + 16 * g) = vh;
            *reinterpret_cast<uint2*>(mid + pl::PB::MID_PLANE + 16 * g) = vl;
          }
        } else {
          const int oy = sg.oy0 + re, ox = sg.ox0 + pix;
          if (pix < pl::PB::TW && ox < a.W) {
            _Float16* o = a.out + (((size_t)sg.n * a.H + oy) * a.W + ox) * 64 + ct * 32 + 4 * h;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
              uint2 vh, vl;
              split2(y[4 * g + 0], y[4 * g + 1], vh.x, vl.x);
              split2(y[4 * g + 2], y[4 * g + 3], vh.y, vl.y);
              *reinterpret_cast<uint2*>(o + 8 * g) = vh;
              *reinterpret_cast<uint2*>(o + a.out_plane + 8 * g) = vl;
            }
          }
        }
      }
    }
    // ---- the contraction of row r0
    if (r0 >= 0 && r0 < nrows) {
      f32x16 am, ac;
      if constexpr (!B) {
        const float* bp = sbias + ct * 32 + 4 * h;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4 b4 = *reinterpret_cast<const float4*>(bp + 8 * g);
          am[4 * g + 0] = b4.x; am[4 * g + 1] = b4.y; am[4 * g + 2] = b4.z; am[4 * g + 3] = b4.w;
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) ac[r] = 0.f;
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) am[r] = ac[r] = 0.f;
      }
      int rb[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) rb[r] = ((r0 + r) % RING) * SLOT;
      auto xaddr = [&](int k) {
        const int r = k / 12, s = (k / 4) % 3, q = k % 4;
        return ring + rb[r] + s * pl::PB::PIXB + q * 32;
      };
      half8 xqh[PD + 1], xql[PD + 1];
#pragma unroll
      for (int k = 0; k < PD; ++k) {
        const char* p = xaddr(K0 + k);
        xqh[k] = *reinterpret_cast<const half8*>(p);
        xql[k] = *reinterpret_cast<const half8*>(p + PLANE);
      }
      static_for([&](auto kc) {
        constexpr int k = decltype(kc)::value;
        if constexpr (k + PD < KN) {
          const char* p = xaddr(K0 + k + PD);
          xqh[(k + PD) % (PD + 1)] = *reinterpret_cast<const half8*>(p);
          xql[(k + PD) % (PD + 1)] = *reinterpret_cast<const half8*>(p + PLANE);
        }
        PL_SB();
        am = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[k], xqh[k % (PD + 1)], am, 0, 0, 0);
        ac = __builtin_amdgcn_mfma_f32_32x32x16_f16(wh[k], xql[k % (PD + 1)], ac, 0, 0, 0);
        ac = __builtin_amdgcn_mfma_f32_32x32x16_f16(wl[k], xqh[k % (PD + 1)], ac, 0, 0, 0);
        PL_SB();
      }, std::make_integer_sequence<int, KN>{});
      if constexpr (CONV2 && !B) {
        // the residual as k_pl_c3p<true>'s two identity k-steps: x[oy, ox] = input row r0 + 2, input column pix + 2
        const char* ib = smem + pl::PB::OFF_IN + ((r0 + 2) % pl::PB::NIN) * pl::PB::IN_SLOT + (pix + 2) * pl::PB::PIXB + ct * 64 + h * 16;
#pragma unroll
        for (int qq = 0; qq < 2; ++qq) {
          const half8 rh = *reinterpret_cast<const half8*>(ib + qq * 32);
          const half8 rl = *reinterpret_cast<const half8*>(ib + pl::PB::IN_PLANE + qq * 32);
          const half8 idf = pb_identity_fragment(pix, h, qq);
          am = __builtin_amdgcn_mfma_f32_32x32x16_f16(idf, rh, am, 0, 0, 0);
          ac = __builtin_amdgcn_mfma_f32_32x32x16_f16(idf, rl, ac, 0, 0, 0);
        }
      }
      if constexpr (!B) {
        float* xw = xch + (j & 1) * (pl::PB::XCH / 2);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float4 v;
          v.x = comb(am[4 * g + 0], ac[4 * g + 0]);
          v.y = comb(am[4 * g + 1], ac[4 * g + 1]);
          v.z = comb(am[4 * g + 2], ac[4 * g + 2]);
          v.w = comb(am[4 * g + 3], ac[4 * g + 3]);
          *reinterpret_cast<float4*>(xw + g * 256) = v;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) yp[r] = comb(am[r], ac[r]);
      }
    }
    if (DMA) pb_issue_row(a, smem, sg, ct, j + pl::PB::LEAD, (j + pl::PB::LEAD) % pl::PB::NIN);     // (past the segment: zero rows)
  }
}

__global__ __launch_bounds__(512, 1) void k_pl_blk64(BlkArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (threadIdx.x < 128) {
    float* sb = reinterpret_cast<float*>(smem + pl::PB::OFF_BIAS);
    sb[threadIdx.x] = threadIdx.x < 64 ? a.b1[threadIdx.x] : a.b2[threadIdx.x - 64];
  }
  const int w = blockIdx.x;
  PSeg sg;
  {
    const int per_img = a.segs * a.strips;
    sg.n = w / per_img;
    const int r = w - sg.n * per_img;
    const int seg = r / a.strips, strip = r - seg * a.strips;
    sg.oy0 = seg * a.SH;
    sg.ox0 = strip * pl::PB::TW;
    sg.R = (a.H - sg.oy0) < a.SH ? (a.H - sg.oy0) : a.SH;
  }
  switch (wave) {
    case 0: case 1: pb_role<false, false>(a, smem, wave, sg); break;
    case 2: case 3: pb_role<false, true>(a, smem, wave - 2, sg); break;
    case 4: case 5: pb_role<true, true>(a, smem, wave - 4, sg); break;
    default: pb_role<true, false>(a, smem, wave - 6, sg); break;
  }
}

}  // namespace
}  // namespace pl

extern "C" LFD_API int lfd_pl_block64(int32_t n, int32_t h, int32_t w, const void* in, int64_t in_plane_halfs, void* out,
                                      int64_t out_plane_halfs, const void* w1_packed, const float* b1, const void* w2_packed,
                                      const float* b2, const void* zeros, lfd_stream_t stream) {
  if (!in || !out || !w1_packed || !b1 || !w2_packed || !b2 || !zeros) return LFD_ERR_INVALID_ARGUMENT;
  if (n < 1 || h < 1 || w < 1) return LFD_ERR_INVALID_ARGUMENT;
  if (!lfd_aligned16(in) || !lfd_aligned16(out) || !lfd_aligned16(w1_packed) || !lfd_aligned16(w2_packed))
    return LFD_ERR_INVALID_ARGUMENT;
  if ((long)(h) * w * 64 * 2 > 0x7fffffffL) return LFD_ERR_UNSUPPORTED;     // 32-bit row offsets inside an image
  const long plane = (long)n * h * w * 64;
  if (in_plane_halfs < plane || out_plane_halfs < plane || (in_plane_halfs & 7) || (out_plane_halfs & 7))
    return LFD_ERR_INVALID_ARGUMENT;
  // the identity is read from the input while the output is written: no overlap
  const char *ib = (const char*)in, *ob = (const char*)out;
  if (ib < ob + 2 * out_plane_halfs * 2 && ob < ib + 2 * in_plane_halfs * 2) return LFD_ERR_INVALID_ARGUMENT;
  pl::BlkArgs a{};
  a.in = (const _Float16*)in; a.in_plane = in_plane_halfs;
  a.out = (_Float16*)out; a.out_plane = out_plane_halfs;
  a.w1 = (const half8*)w1_packed; a.b1 = b1; a.w2 = (const half8*)w2_packed; a.b2 = b2;
  a.zeros = (const _Float16*)zeros;
  a.N = n; a.H = h; a.W = w;
  static unsigned long long attr_done_mask = 0;
  const int dev = lfd_device_ordinal();
  if (LFD_ONCE_PER_DEVICE(attr_done_mask, dev)) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&pl::k_pl_blk64), hipFuncAttributeMaxDynamicSharedMemorySize,
                            pl::PB::LDS_BYTES) != hipSuccess)
      return LFD_ERR_LAUNCH_FAILED;
    LFD_DONE_ON_DEVICE(attr_done_mask, dev);
  }
  // one work item (strip x segment) per workgroup, about one per CU: segments of >= 4 rows
  a.strips = (w + pl::PB::TW - 1) / pl::PB::TW;
  const long cols = (long)n * a.strips;
  int segs = (int)(256 / cols);
  if (segs < 1) segs = 1;
  int sh = (h + segs - 1) / segs;
  if (sh < 4) sh = 4;
  if (sh > h) sh = h;
  a.SH = sh;
  a.segs = (h + sh - 1) / sh;
  const long nwork = cols * a.segs;
  if (nwork > 0x7fffffffL) return LFD_ERR_UNSUPPORTED;
  a.nwork = (int)nwork;
  hipLaunchKernelGGL(pl::k_pl_blk64, dim3(a.nwork), dim3(512), pl::PB::LDS_BYTES, (hipStream_t)stream, a);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}
