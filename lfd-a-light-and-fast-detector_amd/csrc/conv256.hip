// csrc/conv256.hip -- NHWC fp16 conv, 3x3 (or 1x1) stride 1 pad ks/2, 256 input channels, 32 .. 256 output channels, for the
// LARGE maps of a 256-channel FPN neck and FCOSHead / LFDHead towers (lfd/model/neck/fpn.py:57-82 output convs,
// lfd/model/head/fcos_head.py:60-110 towers and output convs; cuDNN in the reference).  v_mfma_f32_32x32x16_f16, fp32
// accumulation, fused bias (+ ReLU), fp16 output or the un-rounded fp32 accumulators (the heads' logits).
//
// csrc/conv_wide.hip is cut for a few thousand pixels under a large filter: 64 pixels x 32 channels per workgroup, the halo
// staged once per output slab.  Here M is large (8 x 135 x 240 pixels on the first FCOS level of eight 1080p frames) and the cut
// is the opposite one:
//   * a workgroup owns 128 output pixels (8 rows x 16 columns = four 32-pixel MFMA tiles of 2 rows) and ALL output channels, so
//     the 10 x 18 halo is staged once: through LDS in four chunks of 64 channels (26 KB, one buffer; chunk c + 1 travels from
//     memory into registers while chunk c is contracted);
//   * no split-K: a wave owns whole accumulators.  With CG channel groups (4 for cout > 128, 2 for cout > 64, else 1) wave w is
//     channel group w % CG (two 32-channel slabs) and pixel group w / CG (CG of the four MFMA tiles): 2 x CG accumulators of
//     16 registers.  Each 16-byte LDS read of the input feeds two MFMAs;
//   * the filter never enters LDS: a wave's fragments are its own (packed order [cout / 32][ks * ks * 16][64 lanes][8] of
//     ops.pack_conv_weight, k-step tap * 16 + 4 c + q), 8 KB per (tap, chunk), fetched one tap ahead into the other half of a
//     register double buffer.  128 pixels amortise the 1.18 MB filter of a 256 -> 256 layer: 151 MFLOP per 1.18 MB + 104 KB;
//   * one fixed summation order per output (chunk, tap, k-step ascending): no atomics, no workspace, the same bits every run;
//   * workgroups walk (image, tile) with stride gridDim.x (at most 512 workgroups); ragged tiles are guarded on the store,
//     halo pixels outside the image are unconditional loads from a clamped address plus a select;
//   * a slab past cout (cout = 32, 96, 160, 224: the second slab of the last channel group) is computed on a clamped filter
//     address and not stored; a wave whose channel group is past cout altogether only helps staging.
// Addressing: the image base is a 64-bit scalar, offsets inside an image are 32-bit (h * w * 256 < 2^31 is checked).
#include "common.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int C256_CIN = 256;
constexpr int C256_MAX_WORKGROUPS = 512;

struct C256Args {
  const _Float16* in;   // [N,H,W,256]
  void* out;            // [N,H,W,cout] fp16 or fp32
  const half8* w;       // packed [cout/32][ks*ks*16][64 lanes]
  const float* bias;    // [cout]
  int N, H, W, cout, relu;
  int tiles_x, tiles_y, ntiles;
};

template <int KS>
struct C256Cfg {
  static constexpr int TH = 8, TW = 16;                 // output tile: MFMA tile pt = rows 2 pt, 2 pt + 1
  static constexpr int PAD = KS / 2;
  static constexpr int IH = TH + KS - 1, IW = TW + KS - 1;
  static constexpr int NPIX = IH * IW;
  static constexpr int PITCH = 144;                     // bytes per LDS pixel: 64 channels x 2 B + 16 B (bank spread)
  static constexpr int NIT = (NPIX * 8 + 255) / 256;    // 16-byte loads per thread and chunk
  static constexpr int NT = KS * KS;
  static constexpr int NQ = C256_CIN / 16;              // k-steps per tap
  static constexpr int NCHUNK = C256_CIN / 64;
  static constexpr int LDS_BYTES = NPIX * PITCH;
  static_assert(LDS_BYTES <= 64 * 1024, "static LDS");
  static_assert(NCHUNK % 2 == 0, "the chunk loop is unrolled by two (register double buffer of the filter)");
};

template <int KS, int CG, bool F32>
__global__ __launch_bounds__(256) void k_conv256(const C256Args a) {
  using C = C256Cfg<KS>;
  constexpr int NPT = CG;                               // MFMA pixel tiles per wave (4 tiles / (4 / CG) pixel groups)
  __shared__ __attribute__((aligned(16))) char smem[C::LDS_BYTES];
  const int tid = threadIdx.x, lane = tid & 63, p = lane & 31, kh = lane >> 5;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cg = wv % CG, pg = wv / CG;
  const int nslabs = a.cout >> 5;
  const int s0 = cg * 2;
  const int nsl = nslabs - s0 < 0 ? 0 : (nslabs - s0 > 2 ? 2 : nslabs - s0);   // this wave's slabs inside cout
  const half8* wslab[2];
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const int sl = s0 + s < nslabs ? s0 + s : nslabs - 1;                      // clamped: computed, never stored
    wslab[s] = a.w + (size_t)sl * C::NT * C::NQ * 64 + lane;
  }
  // pixel of lane p in this wave's MFMA tile t: row 2 (pg NPT + t) + (p >> 4), column p & 15; k half kh of a k-step
  const int lbase = ((2 * pg * NPT + (p >> 4)) * C::IW + (p & 15)) * C::PITCH + kh * 16;

  for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const int tx = t % a.tiles_x;
    const int tq = t / a.tiles_x;
    const int ty = tq % a.tiles_y, n = tq / a.tiles_y;
    const _Float16* in_img = a.in + (size_t)n * a.H * a.W * C256_CIN;

    // ---- where this thread's 16-byte pieces of a halo chunk come from (halfs from in_img, without the chunk's channel
    //      offset; -1: outside the image = the conv's zero padding, or past the tile) -- the same for every chunk
    int goff[C::NIT];
#pragma unroll
    for (int it = 0; it < C::NIT; ++it) {
      const int i = tid + 256 * it;
      const int pix = i >> 3, ck = i & 7;
      const int iy = pix / C::IW, ix = pix - iy * C::IW;
      const int gy = ty * C::TH - C::PAD + iy, gx = tx * C::TW - C::PAD + ix;
      const bool ok = pix < C::NPIX && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W;
      goff[it] = ok ? (gy * a.W + gx) * C256_CIN + ck * 8 : -1;
    }
    auto load_chunk = [&](int c, uint4 (&v)[C::NIT]) {
#pragma unroll
      for (int it = 0; it < C::NIT; ++it) {
        // unconditional load + select (a conditional load is a branch); the stand-in address is the image's first pixel
        v[it] = *reinterpret_cast<const uint4*>(in_img + (goff[it] < 0 ? 0 : goff[it]) + c * 64);
        if (goff[it] < 0) v[it] = make_uint4(0u, 0u, 0u, 0u);
      }
    };
    auto load_filter = [&](int c, int tp, half8 (&f)[8]) {
#pragma unroll
      for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int q = 0; q < 4; ++q) f[s * 4 + q] = wslab[s][(size_t)(tp * C::NQ + c * 4 + q) * 64];
    };

    uint4 v[C::NIT];
    half8 wf[2][8];
    load_filter(0, 0, wf[0]);
    load_chunk(0, v);

    f32x16 acc[2][NPT];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int pt = 0; pt < NPT; ++pt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[s][pt][r] = 0.f;

#pragma unroll 1
    for (int c2 = 0; c2 < C::NCHUNK; c2 += 2) {
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const int c = c2 + hf;
        __syncthreads();          // every wave is done with the previous chunk (or with the previous tile)
#pragma unroll
        for (int it = 0; it < C::NIT; ++it) {
          const int i = tid + 256 * it;
          if (i < C::NPIX * 8) *reinterpret_cast<uint4*>(smem + (i >> 3) * C::PITCH + (i & 7) * 16) = v[it];
        }
        __syncthreads();
        if (c + 1 < C::NCHUNK) load_chunk(c + 1, v);     // the next chunk travels while this one is contracted
#pragma unroll
        for (int tp = 0; tp < C::NT; ++tp) {
          const int cur = (hf * C::NT + tp) & 1;         // (2 NT steps per trip of the c2 loop: the parity restarts at 0)
          if (tp + 1 < C::NT) load_filter(c, tp + 1, wf[cur ^ 1]);
          else if (c + 1 < C::NCHUNK) load_filter(c + 1, 0, wf[cur ^ 1]);
          if (nsl > 0) {          // (wave-uniform, no barrier inside)
            const int dy = tp / KS, dx = tp - dy * KS;
            const int koff = (dy * C::IW + dx) * C::PITCH;
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
              for (int pt = 0; pt < NPT; ++pt) {
                const half8 b = *reinterpret_cast<const half8*>(smem + lbase + pt * 2 * C::IW * C::PITCH + koff + q * 32);
#pragma unroll
                for (int s = 0; s < 2; ++s)
                  acc[s][pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[cur][s * 4 + q], b, acc[s][pt], 0, 0, 0);
              }
          }
        }
      }
    }

    // ---- epilogue: register 4 j + e of lane (kh, p) = channel 32 slab + 8 j + 4 kh + e of pixel p; bias -> ReLU -> store
    const size_t out_img = (size_t)n * a.H * a.W * a.cout;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      if (s >= nsl) continue;
#pragma unroll
      for (int pt = 0; pt < NPT; ++pt) {
        const int oy = ty * C::TH + 2 * (pg * NPT + pt) + (p >> 4), ox = tx * C::TW + (p & 15);
        const bool ook = oy < a.H && ox < a.W;
        const size_t opix = out_img + (size_t)((ook ? oy : 0) * a.W + (ook ? ox : 0)) * a.cout;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c0 = (s0 + s) * 32 + 8 * j + 4 * kh;
          const float4 bv = *reinterpret_cast<const float4*>(a.bias + c0);
          float o4[4] = {acc[s][pt][4 * j] + bv.x, acc[s][pt][4 * j + 1] + bv.y, acc[s][pt][4 * j + 2] + bv.z,
                         acc[s][pt][4 * j + 3] + bv.w};
          if (F32) {
            if (a.relu) {
#pragma unroll
              for (int e = 0; e < 4; ++e) o4[e] = o4[e] > 0.f ? o4[e] : 0.f;
            }
            if (ook) *reinterpret_cast<float4*>(static_cast<float*>(a.out) + opix + c0) = make_float4(o4[0], o4[1], o4[2], o4[3]);
          } else {
            const uint32_t lo2 = a.relu ? LFD_PK_RELU : LFD_PK_NONE;
            uint2 o;
            o.x = lfd_cvt_pk_max(o4[0], o4[1], lo2);
            o.y = lfd_cvt_pk_max(o4[2], o4[3], lo2);
            if (ook) *reinterpret_cast<uint2*>(static_cast<_Float16*>(a.out) + opix + c0) = o;
          }
        }
      }
    }
  }
}

template <int KS, int CG, bool F32>
int launch256(const C256Args& a, hipStream_t st) {
  const int blocks = a.ntiles < C256_MAX_WORKGROUPS ? a.ntiles : C256_MAX_WORKGROUPS;
  hipLaunchKernelGGL((k_conv256<KS, CG, F32>), dim3((unsigned)blocks), dim3(256), 0, st, a);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

template <int KS, bool F32>
int launch256_cg(const C256Args& a, hipStream_t st) {
  if (a.cout > 128) return launch256<KS, 4, F32>(a, st);
  if (a.cout > 64) return launch256<KS, 2, F32>(a, st);
  return launch256<KS, 1, F32>(a, st);
}

}  // namespace

extern "C" int lfd_conv256_nhwc_f16_supported(int32_t cin, int32_t cout, int32_t ks, int32_t out_f32) {
  if (cin != C256_CIN || cout < 32 || cout > 256 || cout % 32) return LFD_ERR_UNSUPPORTED;
  if (ks != 3 && !(ks == 1 && out_f32)) return LFD_ERR_UNSUPPORTED;     // the 1x1 instance exists for fp32 logits only
  return LFD_OK;
}

extern "C" int lfd_conv256_nhwc_f16(const void* in, void* out, const void* w_packed, const float* bias, int32_t n, int32_t h,
                                    int32_t w, int32_t cout, int32_t ks, int32_t relu, int32_t out_f32, lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!in || !out || !w_packed || !bias) return LFD_ERR_INVALID_ARGUMENT;
  if (n < 1 || h < 1 || w < 1) return LFD_ERR_INVALID_ARGUMENT;
  if (!lfd_aligned16(in) || !lfd_aligned16(out) || !lfd_aligned16(w_packed) || !lfd_aligned16(bias)) return LFD_ERR_INVALID_ARGUMENT;
  const int rc = lfd_conv256_nhwc_f16_supported(C256_CIN, cout, ks, out_f32);
  if (rc != LFD_OK) return rc;
  if ((long)h * w * C256_CIN > 0x7fffffffL) return LFD_ERR_UNSUPPORTED;     // 32-bit offsets inside an image
  C256Args a{};
  a.in = (const _Float16*)in; a.out = out; a.w = (const half8*)w_packed; a.bias = bias;
  a.N = n; a.H = h; a.W = w; a.cout = cout; a.relu = relu ? 1 : 0;
  a.tiles_x = (w + 15) / 16;
  a.tiles_y = (h + 7) / 8;
  const long tiles = (long)a.tiles_x * a.tiles_y * n;
  if (tiles > 0x7fffffffL) return LFD_ERR_UNSUPPORTED;
  a.ntiles = (int)tiles;
  if (ks == 1) return launch256_cg<1, true>(a, st);
  return out_f32 ? launch256_cg<3, true>(a, st) : launch256_cg<3, false>(a, st);
}
