// csrc/conv_wide.hip -- NHWC fp16 implicit-GEMM conv (1x1 / 3x3, stride 1 / 2, pad ks/2) for the WIDE layers of LFDResNet's
// own body presets: 'fast' ends in 256 and 512 channels, 'faster' in 256 (lfd_resnet.py:222-231), i.e. every conv whose
// cin or cout is above 128; fused bias (+ residual) + ReLU like csrc/conv_impl.h.  v_mfma_f32_32x32x16_f16, fp32 accumulation.
//
// These layers sit at stride 16-64 of the frame: M is small (8 x 17 x 30 = 4080 pixels at 512 channels for a batch of eight
// 1080p frames) and the filter is large (512 -> 512 3x3: 4.7 MB), so nothing is register-stationary here.  The work is cut
// the way csrc/conv_small.hip cuts the 128 -> 128 layers, generalised over the channel counts:
//   * a workgroup owns 64 output pixels (4 rows x 16 columns = two 32-pixel MFMA tiles) and ONE 32-channel slab of the
//     output (grid.y = cout / 32): at 4080 pixels x 512 channels that is 80 x 16 = 1280 workgroups, 160 for a single frame;
//   * the input halo tile goes through LDS in chunks of 64 channels (6 x 18 pixels at stride 1, 9 x 33 at stride 2; a 1x1
//     conv only fetches the 4 x 16 pixels it reads), one buffer: chunk c + 1 travels from memory into registers while chunk
//     c is contracted, and so do the filter fragments of chunk c + 1;
//   * SPLIT-K over the four waves, always: wave w contracts channels 16 w .. 16 w + 15 of every chunk, all taps -- k-step
//     tap * (cin / 16) + 4 c + w of the packed order [cout / 32][ks * ks * cin / 16][64 lanes][8] (ops.pack_conv_weight), one
//     contiguous 1 KB fragment per tap, used for both pixel tiles;
//   * the four partial accumulators meet in LDS and are added in the FIXED order ((w0 + w1) + w2) + w3: no atomics, no
//     workspace, the same bits on every run; wave w finishes a quarter of the outputs: bias (+ residual) -> ReLU -> fp16;
//   * workgroups walk the pixel tiles with stride gridDim.x (at most 1024 workgroups per launch).
// conv_dispatch also sends the four <= 128 layers of FastBlock / FastestBlock bodies here that conv_impl.h has no instance for;
// two of them read 32 channels: one half-filled chunk, waves 2 and 3 add zeros.
// Not here: the chained 1x1 and the downsample-pair forms of conv_impl.h (the engine launches those layers one by one), and
// training (train_engine.supported stays false above 128 channels).
// Measured: ahead of torch's conv on every layer of the presets but the two 3x3 stride-2 ones at batch eight, whose
// 9 x 33 halo is staged once per output slab; storing even and odd halo columns apart (no two-way bank sharing of the
// stride-2 reads) did not change their time and is not done.
#include "common.h"

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct WideArgs {
  const _Float16* in;   // [N,H,W,cin]
  _Float16* out;        // [N,OH,OW,cout]
  const half8* w;       // packed [cout/32][ks*ks*cin/16][64 lanes]
  const float* bias;    // [cout]
  const _Float16* res;  // [N,OH,OW,cout] or null
  int N, H, W, OH, OW, cin, cout, relu;
  int tiles_x, tiles_y, ntiles;
};

template <int KS, int S>
struct WCfg {
  static constexpr int TH = 4, TW = 16;                 // output tile: MFMA tile pt = rows 2 pt, 2 pt + 1
  static constexpr int LS = KS == 1 ? 1 : S;            // LDS pixels between neighbouring outputs
  static constexpr int GS = KS == 1 ? S : 1;            // image pixels between neighbouring LDS pixels (a 1x1 fetches only what it reads)
  static constexpr int PAD = KS / 2;
  static constexpr int IH = (TH - 1) * LS + KS, IW = (TW - 1) * LS + KS;
  static constexpr int NPIX = IH * IW;
  static constexpr int PITCH = 144;                     // bytes per LDS pixel: 64 channels x 2 B + 16 B (bank spread)
  static constexpr int NIT = (NPIX * 8 + 255) / 256;    // 16-byte loads per thread and chunk
  static constexpr int NT = KS * KS;
  static constexpr int IN_BYTES = NPIX * PITCH;
  static constexpr int PART_BYTES = 4 * 2 * 16 * 64 * 4;  // [wave][pt][register][lane] fp32, in the storage of the consumed input tile
  static constexpr int LDS_BYTES = IN_BYTES > PART_BYTES ? IN_BYTES : PART_BYTES;
  static_assert(LDS_BYTES <= 64 * 1024, "static LDS");
};

template <int KS, int S>
__global__ __launch_bounds__(256) void k_conv_wide(const WideArgs a) {
  using C = WCfg<KS, S>;
  __shared__ __attribute__((aligned(16))) char smem[C::LDS_BYTES];
  float* part = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x, lane = tid & 63, p = lane & 31, kh = lane >> 5;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int slab = blockIdx.y;
  const int nq = a.cin >> 4, nchunk = (a.cin + 63) >> 6;   // cin = 32: one half-filled chunk, waves 2 and 3 contribute zeros
  const half8* wslab = a.w + (size_t)slab * C::NT * nq * 64 + lane;
  // pixel of lane p in MFMA tile pt: row 2 pt + (p >> 4), column p & 15; this wave's 16 channels of the chunk, k half kh
  const int lbase = (((p >> 4) * C::LS) * C::IW + (p & 15) * C::LS) * C::PITCH + wv * 32 + kh * 16;
  const int ept = wv >> 1, ehf = wv & 1;                // epilogue: this wave finishes tile ept, registers 8 ehf .. 8 ehf + 7

  for (int t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
    const int tx = t % a.tiles_x;
    const int tq = t / a.tiles_x;
    const int ty = tq % a.tiles_y, n = tq / a.tiles_y;

    // ---- where this thread's 16-byte pieces of a halo chunk come from (halfs from a.in, without the chunk's channel
    //      offset; -1: outside the image = the conv's zero padding, or past the tile) -- the same for every chunk
    long goff[C::NIT];
#pragma unroll
    for (int it = 0; it < C::NIT; ++it) {
      const int i = tid + 256 * it;
      const int pix = i >> 3, ck = i & 7;
      const int iy = pix / C::IW, ix = pix - iy * C::IW;
      const int gy = (ty * C::TH * C::LS - C::PAD + iy) * C::GS, gx = (tx * C::TW * C::LS - C::PAD + ix) * C::GS;
      const bool ok = pix < C::NPIX && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W && ck * 8 < a.cin;
      goff[it] = ok ? (((long)n * a.H + gy) * a.W + gx) * a.cin + ck * 8 : -1L;
    }
    auto load_chunk = [&](int c, uint4 (&v)[C::NIT]) {
#pragma unroll
      for (int it = 0; it < C::NIT; ++it) {
        // unconditional load + select (a conditional load is a branch); the stand-in address is the tensor's first pixel
        v[it] = *reinterpret_cast<const uint4*>(a.in + (goff[it] < 0 ? 0L : goff[it]) + c * 64);
        if (goff[it] < 0) v[it] = make_uint4(0u, 0u, 0u, 0u);
      }
    };
    auto load_filter = [&](int c, half8 (&f)[C::NT]) {
#pragma unroll
      for (int tp = 0; tp < C::NT; ++tp) f[tp] = wslab[(size_t)(tp * nq + (c * 4 + wv < nq ? c * 4 + wv : nq - 1)) * 64];
    };

    uint4 v[C::NIT];
    half8 wnext[C::NT];
    load_filter(0, wnext);
    load_chunk(0, v);

    f32x16 acc[2];
#pragma unroll
    for (int pt = 0; pt < 2; ++pt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[pt][r] = 0.f;

#pragma unroll 1
    for (int c = 0; c < nchunk; ++c) {
      __syncthreads();          // every wave is done with the previous chunk (or with the previous tile's partial sums)
#pragma unroll
      for (int it = 0; it < C::NIT; ++it) {
        const int i = tid + 256 * it;
        if (i < C::NPIX * 8) *reinterpret_cast<uint4*>(smem + (i >> 3) * C::PITCH + (i & 7) * 16) = v[it];
      }
      half8 wf[C::NT];
#pragma unroll
      for (int tp = 0; tp < C::NT; ++tp) wf[tp] = wnext[tp];
      __syncthreads();
      if (c + 1 < nchunk) {     // the next chunk travels while this one is contracted
        load_filter(c + 1, wnext);
        load_chunk(c + 1, v);
      }
      if (c * 4 + wv >= nq) continue;   // (wave-uniform; only waves 2, 3 of a 32-channel input: no barrier is skipped)
#pragma unroll
      for (int tp = 0; tp < C::NT; ++tp) {
        const int dy = tp / KS, dx = tp - dy * KS;
        const int koff = (dy * C::IW + dx) * C::PITCH;
#pragma unroll
        for (int pt = 0; pt < 2; ++pt) {
          const half8 b = *reinterpret_cast<const half8*>(smem + lbase + pt * 2 * C::LS * C::IW * C::PITCH + koff);
          acc[pt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wf[tp], b, acc[pt], 0, 0, 0);
        }
      }
    }

    // ---- what the epilogue needs from memory, requested before the reduction
    const int oy = ty * C::TH + ept * 2 + (p >> 4), ox = tx * C::TW + (p & 15);
    const bool ook = oy < a.OH && ox < a.OW;
    const size_t opix = (((size_t)n * a.OH + (ook ? oy : 0)) * a.OW + (ook ? ox : 0)) * a.cout;
    float4 bv[2];
    half4 rv[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c0 = slab * 32 + 8 * (2 * ehf + j) + 4 * kh;
      bv[j] = *reinterpret_cast<const float4*>(a.bias + c0);
      rv[j] = a.res ? *reinterpret_cast<const half4*>(a.res + opix + c0) : half4{0, 0, 0, 0};
    }

    // ---- partial sums -> LDS [wave][pt][register][lane], over the consumed input tile
    __syncthreads();
#pragma unroll
    for (int pt = 0; pt < 2; ++pt)
#pragma unroll
      for (int r = 0; r < 16; ++r) part[((wv * 2 + pt) * 16 + r) * 64 + lane] = acc[pt][r];
    __syncthreads();

    // ---- fixed-order sum over the four K quarters; register 4 (2 ehf + j) + e of lane (kh, p) = channel c0 + e
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int c0 = slab * 32 + 8 * (2 * ehf + j) + 4 * kh;
      const float bb[4] = {bv[j].x, bv[j].y, bv[j].z, bv[j].w};
      float o4[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 8 * ehf + 4 * j + e;
        const float s01 = part[((0 * 2 + ept) * 16 + r) * 64 + lane] + part[((1 * 2 + ept) * 16 + r) * 64 + lane];
        const float s012 = s01 + part[((2 * 2 + ept) * 16 + r) * 64 + lane];
        o4[e] = (s012 + part[((3 * 2 + ept) * 16 + r) * 64 + lane]) + bb[e];
        o4[e] += (float)rv[j][e];
      }
      const uint32_t lo2 = a.relu ? LFD_PK_RELU : LFD_PK_NONE;
      uint2 o;
      o.x = lfd_cvt_pk_max(o4[0], o4[1], lo2);
      o.y = lfd_cvt_pk_max(o4[2], o4[3], lo2);
      if (ook) *reinterpret_cast<uint2*>(a.out + opix + c0) = o;
    }
  }
}

template <int KS, int S>
int launch_wide(const WideArgs& a, hipStream_t st) {
  const int slabs = a.cout / 32;
  int blocks = 1024 / slabs;
  if (blocks > a.ntiles) blocks = a.ntiles;
  hipLaunchKernelGGL((k_conv_wide<KS, S>), dim3((unsigned)blocks, (unsigned)slabs), dim3(256), 0, st, a);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

}  // namespace

// The shapes this file takes: channel counts that are multiples of 64 (or 32 itself) on the input side and multiples of 32 on
// the output side, up to 512.  conv_dispatch (conv.hip) routes here what has cin or cout above 128, and the four <= 128 layers
// of FastBlock / FastestBlock bodies that have no instance of conv_impl.h.
int lfd_conv_wide_supported(int cin, int cout, int ks, int stride, int has_res) {
  if ((ks != 1 && ks != 3) || (stride != 1 && stride != 2)) return LFD_ERR_UNSUPPORTED;
  if ((cin != 32 && (cin < 64 || cin > 512 || cin % 64)) || cout < 32 || cout > 512 || cout % 32) return LFD_ERR_UNSUPPORTED;
  if (has_res && stride != 1) return LFD_ERR_UNSUPPORTED;
  return LFD_OK;
}

int lfd_conv_wide_launch(const _Float16* in, _Float16* out, const void* w_packed, const float* bias, const _Float16* res,
                         int n, int h, int w, int cin, int cout, int ks, int stride, int relu, hipStream_t st) {
  const int rc = lfd_conv_wide_supported(cin, cout, ks, stride, res != nullptr);
  if (rc != LFD_OK) return rc;
  WideArgs a{};
  a.in = in; a.out = out; a.w = (const half8*)w_packed; a.bias = bias; a.res = res;
  a.N = n; a.H = h; a.W = w; a.cin = cin; a.cout = cout; a.relu = relu;
  const int pad = ks / 2;
  a.OH = (h + 2 * pad - ks) / stride + 1;
  a.OW = (w + 2 * pad - ks) / stride + 1;
  a.tiles_x = (a.OW + 15) / 16;
  a.tiles_y = (a.OH + 3) / 4;
  const long tiles = (long)a.tiles_x * a.tiles_y * n;
  if (tiles < 1 || tiles > 0x7fffffffL) return LFD_ERR_UNSUPPORTED;
  a.ntiles = (int)tiles;
  if (ks == 3) return stride == 1 ? launch_wide<3, 1>(a, st) : launch_wide<3, 2>(a, st);
  return stride == 1 ? launch_wide<1, 1>(a, st) : launch_wide<1, 2>(a, st);
}
