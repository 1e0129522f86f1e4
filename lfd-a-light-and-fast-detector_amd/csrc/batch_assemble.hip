// csrc/batch_assemble.hip -- one launch builds a whole fp32 NCHW training batch from uint8 HWC source windows:
// cv2 INTER_LINEAR resize (8-bit fixed-point scalar path) + crop + horizontal flip + per-channel table normalisation +
// zero batch padding (include/lfd_hip.h, lfd_batch_assemble_f32; the host side is lfd_amd/data.py).
//
// A store-bound gather: the output is 4 B per pixel and channel, the source a few bytes per pixel.  A workgroup owns one
// image's band of BAND rows and a tile of up to TILE_W columns; the band's row table, the tile's column table (already
// flipped, clamped into the image's window and turned into byte offsets) and the lookup tables sit in LDS, and each lane
// writes 16-byte fp32 vectors along a plane row.  All arithmetic is integer; the weights come from the host.
#include "common.h"

namespace {

constexpr int BA_THREADS = 256;
constexpr int BA_TILE_W = 1024;   // columns per workgroup: 256 lanes x 4
constexpr int BA_BAND = 16;       // rows per workgroup

struct BaArgs {
  const uint8_t* src;
  const lfd_batch_desc_t* desc;
  const int4* coef;
  const float* lut;
  const int32_t* map;
  float* out;
  int n, c_src, c_out, h, w, tiles_x, bands;
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// V = 4: 16-byte stores (w_out % 4 == 0); V = 1: scalar stores
template <int COUT, int V>
__global__ __launch_bounds__(BA_THREADS) void k_batch_assemble(BaArgs a) {
  __shared__ int4 s_col[BA_TILE_W];        // {byte offset of tap 0, of tap 1, a0, a1}; x = -1: batch padding
  __shared__ long long s_roff[BA_BAND][2]; // byte offsets of the two source rows from the window's first pixel
  __shared__ int2 s_rw[BA_BAND];           // {b0, b1}; s_roff[.][0] = -1: batch padding
  __shared__ float s_lut[COUT * 256];

  int bid = blockIdx.x;
  const int tile = bid % a.tiles_x;
  bid /= a.tiles_x;
  const int band = bid % a.bands;
  const int img = bid / a.bands;
  const lfd_batch_desc_t d = a.desc[img];
  const int x0 = tile * BA_TILE_W, cols = min(BA_TILE_W, a.w - x0);
  const int y0 = band * BA_BAND, rows = min(BA_BAND, a.h - y0);
  const int vw = clampi(d.valid_w, 0, a.w), vh = clampi(d.valid_h, 0, a.h);
  const int ww = max(d.win_w, 1), wh = max(d.win_h, 1);
  const int4* tab = a.coef + (long long)img * (a.w + a.h);

  for (int j = threadIdx.x; j < cols; j += BA_THREADS) {
    const int x = x0 + j;
    int4 e = make_int4(-1, 0, 0, 0);
    if (x < vw) {
      const int4 c = tab[d.flip ? vw - 1 - x : x];
      e = make_int4(clampi(c.x - d.win_x0, 0, ww - 1) * a.c_src, clampi(c.y - d.win_x0, 0, ww - 1) * a.c_src, c.z, c.w);
    }
    s_col[j] = e;
  }
  if (threadIdx.x < rows) {
    const int y = y0 + threadIdx.x;
    long long o0 = -1, o1 = 0;
    int2 b = make_int2(0, 0);
    if (y < vh) {
      const int4 r = tab[a.w + y];
      o0 = (long long)clampi(r.x - d.win_y0, 0, wh - 1) * d.src_pitch;
      o1 = (long long)clampi(r.y - d.win_y0, 0, wh - 1) * d.src_pitch;
      b = make_int2(r.z, r.w);
    }
    s_roff[threadIdx.x][0] = o0;
    s_roff[threadIdx.x][1] = o1;
    s_rw[threadIdx.x] = b;
  }
  for (int j = threadIdx.x; j < COUT * 256; j += BA_THREADS) s_lut[j] = a.lut[j];
  int sc[COUT];
#pragma unroll
  for (int c = 0; c < COUT; ++c) sc[c] = clampi(a.map[c], 0, a.c_src - 1);
  __syncthreads();

  const uint8_t* win = a.src + d.src_offset;
  const int items = (cols + V - 1) / V;   // V = 4 only when cols % 4 == 0
  const long long plane = (long long)a.h * a.w;
  float* out_img = a.out + (long long)img * COUT * plane;
  for (int t = threadIdx.x; t < rows * items; t += BA_THREADS) {
    const int r = t / items, q = t - r * items;
    const long long ro0 = s_roff[r][0], ro1 = s_roff[r][1];
    const int2 bw = s_rw[r];
    float v[COUT][V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const int4 e = s_col[q * V + k];
      if (ro0 < 0 || e.x < 0) {
#pragma unroll
        for (int c = 0; c < COUT; ++c) v[c][k] = 0.0f;
        continue;
      }
      const uint8_t* p0 = win + ro0;
      const uint8_t* p1 = win + ro1;
#pragma unroll
      for (int c = 0; c < COUT; ++c) {
        const unsigned h0 = (unsigned)p0[e.x + sc[c]] * (unsigned)e.z + (unsigned)p0[e.y + sc[c]] * (unsigned)e.w;
        const unsigned h1 = (unsigned)p1[e.x + sc[c]] * (unsigned)e.z + (unsigned)p1[e.y + sc[c]] * (unsigned)e.w;
        const int acc = (int)(h0 * (unsigned)bw.x + h1 * (unsigned)bw.y + (1u << 21));
        v[c][k] = s_lut[c * 256 + clampi(acc >> 22, 0, 255)];
      }
    }
    float* o = out_img + (long long)(y0 + r) * a.w + x0 + q * V;
#pragma unroll
    for (int c = 0; c < COUT; ++c) {
      if constexpr (V == 4) {
        *reinterpret_cast<float4*>(o + c * plane) = make_float4(v[c][0], v[c][1], v[c][2], v[c][3]);
      } else {
        o[c * plane] = v[c][0];
      }
    }
  }
}

template <int COUT>
int launch_assemble(const BaArgs& a, long long blocks, hipStream_t st) {
  if (a.w % 4 == 0)
    hipLaunchKernelGGL((k_batch_assemble<COUT, 4>), dim3((unsigned)blocks), dim3(BA_THREADS), 0, st, a);
  else
    hipLaunchKernelGGL((k_batch_assemble<COUT, 1>), dim3((unsigned)blocks), dim3(BA_THREADS), 0, st, a);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

}  // namespace

extern "C" {

int lfd_batch_assemble_f32(const uint8_t* src, const lfd_batch_desc_t* desc, const int32_t* coef, const float* lut,
                           const int32_t* map, int32_t n, int32_t c_src, int32_t c_out, int32_t h_out, int32_t w_out,
                           float* out, lfd_stream_t stream) {
  if (!src || !desc || !coef || !lut || !map || !out) return LFD_ERR_INVALID_ARGUMENT;
  if ((reinterpret_cast<uintptr_t>(desc) & 7) || (reinterpret_cast<uintptr_t>(map) & 7)) return LFD_ERR_INVALID_ARGUMENT;
  if (!lfd_aligned16(coef) || !lfd_aligned16(lut) || !lfd_aligned16(out)) return LFD_ERR_INVALID_ARGUMENT;
  if ((c_src != 1 && c_src != 3) || (c_out != 1 && c_out != 3)) return LFD_ERR_INVALID_ARGUMENT;
  if (n < 1 || h_out < 1 || w_out < 1) return LFD_ERR_INVALID_ARGUMENT;
  if ((long long)n * c_out * h_out * w_out >= (1LL << 31)) return LFD_ERR_UNSUPPORTED;
  BaArgs a{};
  a.src = src; a.desc = desc; a.coef = reinterpret_cast<const int4*>(coef); a.lut = lut; a.map = map; a.out = out;
  a.n = n; a.c_src = c_src; a.c_out = c_out; a.h = h_out; a.w = w_out;
  a.tiles_x = (w_out + BA_TILE_W - 1) / BA_TILE_W;
  a.bands = (h_out + BA_BAND - 1) / BA_BAND;
  const long long blocks = (long long)n * a.bands * a.tiles_x;   // < 2^31: the output has fewer elements
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  return c_out == 3 ? launch_assemble<3>(a, blocks, st) : launch_assemble<1>(a, blocks, st);
}

}  // extern "C"
