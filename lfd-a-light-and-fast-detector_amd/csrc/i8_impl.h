// csrc/i8_impl.h -- what the INT8 deployment mode's kernels share: csrc/conv_i8.hip, block_i8.hip, entry_i8.hip and
// block128_i8.hip.  Every route through them is required to give the same bits, and the numeric contract that rests on stands
// here once.
//
// Lane map.  v_mfma_i32_32x32x32_i8 with A = filter (MFMA rows = output channels) and B = input pixels (MFMA columns = pixels);
// the i32 accumulation is exact (|acc| <= 9 * 128 * 127^2 < 2^31), so no summation order has to be fixed.
//   * a k-step is 32 input channels of one tap: lane (kh = lane >> 5, p = lane & 31) holds the 16 bytes "channels 32 q + 16 kh +
//     0..15" of filter row p (A) and of pixel p (B).  Both operands use the SAME (kh, byte) -> channel assignment, and the
//     instruction pairs byte j of lane half kh of A with byte j of lane half kh of B, so the sum covers each of the 32 channels
//     once whatever k index the hardware gives a (kh, j) slot; the exact tests (asymmetric full-range operands) check that pairing.
//   * C/D map (the f16 32x32 one): register g of lane (kh, p) is MFMA row (g & 3) + 8 (g >> 2) + 4 kh of pixel p.  The packed
//     filter (ops.pack_conv_weight_i8) puts output channel 32 slab + 16 kh + g on that row, so a lane ends with 16 consecutive
//     channels c0 = 32 slab + 16 kh .. c0 + 15 of its pixel: one 16-byte store of int8, two of fp16, four float4 loads of each
//     constant (load16f).
//   * an MFMA pixel tile is 2 rows of 16 pixels: p >> 4 is the row, p & 15 the column.
// Pixel pitch.  A pixel of CH channels is CH + 16 bytes in LDS (16 of bank spread), so a lane's k-fragment is one 16-byte LDS
// read; the halo travels memory -> registers -> LDS in 16-byte pieces of 16 channels, piece i = CH / 16 * pixel + chunk, pixels
// row by row over the halo tile (i8_halo_load / i8_halo_store).  Halo pixels outside the image are loads from a clamped address
// plus a select of 0.
// Tile walk.  Workgroups are persistent and walk t = (n * tiles_y + ty) * tiles_x + tx with stride gridDim.x (i8_tile_of,
// i8_tile_grid); the image base is a 64-bit scalar, offsets inside an image are 32-bit (h * w * 128 < 2^31 is checked by the
// entry points).  Ragged tiles are guarded on the store.
// Epilogue, fp32, evaluated as written:  v = fmaf(acc, mult[co], biasq[co]) (i8_affine);  with a residual
// v = fmaf(q_res, res_mult, v) (i8_residual);  with ReLU v = v > 0 ? v : 0 (i8_relu);  out_i8 = clamp(rint(v), -127, 127), round
// half even (i8_requant16, or i8_requant16_fast where a kernel says so).  A pyramid tap (i8_tap) is half(v * out_scale) of the
// un-requantised v evaluated in float64 and rounded once.
#pragma once
#include "common.h"

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));

union I8x16 { uint4 u; int8_t b[16]; };          // a lane's 16 channels of a pixel: int8,
union F16x16 { uint4 u[2]; _Float16 h[16]; };    // fp16

__device__ __forceinline__ void load16f(const float* src, float (&dst)[16]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float4 f = *reinterpret_cast<const float4*>(src + 4 * j);
    dst[4 * j + 0] = f.x; dst[4 * j + 1] = f.y; dst[4 * j + 2] = f.z; dst[4 * j + 3] = f.w;
  }
}

// ---------------------------------------------------------------------------------------------------------- requantisation
// clamp(rint(v), -127, 127) of 16 values -> 16 bytes: the reference expression (common.h)
__device__ __forceinline__ uint4 i8_requant16(const float (&vv)[16]) {
  I8x16 o;
#pragma unroll
  for (int g = 0; g < 16; ++g) o.b[g] = lfd_requant_i8(vv[g]);
  return o.u;
}

// The same value in three VALU instructions per element and three per packed dword instead of ten.  The clamp comes first (rint
// is monotone and the bounds are integers, so rint(clamp(v)) = clamp(rint(v))); c + 1.5 * 2^23 then lies in [2^23, 2^24), where
// fp32 has a spacing of 1, so the add's own round-to-nearest-even IS rint(c), and the sum's low mantissa byte is that integer in
// two's complement.  LO = 0 folds a preceding ReLU into the clamp (max(v, 0), -0 included, rounds to the same integer as v
// clamped at 0).  Finite v only: the epilogue constants and the fp16 map are finite.
template <int LO>
__device__ __forceinline__ uint32_t i8_q8bits(float v) {
  return __builtin_bit_cast(uint32_t, __builtin_amdgcn_fmed3f(v, (float)LO, 127.f) + 12582912.f);
}
__device__ __forceinline__ uint32_t i8_pack4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {    // the four low bytes
  const uint32_t lo = __builtin_amdgcn_perm(b, a, 0x0c0c0400u), hi = __builtin_amdgcn_perm(d, c, 0x0c0c0400u);
  return __builtin_amdgcn_perm(hi, lo, 0x05040100u);
}
template <int LO>
__device__ __forceinline__ uint4 i8_requant16_fast(const float (&vv)[16]) {
  uint32_t o[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
    o[j] = i8_pack4(i8_q8bits<LO>(vv[4 * j]), i8_q8bits<LO>(vv[4 * j + 1]), i8_q8bits<LO>(vv[4 * j + 2]), i8_q8bits<LO>(vv[4 * j + 3]));
  return make_uint4(o[0], o[1], o[2], o[3]);
}

// ---------------------------------------------------------------------------------------------------------------- epilogue
// One element of it, step by step; a kernel walks its 16 registers through the steps it needs, under its wave-uniform flags
// (csrc/conv_i8.hip) or unconditionally (the fused kernels).  The steps are functions of one element, not of sixteen, because the
// order the compiler meets the elements in decides its register allocation (a 16-wide tap function takes csrc/block_i8.hip from
// 232 registers to 256 and spills), and the kernels were tuned in different orders.
__device__ __forceinline__ float i8_affine(int acc, float mult, float biasq) { return __builtin_fmaf((float)acc, mult, biasq); }
__device__ __forceinline__ float i8_residual(float v, int8_t q_res, float res_mult) { return __builtin_fmaf((float)q_res, res_mult, v); }
__device__ __forceinline__ float i8_relu(float v) { return v > 0.f ? v : 0.f; }

// A pyramid tap: the un-requantised value for the fp16 head, half(v * out_scale).  Evaluated in float64 and rounded once: the fp32
// chain's first rounding (<= 2^-25 |acc mult + biasq|) survives a cancelling residual add and would exceed one fp16 ulp of a
// small result (measured: 1.25 ulp).
__device__ __forceinline__ _Float16 i8_tap(int acc, float mult, float biasq, bool has_res, int8_t q_res, float res_mult, bool relu,
                                           float out_scale) {
  double dv = __builtin_fma((double)acc, (double)mult, (double)biasq);
  if (has_res) dv = __builtin_fma((double)q_res, (double)res_mult, dv);
  if (relu) dv = dv > 0.0 ? dv : 0.0;
  return (_Float16)(float)(dv * (double)out_scale);
}

// -------------------------------------------------------------------------------------------------------- tile walk and halo
struct I8Tile { int tx, ty, n; };
__device__ __forceinline__ I8Tile i8_tile_of(int t, int tiles_x, int tiles_y) {
  const int tx = t % tiles_x;
  const int tq = t / tiles_x;
  return {tx, tq % tiles_y, tq / tiles_y};
}

// piece i = (pixel << I8_LG<CH>) + chunk: CH / 16 pieces per pixel, a power of two (shifts: i is not known to be >= 0 where a
// kernel hides the thread index from the compiler)
template <int CH> constexpr int I8_LG = CH == 64 ? 2 : 3;

// a 16-channel piece of a halo pixel on its way from memory to LDS: 16 bytes of int8, or (csrc/entry_i8.hip's fp16 input) 32 bytes
template <int ESZ = 1> struct I8Piece { uint4 u[ESZ]; };

// Pieces tid + NTHR * (it0 + 0 .. NIT - 1) of a halo tile of IW pixels per row and CH channels per pixel, PIECES pieces in all:
// halo pixel (iy, ix) is image pixel (y0 - PAD + iy, x0 - PAD + ix) of the H x W x CH int8 image at img.
// Unconditional loads from a clamped address + select.  THREE PLACES CARRY THEIR OWN COPY of this arithmetic and have to
// follow any change here: k_entry_i8 (csrc/entry_i8.hip: element size and runtime channel count; it must stay the parent's code),
// and in csrc/conv_i8.hip k_down_i8<64, 128> (the 64 -> 128 stage-entry pair's own kernel) and the 1x1 stride-2 instances of
// k_conv_i8 (a tile of every second pixel); the reasons stand with each.  (H and W are references to the kernel's argument struct, read inside the
// bounds chain: passed by value hipcc evaluates the chain in another order and three instances of k_conv_i8 take 2 .. 10 registers
// more.)
template <int CH, int IW, int PIECES, int PAD, int NTHR, int NIT>
__device__ __forceinline__ void i8_halo_load(I8Piece<> (&v)[NIT], const int8_t* img, int tid, int it0, int y0, int x0, const int& H,
                                             const int& W) {
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = tid + NTHR * (it0 + it);
    static_assert(CH == 64 || CH == 128, "I8_LG");
    const int pix = i >> I8_LG<CH>, ck = i & (CH / 16 - 1);
    const int iy = pix / IW, ix = pix - iy * IW;
    const int gy = y0 - PAD + iy, gx = x0 - PAD + ix;
    const bool ok = i < PIECES && gy >= 0 && gy < H && gx >= 0 && gx < W;
    v[it].u[0] = *reinterpret_cast<const uint4*>(img + (ok ? (gy * W + gx) * CH + ck * 16 : 0));    // < h * w * 128 < 2^31
    if (!ok) v[it].u[0] = make_uint4(0u, 0u, 0u, 0u);
  }
}

// LDS byte of piece i in its tile, and the pieces (int8 by now) into the tile at dst
template <int CH>
__device__ __forceinline__ int i8_halo_slot(int i) { return (i >> I8_LG<CH>) * (CH + 16) + (i & (CH / 16 - 1)) * 16; }
template <int CH, int PIECES, int NTHR, int NIT>
__device__ __forceinline__ void i8_halo_store(char* dst, const I8Piece<> (&v)[NIT], int tid, int it0) {
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int i = tid + NTHR * (it0 + it);
    if (i < PIECES) *reinterpret_cast<uint4*>(dst + i8_halo_slot<CH>(i)) = v[it].u[0];
  }
}

// tiles_x / tiles_y / ntiles of n maps of oh x ow cut into th x tw tiles, written into the kernel's argument struct; returns the
// persistent grid min(ntiles, cap), or 0 where ntiles + cap leaves int: the kernels' own loops add gridDim.x <= cap to t
template <class Args>
int i8_tile_grid(Args& a, int n, int oh, int ow, int th, int tw, int cap) {
  a.tiles_x = (ow + tw - 1) / tw;
  a.tiles_y = (oh + th - 1) / th;
  const long tiles = (long)a.tiles_x * a.tiles_y * n;
  if (tiles > 0x7fffffffL - cap) return 0;
  a.ntiles = (int)tiles;
  return a.ntiles < cap ? a.ntiles : cap;
}

// offset of output pixel (oy, ox) of image n in an [N,OH,OW,CH] tensor, of pixel (0, 0) where the tile is ragged there (!ook: the
// lane loads from it and does not store)
template <int CH>
__device__ __forceinline__ size_t i8_out_pixel(int n, int oy, int ox, int OH, int OW, bool& ook) {
  ook = oy < OH && ox < OW;
  return ((size_t)n * OH * OW + (size_t)((ook ? oy : 0) * OW + (ook ? ox : 0))) * CH;
}

// ------------------------------------------------------------------- one-launch residual blocks (block_i8.hip, block128_i8.hip)
// y = ReLU(conv2(ReLU(conv1(x))) + x), both convs 3x3 stride 1 pad 1, CH -> CH: the tensors and constants of two
// lfd_conv2d_nhwc_i8 calls
struct BlockI8Args {
  const int8_t* in;        // [N,H,W,CH]
  const i32x4* w1;         // packed [CH/32][9*CH/32][64 lanes]
  const float* mult1;      // [CH]
  const float* biasq1;
  const i32x4* w2;
  const float* mult2;
  const float* biasq2;
  int8_t* out_i8;          // [N,H,W,CH]
  _Float16* out_f16;       // [N,H,W,CH] or NULL
  float res_mult, out_scale;
  int N, H, W;
  int tiles_x, tiles_y, ntiles;
};

// the geometry both cut the same way: an 8 x 16 output tile, the mid tile (conv1's output with conv2's halo) and the input halo
template <int CH>
struct BlockI8Cfg {
  static constexpr int C = CH;
  static constexpr int TH = 8, TW = 16;                 // output tile
  static constexpr int MH = TH + 2, MW = TW + 2;        // mid tile
  static constexpr int MPIX = MH * MW;                  // 180
  static constexpr int IH = TH + 4, IW = TW + 4;        // input halo tile
  static constexpr int IPIX = IH * IW;                  // 240
  static constexpr int PITCH = CH + 16;                 // bytes per LDS pixel, input and mid
  static constexpr int IN_BYTES = IPIX * PITCH;
  static constexpr int MID_BYTES = MPIX * PITCH;
  static constexpr int PIECES = IPIX * (CH / 16);       // 16-byte pieces of the input halo
  static constexpr int NIT = (PIECES + 255) / 256;      // per thread of the 256 that load it
  static constexpr int NQ = CH / 32;                    // k-steps per tap
  static constexpr int NK = 9 * NQ;                     // k-steps of a 3x3xCH contraction
};

// conv1: mid pixel m, linear over MH x MW (clamped to the last where the MFMA tile runs past it: !mval, computed and not
// written).  Mid (mrow, mcol), tap (dy, dx) reads input tile (mrow + dy, mcol + dx): pbase = LDS byte of lane half kh's
// fragment of tap (0, 0), k-step 0.
template <class B>
__device__ __forceinline__ void i8_block_mid_pixel(int m, int kh, int& pbase, int& mrow, int& mcol, bool& mval) {
  mval = m < B::MPIX;
  const int mc = mval ? m : B::MPIX - 1;
  mrow = mc / B::MW;
  mcol = mc - mrow * B::MW;
  pbase = (mrow * B::IW + mcol) * B::PITCH + kh * 16;
}
// conv2: output pixel (ly, lx) of the tile reads mid (ly + dy, lx + dx): cbase as pbase above; opix = the lane's 16 channels
// c0.. of that pixel in the output (and, being the same shape, the input) tensor
template <class B>
__device__ __forceinline__ void i8_block_out_pixel(const BlockI8Args& a, const I8Tile& tl, int ly, int lx, int kh, int c0, int& cbase,
                                                   size_t& opix, bool& ook) {
  cbase = (ly * B::MW + lx) * B::PITCH + kh * 16;
  opix = i8_out_pixel<B::C>(tl.n, tl.ty * B::TH + ly, tl.tx * B::TW + lx, a.H, a.W, ook) + c0;
}

// validation and tile set-up of both entry points; LFD_OK, or the status to return.  blocks: the persistent grid (<= cap)
template <class B>
int i8_block_args(BlockI8Args& a, int& blocks, int cap, int32_t n, int32_t h, int32_t w, const void* in, const void* w1_packed,
                  const float* mult1, const float* biasq1, const void* w2_packed, const float* mult2, const float* biasq2,
                  float res_mult, void* out_i8, void* out_f16, float out_scale) {
  if (!in || !w1_packed || !mult1 || !biasq1 || !w2_packed || !mult2 || !biasq2 || !out_i8) return LFD_ERR_INVALID_ARGUMENT;
  if (n < 1 || h < 1 || w < 1) return LFD_ERR_INVALID_ARGUMENT;
  if (!lfd_aligned16(in) || !lfd_aligned16(w1_packed) || !lfd_aligned16(mult1) || !lfd_aligned16(biasq1) ||
      !lfd_aligned16(w2_packed) || !lfd_aligned16(mult2) || !lfd_aligned16(biasq2) || !lfd_aligned16(out_i8) ||
      !lfd_aligned16(out_f16))
    return LFD_ERR_INVALID_ARGUMENT;
  if (in == out_i8) return LFD_ERR_INVALID_ARGUMENT;
  if ((long)h * w * 128 > 0x7fffffffL) return LFD_ERR_UNSUPPORTED;           // 32-bit offsets inside an image
  a.in = (const int8_t*)in; a.w1 = (const i32x4*)w1_packed; a.mult1 = mult1; a.biasq1 = biasq1;
  a.w2 = (const i32x4*)w2_packed; a.mult2 = mult2; a.biasq2 = biasq2;
  a.out_i8 = (int8_t*)out_i8; a.out_f16 = (_Float16*)out_f16; a.res_mult = res_mult; a.out_scale = out_scale;
  a.N = n; a.H = h; a.W = w;
  blocks = i8_tile_grid(a, n, h, w, B::TH, B::TW, cap);
  return blocks ? LFD_OK : LFD_ERR_UNSUPPORTED;
}

}  // namespace
