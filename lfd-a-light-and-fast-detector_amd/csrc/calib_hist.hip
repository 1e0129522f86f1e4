// csrc/calib_hist.hip -- the INT8 calibration's magnitude histogram: hist[bits & 0x7fff] += 1 for every element of
// an fp16 NHWC map that lies in a real channel.  An fp16 magnitude has 15 bits, so the 32768 bins count the values themselves:
// no range in advance, batches add without rebinning, and every threshold rule (lfd_amd/calibration.py) is evaluated from the
// counts exactly.  Stands where the reference hands its calibration batches to TensorRT's IInt8EntropyCalibrator2
// (lfd/deployment/tensorrt/build_engine.py:22), which keeps its histograms to itself.
//
//   * a workgroup (1024 threads, one per CU: 128 KiB of the CU's 160 KiB LDS) keeps a private u32[32768] histogram in LDS and
//     walks chunks of LFD_CALIB_HIST_CHUNK_VECS 16-byte vectors with stride gridDim.x (at most LFD_CALIB_HIST_MAX_WORKGROUPS);
//     a thread has its 4 loads of a chunk in flight before it counts the first.
//   * a non-zero magnitude is one LDS atomic add that returns nothing (ds_add_u32).  The addresses are the data, so bank
//     conflicts are whatever the data makes them; equal addresses inside one instruction serialise.
//   * zeros (+0 and -0: about half of a post-ReLU map) would all serialise on bin 0: they are counted per wave with a ballot and
//     a population count into a wave-uniform register and added to bin 0 once, at the end.
//   * elements of the padded channels c_real .. c - 1 are not counted, whatever they hold (c % 8 == 0: a vector never crosses a
//     pixel; the channel of a vector's first element is one 32-bit modulo per vector, and only where c_real < c).
//   * the non-empty bins are flushed with 64-bit vector atomic adds to hist.  Integer sums do not depend on the order.
//   * no u32 bin can wrap: the entry point refuses maps of more than 2^39 elements, so a workgroup's share
//     (ceil(chunks / workgroups) chunks) stays below 2^32 elements.
#include "common.h"

namespace {

constexpr int CH_THREADS = 1024;
constexpr int CH_BINS = 32768;
constexpr int CH_VECS = LFD_CALIB_HIST_CHUNK_VECS;
constexpr int CH_LOADS = CH_VECS / CH_THREADS;           // 16-byte loads of a thread per chunk
constexpr int CH_LDS_BYTES = CH_BINS * 4;
static_assert(CH_VECS % CH_THREADS == 0, "a chunk is a whole number of loads per thread");
// share of a workgroup: ceil(chunks / MAX_WORKGROUPS) chunks of 8 CH_VECS elements, chunks <= 2^39 / (8 CH_VECS) + 1
static_assert(((1ll << 39) / (8ll * CH_VECS) / LFD_CALIB_HIST_MAX_WORKGROUPS + 1) * 8ll * CH_VECS < (1ll << 32), "u32 bins");

template <bool PADDED>
__global__ __launch_bounds__(CH_THREADS) void k_abs_hist_f16(const uint4* __restrict__ x, long nvec, int cvecs, int c_real,
                                                             unsigned long long* __restrict__ hist) {
  extern __shared__ __attribute__((aligned(16))) unsigned int bins[];
  const int tid = threadIdx.x;
  for (int i = tid; i < CH_BINS / 4; i += CH_THREADS) reinterpret_cast<uint4*>(bins)[i] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();

  unsigned int zeros = 0;       // of this wave (wave-uniform)
  const long nchunks = (nvec + CH_VECS - 1) / CH_VECS;
  for (long ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const long v0 = ch * CH_VECS;
    uint4 v[CH_LOADS];
    bool ok[CH_LOADS];
#pragma unroll
    for (int u = 0; u < CH_LOADS; ++u) {
      const long i = v0 + u * CH_THREADS + tid;
      ok[u] = i < nvec;
      v[u] = x[ok[u] ? i : 0];
    }
    const unsigned int cv0 = PADDED ? (unsigned int)(v0 % cvecs) : 0u;      // (block-uniform)
#pragma unroll
    for (int u = 0; u < CH_LOADS; ++u) {
      // channels this vector may count: all 8, or those below c_real
      const int left = PADDED ? c_real - 8 * (int)((cv0 + (unsigned int)(u * CH_THREADS + tid)) % (unsigned int)cvecs) : 8;
      const unsigned int w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const unsigned int bin = (w[j >> 1] >> (16 * (j & 1))) & 0x7fffu;
        const bool counted = ok[u] && j < left;
        zeros += (unsigned int)__builtin_popcountll(__ballot(counted && bin == 0u));
        if (counted && bin != 0u) atomicAdd(&bins[bin], 1u);
      }
    }
  }
  if ((tid & 63) == 0 && zeros) atomicAdd(&bins[0], zeros);
  __syncthreads();
  for (int i = tid; i < CH_BINS; i += CH_THREADS) {
    const unsigned int cnt = bins[i];
    if (cnt) atomicAdd(hist + i, (unsigned long long)cnt);
  }
}

template <bool PADDED>
int launch_hist(const uint4* x, long nvec, int cvecs, int c_real, unsigned long long* hist, hipStream_t st) {
  auto kern = k_abs_hist_f16<PADDED>;
  static unsigned long long attr_done_mask = 0;
  const int attr_done_dev = lfd_device_ordinal();
  if (LFD_ONCE_PER_DEVICE(attr_done_mask, attr_done_dev)) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, CH_LDS_BYTES) !=
        hipSuccess)
      return LFD_ERR_LAUNCH_FAILED;
    LFD_DONE_ON_DEVICE(attr_done_mask, attr_done_dev);
  }
  const long nchunks = (nvec + CH_VECS - 1) / CH_VECS;
  const int blocks = nchunks < LFD_CALIB_HIST_MAX_WORKGROUPS ? (int)nchunks : LFD_CALIB_HIST_MAX_WORKGROUPS;
  hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(CH_THREADS), CH_LDS_BYTES, st, x, nvec, cvecs, c_real, hist);
  LFD_CHECK_LAUNCH();
  return LFD_OK;
}

}  // namespace

extern "C" int lfd_abs_histogram_f16(const void* x, int64_t rows, int32_t c, int32_t c_real, uint64_t* hist,
                                     lfd_stream_t stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (!hist || rows < 0 || c < 8 || c % 8 || c_real < 1 || c_real > c) return LFD_ERR_INVALID_ARGUMENT;
  if (reinterpret_cast<uintptr_t>(hist) & 7) return LFD_ERR_INVALID_ARGUMENT;
  if (rows == 0) return LFD_OK;
  if (!x || !lfd_aligned16(x)) return LFD_ERR_INVALID_ARGUMENT;
  if (rows > (1ll << 39) / c) return LFD_ERR_UNSUPPORTED;       // a workgroup's u32 bins must not wrap (see the header)
  const long nvec = (long)rows * (c / 8);
  unsigned long long* h = reinterpret_cast<unsigned long long*>(hist);
  return c_real < c ? launch_hist<true>((const uint4*)x, nvec, c / 8, c_real, h, st)
                    : launch_hist<false>((const uint4*)x, nvec, c / 8, c_real, h, st);
}
