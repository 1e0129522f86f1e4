"""Restatements for the INT8 calibration tests (tests/test_calibration_host.py, tests/test_gpu_calib_hist.py,
tests/test_gpu_int8_calibration.py):

  * the threshold rules of lfd_amd/calibration.py written again as plain float64 loops over Python numbers, from the definitions
    in DESIGN 4k and not from the module (no numpy arithmetic: numpy only makes the seeded inputs);
  * seeded magnitude histograms;
  * the geometry of csrc/calib_hist.hip (include/lfd_hip.h: LFD_CALIB_HIST_*), from which the multi-chunk case is derived, and
    the histogram of a tensor by numpy.bincount of its bit patterns."""
import math
import struct

import numpy as np

BINS = 32768
FIRST_NONFINITE = 0x7c00

# ---- geometry of the histogram kernel, restated (the host test compares these with the header)
MAX_WORKGROUPS = 256
CHUNK_VECS = 4096            # 16-byte vectors per chunk
VEC_ELEMS = 8


def val(b):
    """the fp16 value of pattern b, as a Python float"""
    return struct.unpack('<e', struct.pack('<H', b))[0]


def multi_chunk_rows(c):
    """rows of a [rows, c] map that every workgroup of a full grid walks at least twice, some three times, with a ragged last
    chunk"""
    cvecs = c // VEC_ELEMS
    nvec = (2 * MAX_WORKGROUPS + 2) * CHUNK_VECS + 1237
    rows = nvec // cvecs
    nvec = rows * cvecs
    chunks = -(-nvec // CHUNK_VECS)
    assert chunks >= 2 * MAX_WORKGROUPS + 1 and nvec % CHUNK_VECS != 0
    return rows


def bincount_reference(t, c_real):
    """t: numpy float16 [rows, c] -> int64 [32768] over the channels below c_real"""
    bits = np.ascontiguousarray(t[:, :c_real]).view(np.uint16).astype(np.int64) & 0x7fff
    return np.bincount(bits.ravel(), minlength=BINS).astype(np.int64)


# ---- seeded histograms
def _hist_of(values):
    return bincount_reference(np.asarray(values, dtype=np.float32).astype(np.float16).reshape(-1, 1), 1)


def seeded_histograms():
    """{name: int64 [32768]}: half-normal; post-ReLU with half zeros; a single spike over a body; two far-apart clusters"""
    rng = np.random.RandomState(20240)
    out = {}
    out['half_normal'] = _hist_of(np.abs(rng.randn(60000)) * 3.0)
    x = rng.randn(60000) * 2.0
    out['post_relu'] = _hist_of(np.maximum(x, 0.0))
    body = np.abs(rng.randn(40000)) * 0.5
    out['spike'] = _hist_of(np.concatenate([body, [240.0]]))
    out['two_clusters'] = _hist_of(np.concatenate([1.0 + 0.05 * rng.randn(30000), 50.0 + 1.5 * rng.randn(300)]))
    return out


# ---- the rules, as loops
def amax_ref(h):
    a = 0.0
    for b in range(BINS):
        if h[b]:
            a = val(b)
    return a


def clipped_ref(h, t):
    n = above = 0
    for b in range(FIRST_NONFINITE):
        n += int(h[b])
        if val(b) > t:
            above += int(h[b])
    return above / n if n else 0.0


def candidates_ref(nbins, start_bin, stride):
    out = []
    i = start_bin
    while i <= nbins:
        out.append(i)
        i += stride
    if out[-1] != nbins:
        out.append(nbins)
    return out


def cand_threshold_ref(i, a, nbins):
    return a if i == nbins else i * a / nbins


def percentile_ref(h, percentile):
    n = sum(int(c) for c in h)
    if n == 0 or amax_ref(h) == 0.0:
        return 0.0
    k = int(math.ceil(float(n) * percentile / 100.0))
    k = min(max(k, 1), n)
    run = 0
    for b in range(BINS):
        run += int(h[b])
        if run >= k:
            return val(b)


def linear_ref(h, a, nbins):
    lin = [0] * nbins
    for b in range(1, FIRST_NONFINITE):
        if h[b]:
            lin[min(nbins - 1, int(math.floor(val(b) * nbins / a)))] += int(h[b])
    return lin


def entropy_ref(h, nbins, nlevels, start_bin, stride):
    a = amax_ref(h)
    if a == 0.0:
        return 0.0
    lin = linear_ref(h, a, nbins)
    best, best_i = math.inf, None
    for i in candidates_ref(nbins, start_bin, stride):
        p = [float(c) for c in lin[:i]]
        p[i - 1] += float(sum(lin[i:]))
        q = [0.0] * i
        for g in range(nlevels):
            lo, hi = g * i // nlevels, (g + 1) * i // nlevels
            total = sum(lin[lo:hi])
            count = sum(1 for b in range(lo, hi) if lin[b])
            for b in range(lo, hi):
                if lin[b]:
                    q[b] = float(total) / float(count)
        sp, sq = float(sum(lin)), float(sum(lin[:i]))
        terms, kl = [], None
        for b in range(i):
            if p[b] > 0.0:
                if q[b] == 0.0:
                    kl = math.inf
                    break
                big_p, big_q = p[b] / sp, q[b] / sq
                terms.append(big_p * math.log(big_p / big_q))
        if kl is None:
            kl = math.fsum(terms)
        if kl < best:
            best, best_i = kl, i
    return a if best_i is None else cand_threshold_ref(best_i, a, nbins)


def mse_ref(h, nbins, start_bin, stride):
    a = amax_ref(h)
    if a == 0.0:
        return 0.0
    live = [(val(b), float(h[b])) for b in range(1, FIRST_NONFINITE) if h[b]]
    best, best_t = math.inf, a
    for i in candidates_ref(nbins, start_bin, stride):
        t = cand_threshold_ref(i, a, nbins)
        s = t / 127.0
        terms = []
        for v, c in live:
            d = v - s * min(127.0, float(round(v / s)))         # round(): half to even
            terms.append(c * (d * d))
        err = math.fsum(terms)
        if err < best:
            best, best_t = err, t
    return best_t
