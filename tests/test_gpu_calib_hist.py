"""lfd_abs_histogram_f16 (csrc/calib_hist.hip, ops.abs_histogram_f16) on the MI355X against numpy.bincount of the bit patterns,
exact: one element, a padded map, every pattern once beside 2^20 zeros (the contended bin), a multi-chunk walk whose size follows
from the kernel's grid cap and chunk size (tests/golden/calib_cases.py restates them), accumulation into one histogram, and
bit-equal repeats."""
import numpy as np
import pytest
import torch

import calib_cases as CC
from lfd_amd import ops

pytestmark = pytest.mark.gpu


def _bits_tensor(bits, c):
    """uint16 patterns (numpy, any shape with rows * c elements) -> (fp16 device tensor [rows, c], the same as numpy float16)"""
    host = np.ascontiguousarray(bits.astype(np.uint16)).reshape(-1, c).view(np.float16)
    return torch.from_numpy(host.view(np.int16).copy()).view(torch.float16).cuda(), host


def _random_bits(count, seed, zero_share=0.5):
    """post-ReLU-like patterns: zero_share zeros (some of them -0), the rest finite values of either sign"""
    rng = np.random.RandomState(seed)
    mag = rng.randint(1, CC.FIRST_NONFINITE, size=count).astype(np.uint16)
    sign = (rng.randint(0, 2, size=count) << 15).astype(np.uint16)
    bits = mag | sign
    bits[rng.rand(count) < zero_share] &= 0x8000
    return bits


def test_one_element():
    t, host = _bits_tensor(np.array([0x3c00, 1, 2, 3, 4, 5, 6, 7]), 8)
    h = ops.abs_histogram_f16(t, c_real=1)
    assert h.dtype == torch.int64 and h.shape == (CC.BINS,) and h.is_cuda
    want = np.zeros(CC.BINS, dtype=np.int64)
    want[0x3c00] = 1
    assert np.array_equal(h.cpu().numpy(), want)
    neg, _ = _bits_tensor(np.array([0xbc00, 1, 2, 3, 4, 5, 6, 7]), 8)            # -1.0 counts in the bin of 1.0
    assert np.array_equal(ops.abs_histogram_f16(neg, c_real=1).cpu().numpy(), want)


def test_padded_map_does_not_count_the_padded_channels():
    rows, c, c_real = 37, 64, 48
    bits = _random_bits(rows * c, 1).reshape(rows, c)
    bits[:, c_real:] = np.random.RandomState(2).randint(1, 0x8000, size=(rows, c - c_real))      # garbage, NaN patterns included
    t, host = _bits_tensor(bits, c)
    got = ops.abs_histogram_f16(t, c_real=c_real).cpu().numpy()
    assert np.array_equal(got, CC.bincount_reference(host, c_real)) and int(got.sum()) == rows * c_real
    for cr in (1, 7, 8, 9, 63, 64):
        assert np.array_equal(ops.abs_histogram_f16(t, c_real=cr).cpu().numpy(), CC.bincount_reference(host, cr)), cr
    assert np.array_equal(ops.abs_histogram_f16(t).cpu().numpy(), CC.bincount_reference(host, c))        # default: every channel


def test_all_patterns_once_and_the_contended_zero_bin():
    pats = np.arange(1, CC.BINS, dtype=np.uint16)                   # every non-zero magnitude, Inf and the NaNs included
    pats[::2] |= 0x8000
    zeros = np.zeros(2 ** 20 + 1, dtype=np.uint16)                   # + bin 0's own "once"
    zeros[::3] = 0x8000                                              # -0
    bits = np.concatenate([zeros[:2 ** 19], pats, zeros[2 ** 19:]])
    assert bits.size % 8 == 0
    t, host = _bits_tensor(bits, 8)
    got = ops.abs_histogram_f16(t).cpu().numpy()
    assert got[0] == 2 ** 20 + 1 and bool((got[1:] == 1).all())
    assert np.array_equal(got, CC.bincount_reference(host, 8))


@pytest.mark.parametrize('c,c_real', [(8, 8), (24, 19)])
def test_multi_chunk_walk_with_a_ragged_last_chunk(c, c_real):
    rows = CC.multi_chunk_rows(c)
    bits = _random_bits(rows * c, 3 + c)
    bits[-5:] = [0x7bff, 0x0001, 0x8000, 0x3555, 0xfbff]             # the ragged chunk's last vector
    t, host = _bits_tensor(bits, c)
    want = CC.bincount_reference(host, c_real)
    a = ops.abs_histogram_f16(t, c_real=c_real)
    b = ops.abs_histogram_f16(t, c_real=c_real)
    assert np.array_equal(a.cpu().numpy(), want) and int(want.sum()) == rows * c_real
    assert torch.equal(a, b)                                         # two runs: equal bits


def test_two_calls_into_one_histogram_add_and_an_empty_tensor_adds_nothing():
    t1, h1 = _bits_tensor(_random_bits(301 * 16, 10), 16)
    t2, h2 = _bits_tensor(_random_bits(77 * 32, 11, zero_share=0.0), 32)
    out = ops.abs_histogram_f16(t1, c_real=13)
    ret = ops.abs_histogram_f16(t2, c_real=32, out=out)
    assert ret is out
    ops.abs_histogram_f16(torch.empty((0, 16), dtype=torch.float16, device='cuda'), out=out)
    assert np.array_equal(out.cpu().numpy(), CC.bincount_reference(h1, 13) + CC.bincount_reference(h2, 32))
    with pytest.raises(RuntimeError):
        ops.abs_histogram_f16(t1, out=torch.zeros(CC.BINS, dtype=torch.int32, device='cuda'))
    with pytest.raises(RuntimeError):
        ops.abs_histogram_f16(t1.float())
    with pytest.raises(RuntimeError):
        ops.abs_histogram_f16(t1, c_real=17)
