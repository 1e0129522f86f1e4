"""csrc/block128_i8.hip on the MI355X: lfd_block128_i8_fused against the integer reference of tests/golden/block128_i8_cases.py
(power-of-two constants: bit for bit) and against the two lfd_conv2d_nhwc_i8 launches it replaces (arbitrary fp32 constants: bit
for bit as well -- the sums are exact and the fp32 expressions are the same, so there is no near-tie allowance), with and without
the fp16 tap, on the 1 x 1 map, ragged maps and a tile walk of 3.5 tiles per workgroup past the grid cap; guard rows in front
of and behind both outputs, repeatability, and refused calls."""
import functools

import pytest
import torch

import block128_i8_cases as BC
import conv_i8_cases as QC
from lfd_amd import _lib, ops

pytestmark = pytest.mark.gpu

SENTINEL_I8, SENTINEL_F16 = -128, -77.0       # -128 is outside the kernel's range; -77 is no value of a tap after ReLU
CASES = BC.cases()


def _run(c, x, w1p, w2p, k1, k2, tap, into=None):
    """-> (out_i8, out_f16 | None, the guarded buffers); outputs pre-filled with sentinels, one guard pixel row (of the map's
    width) in front of the first pixel and one behind the last.  into: the guarded buffers of an earlier run, launched into
    again as they are"""
    rows, g = c.n * c.h * c.w, c.w
    if into is None:
        qg = torch.full((rows + 2 * g, BC.C), SENTINEL_I8, dtype=torch.int8, device='cuda')
        fg = torch.full((rows + 2 * g, BC.C), SENTINEL_F16, dtype=torch.float16, device='cuda')
    else:
        qg, fg = into
    q, f = qg[g:g + rows], fg[g:g + rows]
    ops.block128_i8_fused(x, w1p, k1.mult.cuda(), k1.biasq.cuda(), w2p, k2.mult.cuda(), k2.biasq.cuda(), k2.res_mult,
                          out_scale=k2.out_scale if tap else None, out=q, out_f16=f if tap else None)
    torch.cuda.synchronize()
    assert bool((qg[:g] == SENTINEL_I8).all()) and bool((qg[g + rows:] == SENTINEL_I8).all()), 'int8 store outside the map'
    assert bool((fg[:g] == SENTINEL_F16).all()) and bool((fg[g + rows:] == SENTINEL_F16).all()), 'fp16 store outside the map'
    assert bool((q != SENTINEL_I8).all()), 'an output was not written'
    if into is None:
        assert bool((f == SENTINEL_F16).all()) != tap, 'out_f16 = None must write no tap; a tap must be written'
    shape = (c.n, c.h, c.w, BC.C)
    return q.view(shape), (f.view(shape) if tap else None), (qg, fg)


@functools.lru_cache(maxsize=2)
def _device_operands(c):
    x, w1, w2 = BC.operands(c)
    return x.cuda(), w1.cuda(), w2.cuda(), ops.pack_conv_weight_i8(w1).cuda(), ops.pack_conv_weight_i8(w2).cuda()


def _check_exact(c, big_bias):
    x, w1, w2, w1p, w2p = _device_operands(c)
    k1, k2 = BC.exact_constants(c, big_bias)
    mid, v, q_ref, f_ref = BC.block128_ref(x, w1, w2, k1, k2)
    assert float(QC.acc_ref(x, w1, 1).abs().max()) < 2 ** 22 and float(QC.acc_ref(mid, w2, 1).abs().max()) < 2 ** 22
    assert torch.equal(v.float().double(), v)                              # the instrument: exact in fp32
    q, f, bufs = _run(c, x, w1p, w2p, k1, k2, tap=True)
    bad = int((q != q_ref).sum())
    assert bad == 0, '%d of %d int8 outputs differ' % (bad, q.numel())
    assert torch.equal(f.view(torch.int16), f_ref.float().half().view(torch.int16)), 'fp16 tap'      # half(float64), exactly
    q, f = q.clone(), f.clone()
    q2, f2, _ = _run(c, x, w1p, w2p, k1, k2, tap=False)                    # no tap: the same int8, nothing else written
    assert f2 is None and torch.equal(q2, q)
    q3, f3, _ = _run(c, x, w1p, w2p, k1, k2, tap=True, into=bufs)          # a second launch into the same buffers
    assert torch.equal(q3, q) and torch.equal(f3.view(torch.int16), f.view(torch.int16))
    return q_ref


@pytest.mark.parametrize('c', CASES, ids=BC.case_id)
def test_power_of_two_constants_bit_for_bit(c):
    q_ref = _check_exact(c, big_bias=False)
    if c.kind != 'pixel':
        assert int(q_ref.max()) == 127 and int(q_ref.min()) == 0           # ReLU floor and the upper clamp are both reached


@pytest.mark.parametrize('c', CASES, ids=BC.case_id)
def test_mid_pixels_outside_the_image_are_zero_padding(c):
    """conv1's biasq is 64 in every channel: conv1 evaluated on the all-zero input outside the image would be 64, the padding
    rule says 0 (tests/test_block128_i8_host.py shows that the two differ in the reference)"""
    _check_exact(c, big_bias=True)


@pytest.mark.parametrize('c', CASES, ids=BC.case_id)
def test_random_constants_equal_the_two_launches(c):
    x, _, _, w1p, w2p = _device_operands(c)
    k1, k2 = BC.random_constants(c)
    mid, _ = ops.conv2d_nhwc_i8(x, w1p, k1.mult.cuda(), k1.biasq.cuda(), BC.C, 3, 1, True)
    q_ref, f_ref = ops.conv2d_nhwc_i8(mid, w2p, k2.mult.cuda(), k2.biasq.cuda(), BC.C, 3, 1, True, residual=x, res_mult=k2.res_mult,
                                      out_scale=k2.out_scale)
    for tap in (True, False):
        q, f, _ = _run(c, x, w1p, w2p, k1, k2, tap)
        assert torch.equal(q, q_ref)
        assert (f is None) == (not tap) and (f is None or torch.equal(f.view(torch.int16), f_ref.view(torch.int16)))


def test_refused_launches_write_nothing():
    l = _lib.lib()
    p, sp = _lib.ptr, _lib.stream_ptr()
    x = torch.zeros((1, 4, 4, 128), dtype=torch.int8, device='cuda')
    out = torch.full((1, 4, 4, 128), -128, dtype=torch.int8, device='cuda')
    f = torch.full((1, 4, 4, 128), SENTINEL_F16, dtype=torch.float16, device='cuda')
    w = torch.zeros(128 * 128 * 9, dtype=torch.int8, device='cuda')
    m = torch.ones(128, device='cuda')

    def block(n=1, h=4, w_=4, x_=x, o=out, f_=f, m_=m):
        return l.lfd_block128_i8_fused(n, h, w_, p(x_), p(w), p(m_), p(m), p(w), p(m), p(m), 0.5, p(o), p(f_), 1.0, sp)

    assert block(x_=None) == -1 and block(o=None) == -1 and block(m_=None) == -1
    assert block(n=0) == -1 and block(h=0) == -1 and block(w_=0) == -1
    assert block(o=x) == -1                                                 # out_i8 aliases in
    assert block(m_=m[1:]) == -1 and block(f_=f.view(-1)[1:]) == -1         # misaligned
    assert block(h=4096, w_=4096) == -4
    torch.cuda.synchronize()
    assert bool((out == -128).all()) and bool((f == SENTINEL_F16).all()) and not bool(x.any())
    with pytest.raises(RuntimeError):
        ops.block128_i8_fused(torch.zeros((1, 4, 4, 64), dtype=torch.int8, device='cuda'), w, m, m, w, m, m, 0.5)
