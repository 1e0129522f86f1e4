"""csrc/block_i8.hip and the pair instances of csrc/conv_i8.hip on the MI355X: lfd_block_i8_fused and lfd_conv2d_downsample_nhwc_i8 against the integer reference of
tests/golden/block_i8_cases.py (power-of-two constants: bit for bit) and against the lfd_conv2d_nhwc_i8 launches they replace
(arbitrary fp32 constants: bit for bit as well -- the sums are exact and the fp32 expressions are the same, so there is no
near-tie allowance), with and without the fp16 tap, on the 1 x 1 map, ragged maps and a tile walk past the grid cap; guard rows,
repeatability, and refused calls."""
import pytest
import torch

import block_i8_cases as BC
import conv_i8_cases as QC
from lfd_amd import _lib, ops

pytestmark = pytest.mark.gpu

SENTINEL_I8, SENTINEL_F16 = -128, -77.0       # -128 is outside the kernels' range; -77 is no value of a tap after ReLU


def _i8(rows, ch, guard):
    return torch.full((rows + guard, ch), SENTINEL_I8, dtype=torch.int8, device='cuda')


def _run_block(c, x, w1p, w2p, k1, k2, tap):
    """-> (out_i8, out_f16 | None); outputs pre-filled with sentinels, one guard pixel row behind the end"""
    rows = c.n * c.h * c.w
    q = _i8(rows, 64, c.w)
    f = torch.full((rows + c.w, 64), SENTINEL_F16, dtype=torch.float16, device='cuda') if tap else None
    ops.block_i8_fused(x, w1p, k1.mult.cuda(), k1.biasq.cuda(), w2p, k2.mult.cuda(), k2.biasq.cuda(), k2.res_mult,
                       out_scale=k2.out_scale if tap else None, out=q, out_f16=f)
    torch.cuda.synchronize()
    assert bool((q[rows:] == SENTINEL_I8).all()) and (f is None or bool((f[rows:] == SENTINEL_F16).all())), 'store past the end'
    assert bool((q[:rows] != SENTINEL_I8).all()), 'an output was not written'
    shape = (c.n, c.h, c.w, 64)
    return q[:rows].view(shape), (f[:rows].view(shape) if tap else None)


def _block_device_operands(c):
    x, w1, w2 = BC.block_operands(c)
    return x.cuda(), w1.cuda(), w2.cuda(), ops.pack_conv_weight_i8(w1).cuda(), ops.pack_conv_weight_i8(w2).cuda()


def _check_block_exact(c, big_bias):
    x, w1, w2, w1p, w2p = _block_device_operands(c)
    k1, k2 = BC.block_exact_constants(c, big_bias)
    mid, v, q_ref, f_ref = BC.block_ref(x, w1, w2, k1, k2)
    assert float(QC.acc_ref(x, w1, 1).abs().max()) < 2 ** 22 and float(QC.acc_ref(mid, w2, 1).abs().max()) < 2 ** 22
    assert torch.equal(v.float().double(), v)                              # the instrument: exact in fp32
    q, f = _run_block(c, x, w1p, w2p, k1, k2, tap=True)
    bad = int((q != q_ref).sum())
    assert bad == 0, '%d of %d int8 outputs differ' % (bad, q.numel())
    assert torch.equal(f.view(torch.int16), f_ref.float().half().view(torch.int16)), 'fp16 tap'
    q2, f2 = _run_block(c, x, w1p, w2p, k1, k2, tap=False)                 # no tap: the same int8, nothing else
    assert f2 is None and torch.equal(q2, q)
    q3, f3 = _run_block(c, x, w1p, w2p, k1, k2, tap=True)                  # two runs, the same bits
    assert torch.equal(q3, q) and torch.equal(f3.view(torch.int16), f.view(torch.int16))
    return q_ref


@pytest.mark.parametrize('c', BC.block_cases(), ids=BC.block_id)
def test_block_power_of_two_constants_bit_for_bit(c):
    q_ref = _check_block_exact(c, big_bias=False)
    if c.kind != 'pixel':
        assert int(q_ref.max()) == 127 and int(q_ref.min()) == 0           # ReLU floor and the upper clamp are both reached


@pytest.mark.parametrize('c', BC.block_cases()[:2], ids=BC.block_id)
def test_block_mid_pixels_outside_the_image_are_zero_padding(c):
    """conv1's biasq is 64 in every channel: conv1 evaluated on the all-zero input outside the image would be 64, the padding
    rule says 0 (tests/test_block_i8_host.py shows that the two differ in the reference)"""
    _check_block_exact(c, big_bias=True)


@pytest.mark.parametrize('c', BC.block_cases(), ids=BC.block_id)
def test_block_random_constants_equal_the_two_launch_route(c):
    x, _, _, w1p, w2p = _block_device_operands(c)
    k1, k2 = BC.block_random_constants(c)
    mid, _ = ops.conv2d_nhwc_i8(x, w1p, k1.mult.cuda(), k1.biasq.cuda(), 64, 3, 1, True)
    q_ref, f_ref = ops.conv2d_nhwc_i8(mid, w2p, k2.mult.cuda(), k2.biasq.cuda(), 64, 3, 1, True, residual=x, res_mult=k2.res_mult,
                                      out_scale=k2.out_scale)
    for tap in (True, False):
        q, f = _run_block(c, x, w1p, w2p, k1, k2, tap)
        assert torch.equal(q, q_ref)
        assert (f is None) == (not tap) and (f is None or torch.equal(f.view(torch.int16), f_ref.view(torch.int16)))


def _run_pair(c, x, w3p, wdp, k3, kd):
    oh, ow = BC.pair_out_hw(c.h, c.w)
    rows = c.n * oh * ow
    q, d = _i8(rows, c.cout, ow), _i8(rows, c.cout, ow)
    ops.conv2d_downsample_nhwc_i8(x, w3p, k3.mult.cuda(), k3.biasq.cuda(), wdp, kd.mult.cuda(), kd.biasq.cuda(), c.cout, out=q, ds_out=d)
    torch.cuda.synchronize()
    assert bool((q[rows:] == SENTINEL_I8).all()) and bool((d[rows:] == SENTINEL_I8).all()), 'store past the end'
    assert bool((q[:rows] != SENTINEL_I8).all()) and bool((d[:rows] != SENTINEL_I8).all()), 'an output was not written'
    shape = (c.n, oh, ow, c.cout)
    return q[:rows].view(shape), d[:rows].view(shape)


def _pair_device_operands(c):
    x, w3, wd = BC.pair_operands(c)
    return x.cuda(), w3.cuda(), wd.cuda(), ops.pack_conv_weight_i8(w3).cuda(), ops.pack_conv_weight_i8(wd).cuda()


@pytest.mark.parametrize('c', BC.pair_cases(), ids=BC.pair_id)
def test_pair_power_of_two_constants_bit_for_bit(c):
    x, w3, wd, w3p, wdp = _pair_device_operands(c)
    k3, kd = BC.pair_exact_constants(c)
    v3, q3_ref, vd, qd_ref = BC.pair_ref(x, w3, wd, k3, kd)
    assert float(QC.acc_ref(x, w3, 2).abs().max()) < 2 ** 22
    assert torch.equal(v3.float().double(), v3) and torch.equal(vd.float().double(), vd)
    q3, qd = _run_pair(c, x, w3p, wdp, k3, kd)
    assert int((q3 != q3_ref).sum()) == 0, '3x3 stride-2 output'
    assert int((qd != qd_ref).sum()) == 0, 'identity branch'
    if c.kind != 'pixel':
        assert int(q3_ref.min()) == 0 and int(qd_ref.min()) == -127       # ReLU on the one, none on the other
    q3b, qdb = _run_pair(c, x, w3p, wdp, k3, kd)
    assert torch.equal(q3b, q3) and torch.equal(qdb, qd)


@pytest.mark.parametrize('c', [c for c in BC.pair_cases() if c.kind != 'pixel'], ids=BC.pair_id)
def test_pair_random_constants_equal_the_two_launches(c):
    x, w3, wd, w3p, wdp = _pair_device_operands(c)
    k3, kd = BC.pair_random_constants(c)
    q3_ref, _ = ops.conv2d_nhwc_i8(x, w3p, k3.mult.cuda(), k3.biasq.cuda(), c.cout, 3, 2, True)
    qd_ref, _ = ops.conv2d_nhwc_i8(x, wdp, kd.mult.cuda(), kd.biasq.cuda(), c.cout, 1, 2, False)
    q3, qd = _run_pair(c, x, w3p, wdp, k3, kd)
    assert torch.equal(q3, q3_ref) and torch.equal(qd, qd_ref)


def test_refused_launches_write_nothing():
    l = _lib.lib()
    p, sp = _lib.ptr, _lib.stream_ptr()
    x = torch.zeros((1, 4, 4, 64), dtype=torch.int8, device='cuda')
    out = torch.full((1, 4, 4, 128), -128, dtype=torch.int8, device='cuda')
    ds = torch.full((1, 4, 4, 128), -128, dtype=torch.int8, device='cuda')
    f = torch.full((1, 4, 4, 64), SENTINEL_F16, dtype=torch.float16, device='cuda')
    w = torch.zeros(128 * 128 * 9, dtype=torch.int8, device='cuda')
    m = torch.ones(128, device='cuda')

    def block(n=1, h=4, w_=4, x_=x, o=out, f_=f, m_=m):
        return l.lfd_block_i8_fused(n, h, w_, p(x_), p(w), p(m_), p(m), p(w), p(m), p(m), 0.5, p(o), p(f_), 1.0, sp)

    assert block(x_=None) == -1 and block(o=None) == -1 and block(m_=None) == -1
    assert block(n=0) == -1 and block(h=0) == -1 and block(w_=0) == -1
    assert block(o=x) == -1                                                 # out_i8 aliases in
    assert block(m_=m[1:]) == -1 and block(f_=f.view(-1)[1:]) == -1         # misaligned
    assert block(h=4096, w_=4096) == -4

    def pair(cin=64, cout=64, x_=x, o=out, d=ds, h=4):
        return l.lfd_conv2d_downsample_nhwc_i8(1, h, 4, cin, cout, p(x_), p(w), p(m), p(m), p(w), p(m), p(m), p(o), p(d), sp)

    assert pair(cin=32) == -4 and pair(cin=128, cout=64) == -4 and pair(cout=256) == -4
    assert pair(x_=None) == -1 and pair(d=None) == -1 and pair(h=0) == -1 and pair(o=x) == -1 and pair(d=out) == -1
    assert pair(d=ds.view(-1)[1:]) == -1
    for key in BC.PAIR_KEYS:
        assert ops.conv2d_downsample_i8_supported(*key)
    assert not ops.conv2d_downsample_i8_supported(128, 64)
    torch.cuda.synchronize()
    assert bool((out == -128).all()) and bool((ds == -128).all()) and bool((f == SENTINEL_F16).all()) and not bool(x.any())
