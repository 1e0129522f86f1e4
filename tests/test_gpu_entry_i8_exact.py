"""csrc/entry_i8.hip on the MI355X: lfd_entry_i8_fused against the integer reference of tests/golden/entry_i8_cases.py
(power-of-two constants: bit for bit) and against the lfd_conv2d_downsample_nhwc_i8 + lfd_conv2d_nhwc_i8 launches it replaces
(arbitrary fp32 constants: bit for bit as well -- the sums are exact and the fp32 expressions are the same, so there is no
near-tie allowance); the fp16 input format against the quantise launch followed by the int8 format; on the 1 x 1 map, ragged
maps and tile walks of 1.5 and 3.5 tiles per workgroup past the grid cap; guard rows, repeatability, and refused calls."""
import pytest
import torch

import conv_i8_cases as QC
import entry_i8_cases as EC
from lfd_amd import _lib, ops

pytestmark = pytest.mark.gpu

SENTINEL_I8 = -128       # outside the kernel's range


def _run(c, x, wp, ks, inv_scale=0.0):
    """-> out_i8 [n,oh,ow,64]; the output pre-filled with the sentinel, one guard pixel row in front and one behind"""
    k1, kd, k2 = ks
    oh, ow = EC.out_hw(c.h, c.w)
    rows = c.n * oh * ow
    buf = torch.full((ow + rows + ow, 64), SENTINEL_I8, dtype=torch.int8, device='cuda')
    q = buf[ow:ow + rows].view(c.n, oh, ow, 64)
    got = ops.entry_i8_fused(x, wp[0], k1.mult.cuda(), k1.biasq.cuda(), wp[1], kd.mult.cuda(), kd.biasq.cuda(), wp[2], k2.mult.cuda(),
                             k2.biasq.cuda(), k2.res_mult, inv_scale=inv_scale, out=q)
    torch.cuda.synchronize()
    assert got.data_ptr() == q.data_ptr()
    assert bool((buf[:ow] == SENTINEL_I8).all()) and bool((buf[ow + rows:] == SENTINEL_I8).all()), 'store outside the output'
    assert bool((q != SENTINEL_I8).all()), 'an output was not written'
    return q


def _device_operands(c):
    x, w1, wd, w2 = EC.operands(c)
    return x.cuda(), (w1.cuda(), wd.cuda(), w2.cuda()), tuple(ops.pack_conv_weight_i8(w).cuda() for w in (w1, wd, w2))


def _check_exact(c, big_bias):
    x, (w1, wd, w2), wp = _device_operands(c)
    ks = EC.exact_constants(c, big_bias)
    y1, ident, v, q_ref = EC.entry_ref(x, w1, wd, w2, *ks)
    assert float(QC.acc_ref(x, w1, 2).abs().max()) < 2 ** 22 and float(QC.acc_ref(y1, w2, 1).abs().max()) < 2 ** 22
    assert torch.equal(v.float().double(), v)                              # the instrument: exact in fp32
    q = _run(c, x, wp, ks)
    bad = int((q != q_ref).sum())
    print('%s big_bias=%s: %d of %d int8 outputs differ' % (EC.case_id(c), big_bias, bad, q.numel()))
    assert bad == 0, '%d of %d int8 outputs differ' % (bad, q.numel())
    assert torch.equal(_run(c, x, wp, ks), q)                              # two launches, the same bits
    return q_ref


@pytest.mark.parametrize('c', EC.cases(), ids=EC.case_id)
def test_power_of_two_constants_bit_for_bit(c):
    q_ref = _check_exact(c, big_bias=False)
    if c.kind != 'pixel':
        assert int(q_ref.max()) == 127 and int(q_ref.min()) == 0           # ReLU floor and the upper clamp are both reached


@pytest.mark.parametrize('c', EC.cases(), ids=EC.case_id)
def test_y1_pixels_outside_the_map_are_zero_padding(c):
    """conv1's biasq is 64 in every channel: conv1 evaluated on the all-zero input outside the map would be 64, the padding
    rule says 0 (tests/test_entry_i8_host.py shows that the two differ in the reference)"""
    _check_exact(c, big_bias=True)


def _replaced_launches(x, wp, ks):
    """lfd_conv2d_downsample_nhwc_i8 + lfd_conv2d_nhwc_i8 over int8 x -> out_i8"""
    k1, kd, k2 = ks
    y1, ident = ops.conv2d_downsample_nhwc_i8(x, wp[0], k1.mult.cuda(), k1.biasq.cuda(), wp[1], kd.mult.cuda(), kd.biasq.cuda(), 64)
    q, _ = ops.conv2d_nhwc_i8(y1, wp[2], k2.mult.cuda(), k2.biasq.cuda(), 64, 3, 1, True, residual=ident, res_mult=k2.res_mult)
    return q


@pytest.mark.parametrize('c', EC.cases(), ids=EC.case_id)
def test_random_constants_equal_the_launches_it_replaces(c):
    x, _, wp = _device_operands(c)
    ks = EC.random_constants(c)
    q_ref = _replaced_launches(x, wp, ks)
    q = _run(c, x, wp, ks)
    bad = int((q != q_ref).sum())
    print('%s: %d of %d int8 outputs differ from pair + conv' % (EC.case_id(c), bad, q.numel()))
    assert bad == 0
    assert torch.equal(_run(c, x, wp, ks), q)


@pytest.mark.parametrize('channels', EC.F16_CHANNELS)
@pytest.mark.parametrize('exact', [True, False], ids=['pow2_scale', 'fp32_scale'])
@pytest.mark.parametrize('c', [c for c in EC.cases() if c.kind in ('pixel', 'edge_even', 'general', 'walk', 'walk_deep')], ids=EC.case_id)
def test_fp16_input_equals_the_quantise_launch_followed_by_the_int8_format(c, exact, channels):
    _, _, wp = _device_operands(c)
    ks = EC.random_constants(c)
    x16, inv = EC.f16_input(c, channels, exact)
    xq = ops.quantize_f16_i8(x16.cuda(), inv, channels=64)
    assert torch.equal(xq.cpu(), EC.quantize_ref(x16, inv))                # the quantise launch is what the host says it is
    q_ref = _run(c, xq, wp, ks)
    assert torch.equal(q_ref, _replaced_launches(xq, wp, ks))
    q = _run(c, x16.cuda(), wp, ks, inv_scale=inv)
    bad = int((q != q_ref).sum())
    print('%s %d channels exact=%s: %d of %d int8 outputs differ' % (EC.case_id(c), channels, exact, bad, q.numel()))
    assert bad == 0
    assert torch.equal(_run(c, x16.cuda(), wp, ks, inv_scale=inv), q)


def test_refused_launches_write_nothing():
    l = _lib.lib()
    p, sp = _lib.ptr, _lib.stream_ptr()
    x = torch.zeros((1, 4, 4, 64), dtype=torch.int8, device='cuda')
    x16 = torch.zeros((1, 4, 4, 64), dtype=torch.float16, device='cuda')
    out = torch.full((1, 2, 2, 64), SENTINEL_I8, dtype=torch.int8, device='cuda')
    w = torch.zeros(64 * 64 * 9, dtype=torch.int8, device='cuda')
    m = torch.ones(64, device='cuda')

    def entry(n=1, h=4, w_=4, fmt=0, ch=64, x_=x, o=out, m_=m, w2=w):
        return l.lfd_entry_i8_fused(n, h, w_, fmt, ch, p(x_), 1.0, p(w), p(m_), p(m), p(w), p(m), p(m), p(w2), p(m), p(m), 0.5, p(o), sp)

    assert entry(x_=None) == -1 and entry(o=None) == -1 and entry(m_=None) == -1 and entry(w2=None) == -1
    assert entry(n=0) == -1 and entry(h=0) == -1 and entry(w_=0) == -1
    assert entry(o=x) == -1 and entry(fmt=1, x_=x16, o=x16) == -1            # out_i8 aliases in
    assert entry(m_=m[1:]) == -1 and entry(o=out.view(-1)[1:]) == -1 and entry(fmt=1, x_=x16.view(-1)[1:]) == -1      # misaligned
    assert entry(ch=32) == -4 and entry(ch=128) == -4 and entry(fmt=1, ch=16, x_=x16) == -4 and entry(fmt=2) == -4
    assert entry(h=4096, w_=4096) == -4 and entry(fmt=1, ch=32, x_=x16, h=4096, w_=4096) == -4
    assert ops.entry_i8_fused_supported(0, 64) and all(ops.entry_i8_fused_supported(1, ch) for ch in EC.F16_CHANNELS)
    assert not ops.entry_i8_fused_supported(0, 32) and not ops.entry_i8_fused_supported(1, 128)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL_I8).all()) and not bool(x.any()) and not bool(x16.any())
