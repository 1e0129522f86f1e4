"""csrc/conv_i8.hip on the MI355X against the float64 oracle of tests/golden/conv_i8_cases.py: (a) bit for bit with power-of-two
constants on every key, map and epilogue variant, tile walk included; (b) arbitrary fp32 constants, equal except at near-ties;
(c) the quantise launches bit for bit against torch; (d) the support query and refused launches.

The operands are full-range int8 and asymmetric in every axis, so (a) is also the check of the i8 MFMA's operand pairing and of
the C/D row map the packed filter order rests on (a wrong map leaves no output right)."""
import ctypes as C

import pytest
import torch

import conv_i8_cases as QC
from lfd_amd import _lib, ops

pytestmark = pytest.mark.gpu

SENTINEL_I8, SENTINEL_F16 = -128, -77.0       # -128 is outside the kernel's range; -77 is no value of v * 2^-3 after ReLU


def _launch(c, x, w_packed, k, res, relu, tap):
    """-> (out_i8, out_f16 | None), outputs pre-filled with sentinels and one guard pixel row behind the end"""
    oh, ow = QC.out_hw(c.h, c.w, c.ks, c.stride)
    rows = c.n * oh * ow
    q = torch.full((rows + ow, c.cout), SENTINEL_I8, dtype=torch.int8, device='cuda')
    f = torch.full((rows + ow, c.cout), SENTINEL_F16, dtype=torch.float16, device='cuda') if tap else None
    ops.conv2d_nhwc_i8(x, w_packed, k.mult.cuda(), k.biasq.cuda(), c.cout, c.ks, c.stride, relu, residual=res,
                       res_mult=k.res_mult, out_scale=k.out_scale if tap else None, out=q, out_f16=f)
    torch.cuda.synchronize()
    assert bool((q[rows:] == SENTINEL_I8).all()) and (f is None or bool((f[rows:] == SENTINEL_F16).all())), 'store past the end'
    shape = (c.n, oh, ow, c.cout)
    return q[:rows].view(shape), (f[:rows].view(shape) if tap else None)


def _device_operands(c):
    x, w, res = QC.operands(c)
    return x.cuda(), w.cuda(), res.cuda(), ops.pack_conv_weight_i8(w).cuda()


@pytest.mark.parametrize('c', QC.small_cases() + QC.walk_cases(), ids=QC.case_id)
def test_power_of_two_constants_bit_for_bit(c):
    x, w, res, wp = _device_operands(c)
    acc = QC.acc_ref(x, w, c.stride)
    assert float(acc.abs().max()) < 2 ** 22
    k = QC.exact_constants(c)
    variants = [(r, a) for r in (False, True) for a in (False, True)] if c.kind != 'walk' else [(True, True), (False, False)]
    for with_res, relu in variants:
        v, q_ref, f_ref = QC.epilogue_ref(acc, k, res if with_res else None, relu)
        assert torch.equal(v.float().double(), v)                      # the instrument: exact in fp32
        q, f = _launch(c, x, wp, k, res if with_res else None, relu, tap=True)
        assert bool((q != SENTINEL_I8).all()), 'an output was not written'
        bad = int((q != q_ref).sum())
        assert bad == 0, '%d of %d int8 outputs differ (res %s, relu %s)' % (bad, q.numel(), with_res, relu)
        assert torch.equal(f.view(torch.int16), f_ref.float().half().view(torch.int16)), 'fp16 tap (res %s, relu %s)' % (with_res, relu)
        q2, f2 = _launch(c, x, wp, k, res if with_res else None, relu, tap=False)       # no tap: the same int8, nothing else
        assert f2 is None and torch.equal(q2, q)


@pytest.mark.parametrize('c', QC.random_cases(), ids=QC.case_id)
def test_random_scales_equal_except_at_near_ties(c):
    x, w, res, wp = _device_operands(c)
    acc = QC.acc_ref(x, w, c.stride)
    k = QC.random_constants(c)
    for with_res in (False, True):
        for relu in (False, True):
            v, q_ref, f_ref = QC.epilogue_ref(acc, k, res if with_res else None, relu)
            tie = QC.near_tie(v)
            share = float(tie.double().mean())
            q, f = _launch(c, x, wp, k, res if with_res else None, relu, tap=True)
            diff = (q.int() - q_ref.int()).abs()
            print('%s res %d relu %d: near-tie share %.4f, differing outputs %d (at ties %d)'
                  % (QC.case_id(c), with_res, relu, share, int((diff > 0).sum()), int(((diff > 0) & tie).sum())))
            assert share <= QC.NEAR_TIE_CAP
            assert int(diff[~tie].max() if bool((~tie).any()) else 0) == 0, 'differs away from a near-tie'
            assert int(diff.max()) <= 1
            err = (f.double() - f_ref).abs()
            assert bool((err <= QC.f16_ulp(f_ref)).all()), 'fp16 tap beyond one ulp: %g' % float((err / QC.f16_ulp(f_ref)).max())


QUANT_REACH = 1024 * 256 * 16         # values one trip of the capped grid covers (csrc/conv_i8.hip: Q8_MAX_WORKGROUPS)


@pytest.mark.parametrize('count', [1, 15, 16, 17, QUANT_REACH + 16 * 300 + 5])
def test_quantize_bit_for_bit(count):
    g = torch.Generator().manual_seed(count)
    x = (torch.randn(count, generator=g) * 3).half()
    x[::7] = (torch.randint(-300, 301, (len(x[::7]),), generator=g).float() / 2 / 37.0).half()   # around ties of x * 37
    x = x.cuda()
    for inv_scale in (37.0, 1.0 / 0.0371, 1000.0):
        out = torch.full((count + 16,), -128, dtype=torch.int8, device='cuda')
        ops.quantize_f16_i8(x, inv_scale, out=out)
        ref = torch.round(x.float() * torch.tensor(inv_scale, dtype=torch.float32)).clamp(-127, 127).to(torch.int8)
        assert torch.equal(out[:count], ref) and bool((out[count:] == -128).all())
    if count > 100:
        assert int(ref.min()) == -127 and int(ref.max()) == 127          # (inv_scale 1000: both clamps)


@pytest.mark.parametrize('pixels,cin,cout', [(1, 32, 64), (37, 32, 64), (1000, 48, 64), (5, 64, 128)])
def test_quantize_pad_bit_for_bit(pixels, cin, cout):
    x = (torch.randn(pixels, cin, generator=torch.Generator().manual_seed(pixels)) * 2).half().cuda()
    out = torch.full((pixels + 1, cout), -128, dtype=torch.int8, device='cuda')
    ops.quantize_f16_i8(x, 29.5, out=out, channels=cout)
    ref = torch.round(x.float() * 29.5).clamp(-127, 127).to(torch.int8)
    assert torch.equal(out[:pixels, :cin], ref) and bool((out[:pixels, cin:] == 0).all()) and bool((out[pixels:] == -128).all())


def test_supported_answers_and_refused_launches_write_nothing():
    l = _lib.lib()
    for key in QC.KEYS:
        assert l.lfd_conv2d_nhwc_i8_supported(*key) == 0 and ops.conv2d_i8_supported(*key)
    for key in ((32, 64, 3, 1), (256, 64, 3, 1), (64, 32, 3, 1), (64, 256, 1, 1), (64, 64, 5, 1), (64, 64, 3, 3), (64, 64, 2, 1)):
        assert l.lfd_conv2d_nhwc_i8_supported(*key) == -4 and not ops.conv2d_i8_supported(*key)
    x = torch.zeros((1, 4, 4, 256), dtype=torch.int8, device='cuda')
    out = torch.full((1, 4, 4, 64), -128, dtype=torch.int8, device='cuda')
    f = torch.full((1, 4, 4, 64), SENTINEL_F16, dtype=torch.float16, device='cuda')
    w = torch.zeros(256 * 64 * 25, dtype=torch.int8, device='cuda')
    m = torch.ones(64, device='cuda')
    for (cin, ks) in ((32, 3), (256, 3), (64, 5)):
        d = _lib.ConvDesc(1, 4, 4, cin, 64, ks, 1, 1, 0, 0)
        rc = l.lfd_conv2d_nhwc_i8(C.byref(d), _lib.ptr(x), _lib.ptr(w), _lib.ptr(m), _lib.ptr(m), None, 0.0, _lib.ptr(out), _lib.ptr(f),
                                  1.0, _lib.stream_ptr())
        assert rc == -4
    d = _lib.ConvDesc(1, 4, 4, 64, 64, 3, 1, 1, 0, 0)
    assert l.lfd_conv2d_nhwc_i8(C.byref(d), None, _lib.ptr(w), _lib.ptr(m), _lib.ptr(m), None, 0.0, _lib.ptr(out), None, 1.0, None) == -1
    assert l.lfd_conv2d_nhwc_i8(C.byref(d), _lib.ptr(out), _lib.ptr(w), _lib.ptr(m), _lib.ptr(m), None, 0.0, _lib.ptr(out), None, 1.0,
                                None) == -1                                                    # in == out
    assert l.lfd_quantize_nhwc_f16_i8(None, _lib.ptr(out), 4, 1.0, None) == -1
    assert l.lfd_quantize_pad_nhwc_f16_i8(_lib.ptr(f), _lib.ptr(out), 4, 24, 64, 1.0, None) == -4
    torch.cuda.synchronize()
    assert bool((out == -128).all()) and bool((f == SENTINEL_F16).all())
