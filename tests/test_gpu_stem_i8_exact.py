"""The int8-output forms of the RGB stem launches on the MI355X -- lfd_stem_conv_i8 (csrc/stem.hip) and lfd_stem_faster_fused_i8
(csrc/stem_fused.hip, k_stem2x) -- compared in every bit (each assertion is torch.equal) with
  (i)  the fp16 entry point followed by lfd_quantize_nhwc_f16_i8 on the same operands: Gaussian frames and filters, an inv_scale
       that is no power of two and a second, four times as large, under which a share of the outputs clamps at 127;
  (ii) the host reference of tests/golden/stem_i8_cases.py: the integer operands of stem_cases.py with the power-of-two inv_scales
       0.5 (ties on x.5) and 2 (the clamp), for which the float64 chain is exact.
The output is a view in the middle of a buffer filled with -128, a value the clamp never produces, one map row of guard on either
side: no -128 may remain in the view and the guards must stay untouched.  A second launch into the same buffer gives the same
bytes.  Refused calls return their status and leave the buffer as it was.

Every knob change goes through `knobs`, which restores the previous value; the last test finds the knobs at their defaults."""
import contextlib

import pytest
import torch

import stem_cases as S
import stem_i8_cases as Q
from lfd_amd import _lib, engine, ops
from lfd_amd._lib import check, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def knobs(**kw):
    prev = {}
    try:
        for k, v in kw.items():
            prev[k] = _lib.tune(k, v)
        yield
    finally:
        for k, v in prev.items():
            _lib.tune(k, v)


def _case_knobs(c):
    kw = dict(S.needs_knobs(c.inst, c.route))
    if c.inst.kernel == 'stem2x':
        kw['X2_STAGGER'] = int(c.stagger)
    return kw


class Guarded(object):
    """the int8 output [n, oh, ow, 64], filled with -128, in the middle of a -128-filled buffer: one map row of guard on each side"""

    def __init__(self, shape):
        n = shape[0] * shape[1] * shape[2] * shape[3]
        self.guard = shape[2] * shape[3]
        assert self.guard % 16 == 0
        self.buf = torch.full((n + 2 * self.guard,), Q.FILL, dtype=torch.int8, device='cuda')
        self.view = self.buf[self.guard:self.guard + n].view(shape)
        assert self.view.data_ptr() % 16 == 0

    def check(self):
        g = self.guard
        assert not bool((self.view == Q.FILL).any()), 'unwritten output'
        assert bool((self.buf[:g] == Q.FILL).all()) and bool((self.buf[-g:] == Q.FILL).all()), 'written outside the output'


def _packed(stages):
    return [((engine.pack_stem_weight(w) if k == 0 else ops.pack_conv_weight(w)).cuda(), b.cuda()) for k, (w, b, _) in enumerate(stages)]


def _on_device(t, route):
    """the frame on the device; route 'misaligned': an fp16 frame at a base 2 bytes past a 16-byte boundary"""
    t = t.cuda()
    if route == 'misaligned':
        assert t.dtype == torch.float16
        buf = torch.zeros(t.numel() + 64, dtype=torch.float16, device='cuda')
        m = buf[1:1 + t.numel()].view_as(t)
        m.copy_(t)
        assert m.data_ptr() % 16 == 2
        return m
    assert t.data_ptr() % 16 == 0
    return t


def _launch_i8(inst, frame, packed, n, h, w, inv_scale, out):
    p = [ptr(x) for wb in packed for x in wb]
    if inst.kernel == 'stem':
        return lib().lfd_stem_conv_i8(ptr(frame), inst.fmt, n, h, w, inst.c, p[0], p[1], p[2], p[3], inv_scale, ptr(out), stream_ptr())
    return lib().lfd_stem_faster_fused_i8(ptr(frame), inst.fmt, n, h, w, inst.c, *p, inv_scale, ptr(out), stream_ptr())


def _launch_f16(inst, frame, packed, n, h, w, out):
    p = [ptr(x) for wb in packed for x in wb]
    if inst.kernel == 'stem':
        check(lib().lfd_stem_conv_f16(ptr(frame), inst.fmt, n, h, w, inst.c, p[0], p[1], p[2], p[3], ptr(out), stream_ptr()), 'f16')
    else:
        check(lib().lfd_stem_faster_fused_f16(ptr(frame), inst.fmt, n, h, w, inst.c, *p, ptr(out), stream_ptr()), 'f16')


def _run_i8(c, frame, packed, inv_scale):
    g = Guarded((c.n,) + S.out_map(c.inst, c.h, c.w) + (64,))
    with knobs(**_case_knobs(c)):
        check(_launch_i8(c.inst, frame, packed, c.n, c.h, c.w, inv_scale, g.view), S.case_id(c))
        torch.cuda.synchronize()
    g.check()
    return g


def _gauss_frame(inst, n, h, w, seed):
    """what the frame format holds for Gaussian-like operands: uniform fp16 / fp32 values, or random bytes"""
    gen = torch.Generator().manual_seed(seed)
    if inst.fmt == S.FMT_U8:
        return torch.randint(0, 256, (n, h, w, 3), dtype=torch.uint8, generator=gen)
    return S.to_format(inst, S.gauss_values(inst, n, h, w, seed))


def _check_case(c):
    """(i) and (ii) for one case"""
    inst = c.inst
    seed = S.case_seed(c)
    # ---- (i) Gaussian operands against the fp16 entry point + the quantise launch
    stages = S.gauss_stages(inst, seed + 1)
    packed = _packed(stages)
    frame = _on_device(_gauss_frame(inst, c.n, c.h, c.w, seed + 1), c.route)
    y = torch.empty((c.n,) + S.out_map(inst, c.h, c.w) + (64,), dtype=torch.float16, device='cuda')
    with knobs(**_case_knobs(c)):
        _launch_f16(inst, frame, packed, c.n, c.h, c.w, y)
    amax = float(y.float().abs().max())
    assert amax > 0
    inv = 113.7 / amax                                          # no power of two; nothing clamps
    for k, s in enumerate((inv, 4.0 * inv)):                    # ... and one under which a share of the outputs clamps
        want = ops.quantize_f16_i8(y, s)
        g = _run_i8(c, frame, packed, s)
        assert torch.equal(g.view, want), '%s: inv_scale %r' % (S.case_id(c), s)
        if y.numel() >= 4096:
            assert int(want.max()) == (127 if k else 114)       # rint(113.7); four times that is far above the clamp
            assert k == 0 or int((y.float() * s > 127.5).sum()) > 0
    again = _run_i8(c, frame, packed, 4.0 * inv)                # a second launch: the same bytes
    assert torch.equal(again.view, g.view)
    del y, want, g, again
    # ---- (ii) integer operands against the host reference
    values, stages = S.int_values(inst, c.n, c.h, c.w, seed), S.int_stages(inst, seed)
    packed = _packed(stages)
    frame = _on_device(S.to_format(inst, values), c.route)
    ref64 = S.ref_in_chunks(values.cuda(), stages)
    assert float(ref64.abs().max()) <= S.F16_EXACT
    for s in Q.INT_INV_SCALES:
        ref = torch.from_numpy(Q.quantize_ref(ref64, s)).cuda()
        g = _run_i8(c, frame, packed, s)
        assert torch.equal(g.view, ref), '%s: integer operands, inv_scale %r' % (S.case_id(c), s)


# ------------------------------------------------------------------------------------------------ (a) lfd_stem_conv_i8
@pytest.mark.parametrize('shape', Q.PAIR_SHAPES, ids=lambda s: '%dx%dx%d' % s)
@pytest.mark.parametrize('inst', Q.PAIR_INSTANCES, ids=S.inst_id)
def test_stem_conv_i8(inst, shape):
    _check_case(Q.as_case(inst, shape))


@pytest.mark.parametrize('shape', Q.PAIR_SHAPES[2:4], ids=lambda s: '%dx%dx%d' % s)
def test_stem_conv_i8_uint8_frames_give_the_bits_of_their_fp16_frames(shape):
    """frames of the bytes {0, 255} == the same frames as -1 / +1 in fp16 NHWC and in fp32 NCHW"""
    u8 = Q.PAIR_INSTANCES[2]
    c = Q.as_case(u8, shape)
    values, stages = S.int_values(u8, c.n, c.h, c.w, S.case_seed(c)), S.gauss_stages(u8, 3)
    assert bool((values.abs() == 1).all())
    packed = _packed(stages)
    a = _run_i8(c, S.to_format(u8, values).cuda(), packed, 40.0)
    assert int(a.view.max()) > 10
    for other in Q.PAIR_INSTANCES[:2]:
        b = _run_i8(c._replace(inst=other), S.to_format(other, values).cuda(), packed, 40.0)
        assert torch.equal(a.view, b.view), S.inst_id(other)


# ------------------------------------------------------------------------------------------------ (b) lfd_stem_faster_fused_i8
X2_PARAMS = [(i, c) for i in Q.X2_INSTANCES for c in Q.x2_cases(i)]


@pytest.mark.parametrize('inst,case', X2_PARAMS, ids=['%s_%s' % (S.inst_id(i), Q.x2_case_id(c)) for i, c in X2_PARAMS])
def test_stem_faster_fused_i8(inst, case):
    _check_case(Q.as_case(inst, case))


@pytest.mark.parametrize('fmt', [S.FMT_F16, S.FMT_U8], ids=['f16', 'u8'])
def test_stem_faster_fused_i8_general_kernel_equals_the_aligned_one(fmt):
    """X2_ALN = 0 against 1 on the same 16-byte-row frames, bit for bit (896 tiles: every LDS buffer and the ring are reused);
    uint8 frames of {0, 255} against their -1 / +1 fp16 frames"""
    aln, gen = S.Inst('stem2x', 64, fmt, 1, 1), S.Inst('stem2x', 64, fmt, 1, 0)
    c = Q.as_case(aln, Q.X2_896)
    stages = S.gauss_stages(aln, 11)
    packed = _packed(stages)
    values = S.int_values(aln, c.n, c.h, c.w, 11, pm1=True)
    frame = S.to_format(aln, values).cuda()
    a = _run_i8(c, frame, packed, 30.0)
    b = _run_i8(c._replace(inst=gen, route='knob'), frame, packed, 30.0)
    assert _lib.tune('X2_ALN') == 1 and torch.equal(a.view, b.view) and int(a.view.max()) > 10
    if fmt == S.FMT_U8:
        f16 = S.Inst('stem2x', 64, S.FMT_F16, 1, 1)
        d = _run_i8(c._replace(inst=f16), S.to_format(f16, values).cuda(), packed, 30.0)
        assert torch.equal(a.view, d.view)


# ------------------------------------------------------------------------------------------------ refused calls
def test_refused_calls_leave_the_buffer_untouched():
    pair, x2 = Q.PAIR_INSTANCES[1], Q.X2_INSTANCES[0]
    n, h, w = 1, 16, 128
    INVALID, UNSUPPORTED = -1, -4
    for inst in (pair, x2):
        packed = _packed(S.gauss_stages(inst, 1))
        frame = S.to_format(inst, S.gauss_values(inst, n, h, w, 1)).cuda()
        oh, ow = S.out_map(inst, h, w)
        buf = torch.full((n * oh * ow * 64 + 64,), Q.FILL, dtype=torch.int8, device='cuda')
        out = buf[:n * oh * ow * 64]
        assert _launch_i8(inst._replace(c=32), frame, packed, n, h, w, 1.0, out) == UNSUPPORTED          # a 32-channel stem
        assert _launch_i8(inst._replace(fmt=3), frame, packed, n, h, w, 1.0, out) == UNSUPPORTED         # no such frame format
        assert _launch_i8(inst, frame, packed, n, h, w, 1.0, buf[8:]) == INVALID                         # out 8 bytes past a 16-byte boundary
        assert _launch_i8(inst, frame, packed, 0, h, w, 1.0, out) == INVALID
        if inst.kernel == 'stem2x':
            f32 = S.to_format(inst._replace(fmt=S.FMT_F32), S.gauss_values(inst, n, h, w, 1)).cuda()
            assert _launch_i8(inst._replace(fmt=S.FMT_F32), f32, packed, n, h, w, 1.0, out) == UNSUPPORTED   # NCHW fp32 frames
        else:
            p = [ptr(x) for wb in packed for x in wb]
            assert lib().lfd_stem_conv_i8(ptr(frame), inst.fmt, n, h, w, 64, p[0], p[1], None, None, 1.0, ptr(out),
                                          stream_ptr()) == UNSUPPORTED                                    # without the 1x1 tail
        torch.cuda.synchronize()
        assert bool((buf == Q.FILL).all())
        assert _launch_i8(inst, frame, packed, n, h, w, 1.0, out) == 0                                   # the accepted call writes it all
        torch.cuda.synchronize()
        assert not bool((out == Q.FILL).any()) and bool((buf[-64:] == Q.FILL).all())


def test_knobs_are_back_at_their_defaults():
    for k, v in S.KNOB_DEFAULTS.items():
        assert _lib.tune(k) == v, 'knob %s left at %d' % (k, _lib.tune(k))
