"""The fp16 stem kernels -- k_stem (csrc/stem.hip), k_stem_fused and k_stem2x (csrc/stem_fused.hip) and the fp16 form of
k_stem_gray (csrc/stem_gray.hip) -- against the float64 reference of tests/golden/stem_cases.py: all 12 + 6 + 4 + 12 instances,
at shapes that walk the persistent tile loops (6240 tiles on 2048 workgroups, 1044 on 512 / 256, 4200 on 256 with and without
the start-up stagger) and at the edges (one pixel, exactly one tile, one pixel past it either way, nine tiles, a frame whose
whole intermediate is smaller than one halo region).

On INTEGER operands (stem_cases.py: the instrument) the kernel must equal the reference bit for bit: every assertion on them is
torch.equal.  The output is a NaN-filled view in the middle of a sentinel-filled buffer, one map row of guard on either side:
no NaN may be left and the guards must stay untouched.  uint8 frames of the bytes {0, 255} must give the bits of the -1 / +1
fp16 frames.  On Gaussian operands the gates are the existing ones (1.2e-3 for a pair, 4e-3 for the four-conv chain).
tests/test_stem_reference_host.py shows, without a GPU, which wrong references these comparisons reject and which error (a
skipped intermediate rounding) the integer operands cannot see.

Every knob change goes through `knobs`, which restores the previous value; the last test finds the three knobs at their defaults."""
import contextlib

import pytest
import torch

import stem_cases as S
from lfd_amd import _lib, engine, ops
from lfd_amd._lib import check, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu

SENTINEL = -12344.0            # an fp16 value no case produces (|outputs| <= 2048)


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
    """the output [n, oh, ow, c], NaN-filled, in the middle of a sentinel-filled buffer: one map row of guard on each side"""

    def __init__(self, shape):
        n = shape[0] * shape[1] * shape[2] * shape[3]
        self.guard = shape[2] * shape[3]
        assert (self.guard * 2) % 16 == 0
        self.buf = torch.full((n + 2 * self.guard,), SENTINEL, dtype=torch.float16, device='cuda')
        self.view = self.buf[self.guard:self.guard + n].view(shape)
        self.view.fill_(float('nan'))
        assert self.view.data_ptr() % 16 == 0

    def untouched(self):
        g = self.guard
        return bool((self.buf[:g] == SENTINEL).all()) and bool((self.buf[-g:] == SENTINEL).all())


def _packed(inst, stages):
    """-> [(packed filter, bias)] on the device, in the layouts the entry points take"""
    first = engine.pack_stem_gray_weight if inst.kernel == 'gray' else engine.pack_stem_weight
    return [((first(w) if k == 0 else ops.pack_conv_weight(w)).cuda(), b.cuda()) for k, (w, b, _) in enumerate(stages)]


def _device_frame(inst, values, route):
    """the frame in the instance's format on the device; route 'misaligned': at a base 2 bytes past a 16-byte boundary"""
    t = S.to_format(inst, values).cuda()
    if route == 'misaligned':
        assert t.dtype == torch.float16
        buf = torch.zeros(t.numel() + 64, dtype=torch.float16, device='cuda')
        m = buf[1:1 + t.numel()].view_as(t)
        m.copy_(t)
        assert m.data_ptr() % 16 == 2
        return m, buf
    assert t.data_ptr() % 16 == 0
    return t, t


def _launch(inst, frame, packed, n, h, w, out):
    p = [x for wb in packed for x in wb]
    if inst.kernel in ('stem', 'gray'):
        fn = lib().lfd_stem_conv_f16 if inst.kernel == 'stem' else lib().lfd_stem_gray_f16
        w2, b2 = (p[2], p[3]) if inst.tail else (None, None)
        check(fn(ptr(frame), inst.fmt, n, h, w, inst.c, ptr(p[0]), ptr(p[1]), ptr(w2), ptr(b2), ptr(out), stream_ptr()), S.inst_id(inst))
    else:
        check(lib().lfd_stem_faster_fused_f16(ptr(frame), inst.fmt, n, h, w, inst.c, ptr(p[0]), ptr(p[1]), ptr(p[2]), ptr(p[3]), ptr(p[4]),
                                              ptr(p[5]), ptr(p[6]), ptr(p[7]), ptr(out), stream_ptr()), S.inst_id(inst))
    torch.cuda.synchronize()


def _run(c, values, stages, inst=None):
    """runs the case's entry point on `values` (NHWC float, CPU) under the case's knobs -> (Guarded output, values on the device)"""
    inst = inst or c.inst
    frame, keep = _device_frame(inst, values, c.route)
    packed = _packed(inst, stages)
    g = Guarded((c.n,) + S.out_map(inst, c.h, c.w) + (inst.c,))
    with knobs(**_case_knobs(c._replace(inst=inst))):
        _launch(inst, frame, packed, c.n, c.h, c.w, g.view)
    del keep
    return g


def _explain(c, got, ref):
    """where an integer comparison failed: the count, the first wrong element as tile / row / column, the workgroup iteration"""
    bad = (got != ref).nonzero()
    geo = S.tile_geometry(c.inst)
    lc = S.launch(c.inst, c.n, c.h, c.w)
    where = {t: (b, k) for b, tiles in enumerate(S.tile_walk(c.inst, lc)) for k, t in enumerate(tiles)}
    img, oy, ox, ch = bad[0].tolist()

    def tile_of(i, y, x):
        return int(i * lc.tiles_x * lc.tiles_y + (y // geo.TH) * lc.tiles_x + x // geo.TW)
    t = tile_of(img, oy, ox)
    tiles = sorted({tile_of(i, y, x) for i, y, x, _ in bad[:4096].tolist()})
    return ('%s: %d of %d elements differ (%d NaN); first at image %d pixel (%d, %d) channel %d: got %s, reference %s; tile %d = tile row %d, '
            'tile column %d of its image (row %d, column %d inside the tile) = iteration %d of workgroup %d; iterations of the first wrong tiles: %s'
            % (S.case_id(c), bad.size(0), ref.numel(), int(torch.isnan(got).sum()), img, oy, ox, ch, float(got[img, oy, ox, ch]),
               float(ref[img, oy, ox, ch]), t, (oy // geo.TH), ox // geo.TW, oy % geo.TH, ox % geo.TW, where[t][1], where[t][0],
               [where[k][1] for k in tiles[:16]]))


def _assert_exact(c, g, ref64):
    ref = ref64.float().half()
    assert float(ref64.abs().max()) <= S.F16_EXACT
    got = g.view
    assert got.shape == ref.shape
    assert torch.equal(got, ref), _explain(c, got, ref)
    assert not bool(torch.isnan(got).any()), 'unwritten output'
    assert g.untouched(), 'written outside the output'


def _reference(values, stages):
    return S.ref_in_chunks(values.cuda(), stages)


# ------------------------------------------------------------------------------------------------ the walks
@pytest.mark.parametrize('c', S.all_walk_cases(), ids=S.case_id)
def test_walk_case_is_exact_on_integer_operands(c):
    """every instance on its walk shapes: equal to the float64 reference, no NaN left, the guards untouched, the same bits on a
    second run"""
    values, stages = S.case_int_operands(c)
    g = _run(c, values, stages)
    ref = _reference(values, stages)
    _assert_exact(c, g, ref)
    del ref
    again = _run(c, values, stages)
    assert torch.equal(again.view, g.view)


@pytest.mark.parametrize('inst', S.INSTANCES, ids=S.inst_id)
def test_edge_cases_are_exact_on_integer_operands(inst):
    """one pixel, 2 x 2, exactly one tile from an odd and from an even frame, one pixel past a tile either way, nine tiles, two
    frames of four tiles, (1, 8, 8), (1, 19, 24) and for the fused kernels 3 x 5"""
    for c in S.edge_cases(inst):
        values, stages = S.case_int_operands(c)
        g = _run(c, values, stages)
        _assert_exact(c, g, _reference(values, stages))


# ------------------------------------------------------------------------------------------------ uint8 == -1 / +1 fp16
@pytest.mark.parametrize('inst', [i for i in S.INSTANCES if i.fmt == S.FMT_U8], ids=S.inst_id)
def test_uint8_frames_give_the_bits_of_their_fp16_frames(inst):
    """frames of the bytes {0, 255} through the uint8 instance == the same frames as -1 / +1 fp16 through the fp16 instance
    (and as fp32 NCHW where the kernel takes it), on the walk shape and on the edges"""
    for c in S.walk_cases(inst)[:1] + S.edge_cases(inst):
        values, stages = S.case_int_operands(c)
        assert bool((values.abs() == 1).all())
        a = _run(c, values, stages)
        others = [S.FMT_F16] + ([S.FMT_F32] if inst.kernel != 'stem2x' else [])
        for fmt in others:
            b = _run(c, values, stages, inst=inst._replace(fmt=fmt))
            assert not bool(torch.isnan(a.view).any()) and torch.equal(a.view, b.view), (S.case_id(c), S.FMT_NAMES[fmt])


# ------------------------------------------------------------------------------------------------ Gaussian operands
GAUSS_INSTANCES = [S.Inst('stem', 64, 1, 1, 0), S.Inst('gray', 64, 1, 1, 0), S.Inst('fused', 64, 1, 1, 0), S.Inst('fused', 32, 1, 1, 0),
                   S.Inst('stem2x', 64, 1, 1, 1)]


@pytest.mark.parametrize('c', [c for i in GAUSS_INSTANCES for c in S.walk_cases(i) if c.kind != 'c'], ids=S.case_id)
def test_walk_case_passes_the_gate_on_gaussian_operands(c):
    """the distribution of the existing tolerance tests on the walk shapes, one fp16 instance per kernel (both k_stem_fused
    widths: the 64-channel one has no other test): 1.2e-3 * max(|ref|, 1) for a pair, 4e-3 * max(|ref|, 1) for the chain"""
    values, stages = S.case_gauss_operands(c)
    g = _run(c, values, stages)
    ref = _reference(values, stages)
    gate = S.GAUSS_GATE_PAIR if len(stages) == 2 else S.GAUSS_GATE_CHAIN
    assert not bool(torch.isnan(g.view).any()) and g.untouched()
    ratio = float(((g.view.double() - ref).abs() / (gate * ref.abs().clamp(min=1.0))).max())
    lc = S.launch(c.inst, c.n, c.h, c.w)
    print('GATE %s ntiles=%d blocks=%d worst_error_over_gate=%.3f' % (S.case_id(c), lc.ntiles, lc.blocks, ratio))
    assert ratio <= 1.0


# ------------------------------------------------------------------------------------------------ knobs
def test_knobs_are_back_at_their_defaults():
    with pytest.raises(RuntimeError):
        with knobs(STEM2X=0, X2_ALN=0, X2_STAGGER=1):
            assert _lib.tune('STEM2X') == 0 and _lib.tune('X2_ALN') == 0 and _lib.tune('X2_STAGGER') == 1
            raise RuntimeError('a failing test')
    for k, v in S.KNOB_DEFAULTS.items():
        assert _lib.tune(k) == v, 'knob %s left at %d' % (k, _lib.tune(k))
