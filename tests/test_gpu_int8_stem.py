"""The stem_int8 option of the INT8 deployment mode on the MI355X (build_int8_engine(..., stem_int8=True); lfd_stem_conv_i8 in
csrc/stem.hip, lfd_stem_faster_fused_i8 in csrc/stem_fused.hip) against the default layer-by-layer engine of the same
model and the same calibration cache, under every route: cls / reg, every tap buffer, int8 buffer 0 and every other int8 map both
engines write must be equal bit for bit, eager and under graph capture plus a replay; the plan's record shows that no quantise
launch ran and that the first entry launch of the 'full' route read int8; scales, names and the cache are unchanged; models and
frame formats without an int8 stem run the launches they run without the option.

Weights, frames and the calibration set are those of tests/test_gpu_int8_full.py."""
import functools
import os
import tempfile

import pytest
import torch

from conftest import load_golden
from lfd_amd import INT8Calibrator, build_int8_engine, configs, deployment

pytestmark = pytest.mark.gpu

ELIGIBLE = [('TT100K_LFD_L', 3), ('WIDERFACE_LFD_S', 3), ('TL_LFD_L', 3)]            # part (a), part (b), part (a)
INELIGIBLE = [('WIDERFACE_LFD_XS', 3), ('WIDERFACE_LFD_S', 1)]
ROUTES = [(False, False), (True, False), ('full', False), ('full', True)]            # (fused, block128)
ROUTE_IDS = ['layers', 'fused', 'full', 'full_block128']
FORMATS = {'TT100K_LFD_L': frozenset([0, 1, 2]), 'TL_LFD_L': frozenset([0, 1, 2]), 'WIDERFACE_LFD_S': frozenset([1, 2]),
           'WIDERFACE_LFD_XS': frozenset()}
STEM_ENTRY = {'TT100K_LFD_L': 'lfd_stem_conv_i8', 'TL_LFD_L': 'lfd_stem_conv_i8', 'WIDERFACE_LFD_S': 'lfd_stem_faster_fused_i8'}


class NoBatches(INT8Calibrator):
    def get_batch(self, names=None, p_str=None):
        raise AssertionError('the cache was there: no calibration batch may be asked for')


@functools.lru_cache(maxsize=None)
def _case(name, ch):
    g = load_golden(('ref_model_gray_%s.npz' if ch == 1 else 'ref_model_%s.npz') % name)
    m = configs.build_model(name, seed=666, input_channels=ch)
    configs.perturb_weights(m, seed=1)
    m.eval()
    assert deployment.state_sha256(m.state_dict()) == str(g['sha'])
    n, h, w = [int(v) for v in g['shape']]
    x = torch.rand(n, ch, h, w, generator=torch.Generator().manual_seed(int(g['x_seed']))) * 2 - 1
    extra = torch.rand(4, ch, h, w, generator=torch.Generator().manual_seed(1234)) * 2 - 1
    m.cuda()
    cache = os.path.join(tempfile.mkdtemp(prefix='lfd_int8stem_'), 'calibration.json')
    data = torch.cat([x, extra]).numpy()
    plain = build_int8_engine(m, INT8Calibrator(data, cache, batch_size=1))        # the default engine writes the cache
    assert plain.calibrated and os.path.exists(cache) and plain.stem_int8 is False
    blob = open(cache, 'rb').read()
    x = x.cuda()
    frames = {0: x, 1: x.permute(0, 2, 3, 1).half().contiguous(),
              2: torch.randint(0, 256, (n, h, w, ch), dtype=torch.uint8, generator=torch.Generator().manual_seed(7)).cuda()}
    return dict(m=m, frames=frames, plain=plain, cache=cache, data=data, blob=blob, engines={})


def _engine(cs, fused, block128, stem_int8=True):
    """built from the cache the default engine wrote, with a calibrator that refuses to give batches"""
    key = (fused, block128, stem_int8)
    if key not in cs['engines']:
        e = build_int8_engine(cs['m'], NoBatches(cs['data'], cs['cache'], batch_size=1), fused=fused, block128=block128,
                              stem_int8=stem_int8)
        assert not e.calibrated and open(cs['cache'], 'rb').read() == cs['blob']
        cs['engines'][key] = e
    return cs['engines'][key]


def _forward(eng, x, slot=0):
    with torch.no_grad():
        cls, reg = eng.forward_resident(x, slot)
    torch.cuda.synchronize()
    return cls, reg, eng.plan.state_for(*((x.shape[0], x.shape[2], x.shape[3]) if x.dtype != torch.uint8 and x.dtype != torch.float16
                                          else x.shape[:3]), slot)


def _fmt(x):
    return {torch.float32: 0, torch.float16: 1, torch.uint8: 2}[x.dtype]


def _check_record(eng, x):
    """the plan's own record of the launches in front of the stages"""
    p, front = eng.plan, eng.plan.front
    if _fmt(x) in p.stem_int8_formats:
        assert front['stem'] in ('lfd_stem_conv_i8', 'lfd_stem_faster_fused_i8') and front['quantise'] is False
        assert front['entry_in_format'] == (0 if p.route == 'full' else None)
    else:                                                        # today's launches
        assert front['stem'] == 'fp16' and front['quantise'] is (p.entry_f16 is None)
        assert front['entry_in_format'] == (1 if p.route == 'full' else None)


def _compare(ref, eng, x):
    """eng against the engine ref on x: outputs, taps and every int8 map both write, eager and graphed"""
    rp, ep = ref.plan, eng.plan
    cls0, reg0, st0 = _forward(ref, x)
    cls0, reg0 = cls0.clone(), reg0.clone()
    for graph in (False, True):
        eng.use_graph = graph
        try:
            for _ in range(2 if graph else 1):                   # under use_graph: the capture, then a replay
                cls1, reg1, st1 = _forward(eng, x)
        finally:
            eng.use_graph = False
        _check_record(eng, x)
        assert torch.equal(cls1, cls0) and torch.equal(reg1, reg0), 'graph %s' % graph
        assert rp.taps == ep.taps and len(ep.taps) > 0
        for t in ep.taps:
            assert torch.equal(st1.bufs[t].view(torch.int16), st0.bufs[t].view(torch.int16)), 'tap buffer %d (graph %s)' % (t, graph)
        both = sorted(set(st0.qbufs) & set(st1.qbufs))
        assert sorted(st1.qbufs) == sorted(set(ep.qbuf_channels) - ep.unwritten) and len(both) >= 3
        assert (0 in both) == (0 not in rp.unwritten and 0 not in ep.unwritten)
        if _fmt(x) not in ep.stem_int8_formats and ep.entry_f16 is not None:
            both = [b for b in both if b != 0]                   # allocated for the other formats, not written by this call
        for b in both:
            assert torch.equal(st1.qbufs[b], st0.qbufs[b]), 'int8 map %d (graph %s)' % (b, graph)
        if 0 in both:
            assert bool((st1.qbufs[0][..., ep.stem_channels_real:] == 0).all())       # padded stem channels quantise to 0


@pytest.mark.parametrize('fused,block128', ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize('name,ch', ELIGIBLE, ids=[n for n, _ in ELIGIBLE])
def test_stem_int8_engine_equals_the_default_engine_bit_for_bit(name, ch, fused, block128):
    cs = _case(name, ch)
    plain, eng = cs['plain'], _engine(cs, fused, block128)
    assert eng.stem_int8 is True and eng.plan.stem_int8 is True and eng.plan.stem_int8_formats == FORMATS[name]
    assert eng.scales == plain.scales and eng.plan.tensor_names == plain.plan.tensor_names
    assert eng.plan.inv_stem_scale == plain.plan.inv_stem_scale
    assert [c.name for c in eng.plan.layers] == [c.name for c in plain.plan.layers]
    off = _engine(cs, fused, block128, stem_int8=False)
    assert eng.plan.launches == off.plan.launches and eng.plan.int8_launches() == off.plan.int8_launches()
    assert eng.plan.tap_ready_after == off.plan.tap_ready_after and 0 not in eng.plan.unwritten
    for fmt in (1, 2, 0):                                        # NHWC fp16, NHWC uint8, NCHW fp32 (eligible behind a 'fast' stem)
        x = cs['frames'][fmt]
        _compare(plain, eng, x)
        if fmt in eng.plan.stem_int8_formats:
            assert eng.plan.front['stem'] == STEM_ENTRY[name]
    assert open(cs['cache'], 'rb').read() == cs['blob']


@pytest.mark.parametrize('name', ['TT100K_LFD_L', 'WIDERFACE_LFD_S'])
def test_uint8_frames_at_a_ragged_shape(name):
    """uint8 NHWC frames at a size whose maps are ragged against every tile; a shape that only ever sees an eligible format keeps
    no fp16 stem map"""
    cs = _case(name, 3)
    eng = _engine(cs, 'full', True)
    img = torch.randint(0, 256, (1, 120, 168, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).cuda()
    _compare(cs['plain'], eng, img)
    st = eng.plan.state_for(1, 120, 168, 0)
    assert eng.plan.stage_in not in st.bufs and st.qbufs[0].shape[3] == 64
    assert cs['plain'].plan.stage_in in cs['plain'].plan.state_for(1, 120, 168, 0).bufs       # the default engines keep theirs


@pytest.mark.parametrize('fused', [True, 'full'], ids=['fused', 'full'])
def test_eligible_and_ineligible_formats_at_one_shape_under_graph_capture(fused):
    """WIDERFACE_LFD_S: NHWC fp16 frames take the int8 stem, NCHW fp32 frames the two-kernel fp16 stem.  One engine, one shape,
    use_graph: each format replays its own graph"""
    cs = _case('WIDERFACE_LFD_S', 3)
    plain, eng = cs['plain'], _engine(cs, fused, False)
    xs = [cs['frames'][1], cs['frames'][0], cs['frames'][1], cs['frames'][0], cs['frames'][2]]
    want = []
    for x in xs:
        c, r, _ = _forward(plain, x)
        want.append((c.clone(), r.clone()))
    eng.use_graph = True
    try:
        for x, (c0, r0) in zip(xs, want):
            c1, r1, st = _forward(eng, x)
            assert torch.equal(c1, c0) and torch.equal(r1, r0), _fmt(x)
        assert sorted(k[1] for k in st.graph) == [0, 1, 2]       # one graph per (buffer, frame format)
    finally:
        eng.use_graph = False
    # the fp32 call allocated the fp16 stem map on first use; eagerly it runs today's launches
    assert eng.plan.stage_in in st.bufs
    _forward(eng, cs['frames'][0])
    _check_record(eng, cs['frames'][0])
    assert eng.plan.front['stem'] == 'fp16'


@pytest.mark.parametrize('name,ch', INELIGIBLE, ids=['WIDERFACE_LFD_XS', 'WIDERFACE_LFD_S_gray'])
def test_models_without_an_int8_stem_run_todays_launches(name, ch):
    cs = _case(name, ch)
    for fused, block128 in ((False, False), ('full', False)):
        on, off = _engine(cs, fused, block128), _engine(cs, fused, block128, stem_int8=False)
        assert on.stem_int8 is True and on.plan.stem_int8_formats == frozenset() and on.plan.unwritten == off.plan.unwritten
        assert on.plan.launches == off.plan.launches and on.scales == off.scales == cs['plain'].scales
        for fmt in (0, 1):
            x = cs['frames'][fmt]
            _compare(off, on, x)
            assert on.plan.front == off.plan.front and on.plan.front['stem'] == 'fp16'
            st = on.plan.state_for(x.shape[0], *(x.shape[2:] if fmt == 0 else x.shape[1:3]), 0)
            assert on.plan.stage_in in st.bufs
        c0, r0, _ = _forward(cs['plain'], cs['frames'][0])
        c0, r0 = c0.clone(), r0.clone()
        c1, r1, _ = _forward(on, cs['frames'][0])
        assert torch.equal(c1, c0) and torch.equal(r1, r0)


def test_option_values():
    cs = _case('WIDERFACE_LFD_XS', 3)
    import numpy
    for bad in (1, 0, 'yes', numpy.bool_(True)):
        with pytest.raises(ValueError):
            build_int8_engine(cs['m'], NoBatches(cs['data'], cs['cache'], batch_size=1), stem_int8=bad)
    with pytest.raises(AttributeError):
        cs['plain'].stem_int8 = True                             # read-only
