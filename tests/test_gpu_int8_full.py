"""The fused='full' route of the INT8 deployment mode on the MI355X (build_int8_engine(..., fused='full'); csrc/entry_i8.hip,
DESIGN 4j) against the default layer-by-layer engine of the same model and the same calibration cache: cls / reg, every tap
buffer and every int8 map both routes write must be equal bit for bit, eager and under graph replay; the launch counts and the
route; no buffer for a map that stays on chip; caches written by one route serve the others.

Weights, frames and the calibration set are those of tests/test_gpu_int8_engine.py."""
import functools
import os
import tempfile

import pytest
import torch

from conftest import load_golden
from lfd_amd import INT8Calibrator, build_int8_engine, configs, deployment, engine_i8

pytestmark = pytest.mark.gpu

CASES = [('WIDERFACE_LFD_XS', 3), ('WIDERFACE_LFD_S', 3), ('TT100K_LFD_L', 3), ('WIDERFACE_LFD_S', 1)]
IDS = ['%s%s' % (n, '_gray' if c == 1 else '') for n, c in CASES]


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
    cache = os.path.join(tempfile.mkdtemp(prefix='lfd_int8full_'), 'calibration.json')
    data = torch.cat([x, extra]).numpy()
    plain = build_int8_engine(m, INT8Calibrator(data, cache, batch_size=1))
    assert plain.calibrated and os.path.exists(cache)
    blob = open(cache, 'rb').read()
    full = build_int8_engine(m, NoBatches(data, cache, batch_size=1), fused='full')      # from the cache the other route wrote
    assert open(cache, 'rb').read() == blob
    return dict(m=m, x=x.cuda(), plain=plain, full=full, cache=cache, data=data)


def _forward(eng, x):
    with torch.no_grad():
        cls, reg = eng.forward_resident(x)
    torch.cuda.synchronize()
    return cls, reg, eng.plan.state_for(*((x.shape[0], x.shape[2], x.shape[3]) if x.dtype != torch.uint8 else x.shape[:3]), 0)


def _compare(plain, full, x):
    """the 'full' engine against the default one on x: outputs, taps and every int8 map both write, eager and graphed"""
    pp, fp = plain.plan, full.plan
    cls0, reg0, st0 = _forward(plain, x)
    cls0, reg0 = cls0.clone(), reg0.clone()
    for graph in (False, True):
        full.use_graph = graph
        try:
            for _ in range(2 if graph else 1):                   # under use_graph: the capture, then a replay
                cls1, reg1, st1 = _forward(full, x)
        finally:
            full.use_graph = False
        assert torch.equal(cls1, cls0) and torch.equal(reg1, reg0), 'graph %s' % graph
        assert pp.taps == fp.taps and len(fp.taps) > 0
        for t in fp.taps:
            assert torch.equal(st1.bufs[t].view(torch.int16), st0.bufs[t].view(torch.int16)), 'tap buffer %d (graph %s)' % (t, graph)
        assert torch.equal(st1.bufs[fp.stage_in].view(torch.int16), st0.bufs[pp.stage_in].view(torch.int16))     # the fp16 stem map
        written = 0
        for c0, c1 in zip(pp.layers, fp.layers):
            assert (c0.dst, c0.cout_real) == (c1.dst, c1.cout_real)
            if c1.dst in fp.unwritten:                           # on chip only
                assert c1.dst not in st1.qbufs
                continue
            written += 1
            assert torch.equal(st1.qbufs[c1.dst], st0.qbufs[c0.dst]), '%s (graph %s)' % (c1.name, graph)
            assert bool((st1.qbufs[c1.dst][..., c1.cout_real:] == 0).all()), 'padded channels of %s' % c1.name
        assert written == len(fp.layers) - len(fp.unwritten - set([0])) > 0
        assert sorted(st1.qbufs) == sorted(set(fp.qbuf_channels) - fp.unwritten)       # no buffer for an unwritten map
        assert sorted(st0.qbufs) == sorted(pp.qbuf_channels)


@pytest.mark.parametrize('name,ch', CASES, ids=IDS)
def test_full_engine_equals_the_layer_by_layer_engine_bit_for_bit(name, ch):
    cs = _case(name, ch)
    plain, full = cs['plain'], cs['full']
    assert full.fused == 'full' and full.route == 'full' and plain.route == 'layers' and plain.fused is False
    assert not full.calibrated and full.scales == plain.scales
    assert full.plan.tensor_names == plain.plan.tensor_names
    assert [c.name for c in full.plan.layers] == [c.name for c in plain.plan.layers]
    _compare(plain, full, cs['x'])


def test_uint8_frames():
    """uint8 NHWC frames (the stem's fused normalisation) at a size whose maps are ragged against every tile"""
    cs = _case('WIDERFACE_LFD_XS', 3)
    img = torch.randint(0, 256, (1, 120, 168, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).cuda()
    _compare(cs['plain'], cs['full'], img)


@pytest.mark.parametrize('name,ch', CASES, ids=IDS)
def test_launch_counts_and_route(name, ch):
    cs = _case(name, ch)
    pp, fp = cs['plain'].plan, cs['full'].plan
    lay = pp.layers
    assert fp.launches == engine_i8.lower_fused(lay, entry=True) and pp.launches is None
    fused = engine_i8.lower_fused(lay)
    n_entry = [l.kind for l in fp.launches].count('entry')
    assert n_entry >= 2 and fp.int8_launches() == len(fp.launches) == len(fused) - n_entry and pp.int8_launches() == len(lay)
    if ch == 3:
        assert (fp.int8_launches(), len(fused), len(lay)) == {'WIDERFACE_LFD_S': (14, 17, 26), 'WIDERFACE_LFD_XS': (12, 15, 26),
                                                              'TT100K_LFD_L': (16, 18, 28)}[name]
    # the first entry launch reads the fp16 stem map: the quantise launch is gone and so is its buffer
    assert fp.entry_f16 == 0 and 0 in fp.unwritten and pp.entry_f16 is None
    assert cs['full'].route == 'full' and cs['plain'].route == 'layers'
    with pytest.raises(AttributeError):
        cs['full'].route = 'fused'                               # read-only
    with pytest.raises(ValueError):
        build_int8_engine(cs['m'], NoBatches(cs['data'], cs['cache'], batch_size=1), fused='all')


def test_a_cache_written_by_the_full_route_serves_the_others():
    cs = _case('WIDERFACE_LFD_XS', 3)
    cache = os.path.join(tempfile.mkdtemp(prefix='lfd_int8full_'), 'calibration.json')
    full = build_int8_engine(cs['m'], INT8Calibrator(cs['data'], cache, batch_size=1), fused='full')      # calibrates
    assert full.calibrated and full.route == 'full'
    assert open(cache, 'rb').read() == open(cs['cache'], 'rb').read()      # the calibration walk does not depend on the route
    assert full.scales == cs['plain'].scales
    engines = [build_int8_engine(cs['m'], NoBatches(cs['data'], cache, batch_size=1), fused=f) for f in (False, True)]
    assert [e.route for e in engines] == ['layers', 'fused'] and not any(e.calibrated for e in engines)
    cls0, reg0, _ = _forward(cs['plain'], cs['x'])
    cls0, reg0 = cls0.clone(), reg0.clone()
    for e in [full] + engines:
        cls1, reg1, _ = _forward(e, cs['x'])
        assert torch.equal(cls1, cls0) and torch.equal(reg1, reg0), e.route
