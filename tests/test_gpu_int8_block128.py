"""The block128 option of the INT8 deployment mode on the MI355X (build_int8_engine(..., fused=True | 'full', block128=True);
csrc/block128_i8.hip) against the default layer-by-layer engine of the same model and the same calibration cache:
cls / reg, every tap buffer and every int8 map both routes write must be equal bit for bit, eager and under graph replay; the
launch lists, the route, which stays what it was, and engine.block128; no buffer for a map that stays on chip.

Weights, frames and the calibration set are those of tests/test_gpu_int8_engine.py."""
import functools
import os
import tempfile

import pytest
import torch

from conftest import load_golden
from lfd_amd import INT8Calibrator, build_int8_engine, configs, deployment, engine_i8

pytestmark = pytest.mark.gpu

CASES = [('WIDERFACE_LFD_S', 3), ('TT100K_LFD_L', 3), ('TL_LFD_L', 3), ('WIDERFACE_LFD_S', 1), ('WIDERFACE_LFD_XS', 3)]
IDS = ['%s%s' % (n, '_gray' if c == 1 else '') for n, c in CASES]
ROUTES = [(True, 'fused'), ('full', 'full')]


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
    cache = os.path.join(tempfile.mkdtemp(prefix='lfd_int8b128_'), 'calibration.json')
    data = torch.cat([x, extra]).numpy()
    plain = build_int8_engine(m, INT8Calibrator(data, cache, batch_size=1))
    assert plain.calibrated and os.path.exists(cache)
    blob = open(cache, 'rb').read()
    # from the cache the default route wrote
    opts = dict((route, build_int8_engine(m, NoBatches(data, cache, batch_size=1), fused=fused, block128=True))
                for fused, route in ROUTES)
    assert open(cache, 'rb').read() == blob
    return dict(m=m, x=x.cuda(), plain=plain, opts=opts, cache=cache, data=data)


def _forward(eng, x):
    with torch.no_grad():
        cls, reg = eng.forward_resident(x)
    torch.cuda.synchronize()
    return cls, reg, eng.plan.state_for(x.shape[0], x.shape[2], x.shape[3], 0)


def _compare(plain, opt, x):
    """the block128 engine against the default one on x: outputs, taps and every int8 map both write, eager and graphed"""
    pp, fp = plain.plan, opt.plan
    cls0, reg0, st0 = _forward(plain, x)
    cls0, reg0 = cls0.clone(), reg0.clone()
    for graph in (False, True):
        opt.use_graph = graph
        try:
            for _ in range(2 if graph else 1):                   # under use_graph: the capture, then a replay
                cls1, reg1, st1 = _forward(opt, x)
        finally:
            opt.use_graph = False
        assert torch.equal(cls1, cls0) and torch.equal(reg1, reg0), 'graph %s' % graph
        assert pp.taps == fp.taps and len(fp.taps) > 0
        for t in fp.taps:
            assert torch.equal(st1.bufs[t].view(torch.int16), st0.bufs[t].view(torch.int16)), 'tap buffer %d (graph %s)' % (t, graph)
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


@pytest.mark.parametrize('fused,route', ROUTES, ids=[r for _, r in ROUTES])
@pytest.mark.parametrize('name,ch', CASES[:4], ids=IDS[:4])
def test_block128_engine_equals_the_layer_by_layer_engine_bit_for_bit(name, ch, fused, route):
    cs = _case(name, ch)
    plain, opt = cs['plain'], cs['opts'][route]
    assert opt.block128 is True and plain.block128 is False
    assert opt.route == route and opt.fused == fused and plain.route == 'layers'          # the route is what it was
    with pytest.raises(AttributeError):
        opt.block128 = False                                     # read-only
    assert not opt.calibrated and opt.scales == plain.scales
    assert opt.plan.tensor_names == plain.plan.tensor_names
    assert [c.name for c in opt.plan.layers] == [c.name for c in plain.plan.layers]
    la = opt.plan.launches
    n128 = [l.kind for l in la].count('block128')
    assert la == engine_i8.lower_fused(plain.plan.layers, entry=route == 'full', block128=True)
    assert n128 == {'WIDERFACE_LFD_S': 2, 'TT100K_LFD_L': 2, 'TL_LFD_L': 3}[name]
    assert opt.plan.int8_launches() == len(engine_i8.lower_fused(plain.plan.layers, entry=route == 'full')) - n128
    # conv1's map of every 'block128' launch stays on chip
    assert all(opt.plan.layers[l.layers[0]].dst in opt.plan.unwritten for l in la if l.kind == 'block128')
    _compare(plain, opt, cs['x'])


def test_a_model_without_an_eligible_block_gets_the_same_launch_list():
    cs = _case('WIDERFACE_LFD_XS', 3)
    lay = cs['plain'].plan.layers
    for fused, route in ROUTES:
        opt = cs['opts'][route]
        assert opt.block128 is True and opt.route == route
        assert opt.plan.launches == engine_i8.lower_fused(lay, entry=route == 'full')
        assert 'block128' not in [l.kind for l in opt.plan.launches]
    _compare(cs['plain'], cs['opts']['full'], cs['x'])


def test_block128_needs_a_fused_route():
    cs = _case('WIDERFACE_LFD_S', 3)
    with pytest.raises(ValueError):
        build_int8_engine(cs['m'], NoBatches(cs['data'], cs['cache'], batch_size=1), block128=True)
    with pytest.raises(ValueError):
        build_int8_engine(cs['m'], NoBatches(cs['data'], cs['cache'], batch_size=1), fused=False, block128=True)
    with pytest.raises(ValueError):
        build_int8_engine(cs['m'], NoBatches(cs['data'], cs['cache'], batch_size=1), fused='all', block128=True)
