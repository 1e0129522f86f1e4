"""The fused route of the INT8 deployment mode on the MI355X (build_int8_engine(..., fused=True); csrc/block_i8.hip, csrc/conv_i8.hip)
against the default layer-by-layer engine of the same model and the same calibration cache: cls / reg, every tap buffer and every
int8 map both routes write must be equal bit for bit, eager and under graph replay; the launch counts; the default untouched.

Weights, frames and the calibration set are those of tests/test_gpu_int8_engine.py."""
import functools
import os
import tempfile

import numpy as np
import pytest
import torch

from conftest import load_golden
from lfd_amd import INT8Calibrator, build_int8_engine, configs, deployment, engine_i8

pytestmark = pytest.mark.gpu

CASES = [('WIDERFACE_LFD_S', 3), ('WIDERFACE_LFD_XS', 3), ('TT100K_LFD_L', 3), ('WIDERFACE_LFD_S', 1), ('TL_LFD_S', 3)]
IDS = ['%s%s' % (n, '_gray' if c == 1 else '') for n, c in CASES]
# int8 launches of the stages per forward (the quantise launch not counted): fused, layer by layer
LAUNCHES = {'WIDERFACE_LFD_S': (17, 26), 'WIDERFACE_LFD_XS': (15, 26), 'TT100K_LFD_L': (18, 28)}


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
    seed = int(g['x_seed'])
    x = torch.rand(n, ch, h, w, generator=torch.Generator().manual_seed(seed)) * 2 - 1
    extra = torch.rand(4, ch, h, w, generator=torch.Generator().manual_seed(1234)) * 2 - 1
    m.cuda()
    cache = os.path.join(tempfile.mkdtemp(prefix='lfd_int8f_'), 'calibration.json')
    data = torch.cat([x, extra]).numpy()
    plain = build_int8_engine(m, INT8Calibrator(data, cache, batch_size=1))
    assert plain.calibrated and os.path.exists(cache)
    blob = open(cache, 'rb').read()
    fused = build_int8_engine(m, NoBatches(data, cache, batch_size=1), fused=True)       # from the cache the other route wrote
    assert open(cache, 'rb').read() == blob
    return dict(m=m, x=x.cuda(), plain=plain, fused=fused, cache=cache, data=data)


def _forward(eng, x):
    with torch.no_grad():
        cls, reg = eng.forward_resident(x)
    torch.cuda.synchronize()
    return cls, reg, eng.plan.state_for(x.shape[0], x.shape[2], x.shape[3], 0)


@pytest.mark.parametrize('name,ch', CASES, ids=IDS)
def test_fused_engine_equals_the_layer_by_layer_engine_bit_for_bit(name, ch):
    cs = _case(name, ch)
    plain, fused, x = cs['plain'], cs['fused'], cs['x']
    assert fused.fused and not plain.fused and not fused.calibrated and fused.scales == plain.scales
    pp, fp = plain.plan, fused.plan
    assert fp.tensor_names == pp.tensor_names and [c.name for c in fp.layers] == [c.name for c in pp.layers]
    cls0, reg0, st0 = _forward(plain, x)
    cls0, reg0 = cls0.clone(), reg0.clone()
    for graph in (False, True):
        fused.use_graph = graph
        try:
            for _ in range(2 if graph else 1):                   # under use_graph: the capture, then a replay
                cls1, reg1, st1 = _forward(fused, x)
        finally:
            fused.use_graph = False
        assert torch.equal(cls1, cls0) and torch.equal(reg1, reg0), 'graph %s' % graph
        assert pp.taps == fp.taps and len(fp.taps) > 0
        for t in fp.taps:
            assert torch.equal(st1.bufs[t].view(torch.int16), st0.bufs[t].view(torch.int16)), 'tap buffer %d (graph %s)' % (t, graph)
        written = 0
        for c0, c1 in zip(pp.layers, fp.layers):
            assert (c0.dst, c0.cout_real) == (c1.dst, c1.cout_real)
            if c1.dst in fp.unwritten:                           # the map between a fused block's convs: on chip only
                assert c1.dst not in st1.qbufs
                continue
            written += 1
            assert torch.equal(st1.qbufs[c1.dst], st0.qbufs[c0.dst]), '%s (graph %s)' % (c1.name, graph)
            assert bool((st1.qbufs[c1.dst][..., c1.cout_real:] == 0).all()), 'padded channels of %s' % c1.name
            if c1.tap is not None:
                assert bool((st1.bufs[c1.tap][..., c1.cout_real:] == 0).all()), 'padded tap channels of %s' % c1.name
        assert torch.equal(st1.qbufs[0], st0.qbufs[0])
        # every block output is among the maps compared
        assert written == len(fp.layers) - len(fp.unwritten) and len(fp.unwritten) == [l.kind for l in fp.launches].count('block')
    assert any(l.kind == 'block' for l in fp.launches) and any(l.kind == 'pair' for l in fp.launches)


@pytest.mark.parametrize('name,ch', CASES[:4], ids=IDS[:4])
def test_launch_counts(name, ch):
    cs = _case(name, ch)
    n_fused, n_plain = LAUNCHES[name]
    assert cs['fused'].plan.int8_launches() == len(cs['fused'].plan.launches) == n_fused
    assert cs['plain'].plan.int8_launches() == len(cs['plain'].plan.layers) == n_plain and cs['plain'].plan.launches is None
    assert cs['fused'].plan.launches == engine_i8.lower_fused(cs['plain'].plan.layers)


@pytest.mark.parametrize('name,ch', [CASES[0], CASES[2]], ids=[IDS[0], IDS[2]])
def test_detect_and_get_results_rows_are_equal(name, ch):
    cs = _case(name, ch)
    plain, fused, m, x = cs['plain'], cs['fused'], cs['m'], cs['x']
    n, h, w = x.shape[0], x.shape[2], x.shape[3]
    meta_rows = [dict(resized_height=h, resized_width=w, resize_scale=1.0)] * n
    meta = torch.tensor([[float(w), float(h), 1.0]] * n, device='cuda')
    with torch.no_grad():
        cls = plain(x)[0]
    old = m._classification_threshold
    m._classification_threshold = float(np.quantile((cls.sigmoid() if cls.shape[2] == 1 else cls.softmax(-1)[..., :-1]).cpu().numpy(), 0.9))
    try:
        with torch.no_grad():
            d0 = plain.detect(x, meta)
            counts0, dets0, labels0 = d0.counts.clone(), d0.dets.clone(), d0.labels.clone()   # (the model's buffers serve both engines)
            d1 = fused.detect(x, meta)
            assert torch.equal(d1.counts, counts0)
            for i in range(n):                                   # rows behind the kept count (column 1) are not written
                k = int(counts0[i, 1])
                assert torch.equal(d1.dets[i, :k], dets0[i, :k]) and torch.equal(d1.labels[i, :k], labels0[i, :k])
            assert int(counts0[:, 1].sum()) > 0
            rows0 = plain.get_results(plain(x), meta_rows)
            rows1 = fused.get_results(fused(x), meta_rows)
    finally:
        m._classification_threshold = old
    assert rows0 == rows1 and sum(len(r) for r in rows1) > 0


def test_the_default_is_layer_by_layer_and_its_plan_is_untouched():
    cs = _case(*CASES[1])
    eng = build_int8_engine(cs['m'], NoBatches(cs['data'], cs['cache'], batch_size=1))
    assert eng.fused is False and eng.plan.launches is None and eng.plan.unwritten == frozenset()
    with pytest.raises(AttributeError):
        eng.fused = True                                         # read-only
    st = eng.plan.state_for(1, 64, 64, 'probe')
    assert sorted(st.qbufs) == sorted(eng.plan.qbuf_channels)    # every int8 map has its buffer
    assert eng.plan.tap_ready_after == cs['plain'].plan.tap_ready_after
    fp = cs['fused'].plan
    stf = fp.state_for(1, 64, 64, 'probe')
    assert sorted(stf.qbufs) == sorted(set(fp.qbuf_channels) - fp.unwritten) and len(fp.unwritten) > 0
