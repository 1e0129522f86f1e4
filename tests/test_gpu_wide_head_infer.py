"""Heads with more than 64 output rows in the 'fp16' inference mode: lfd_head_forward_wide_f16 -- k_head2's output pass with three
and four tiles of final rows -- and the engine that calls it.

Kernel level, on the instrument of tests/golden/head_cases.py (cases: tests/golden/wide_head_cases.py; the gates and the walk
properties are checked on the CPU by tests/test_wide_head_infer_host.py), every k_head2 variant on every case:
  * bit for bit against the float64 chain on the integer instrument;
  * within the gates on Gaussian operands, every variant the same bits as the first;
  * guards, the rows between the levels and the outputs a tower does not have stay NaN (head_cases.Device.outputs);
  * argument validation without a launch.
End to end: COCO-sized WIDERFACE_LFD_S (80 classes, merged head) and TT100K_LFD_S (81 channels, separate towers on two streams)
against the oracles; 61 and 124 classes; the grayscale twin; determinism and graph replay; get_results on the engine's own logits; the 'fp32_storage'
route of the same model."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import head_cases as H
import wide_head_cases as W
from oracle import net_oracle
from lfd_amd import _lib, configs, engine

pytestmark = pytest.mark.gpu
NAMES = [c['name'] for c in W.CASES]


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


def _knobs_for(c, variant):
    kw = dict(H.VARIANTS[variant]['knobs'])
    if c['chunk']:
        kw['H2_CHUNK'] = c['chunk']
    return kw


@functools.lru_cache(maxsize=None)
def _ops(name, kind):
    return H.operands(W.BY_NAME[name], kind)


@functools.lru_cache(maxsize=None)
def _ref(name, kind):
    c, O = W.BY_NAME[name], _ops(name, kind)
    return H.chain(c, O, 'head', ab=O.get('ab'))


def _first_difference(c, key, got, ref):
    m = ~torch.isnan(ref)
    bad = ((got.double() != ref) & m).nonzero()
    if not len(bad):
        return '%s: unwritten / non-finite element' % key
    i, j, ch = bad[0].tolist()
    geo = H.geometry(c)
    l = max(k for k, po in enumerate(geo['p_off']) if po <= j)
    return '%s: %d elements differ from float64, first at image %d, level %d, pixel %d, channel %d' % (key, len(bad), i, l, j - geo['p_off'][l], ch)


# ------------------------------------------------------------------------------------------------ output pass, exact
@pytest.mark.parametrize('name', NAMES)
def test_wide_output_pass_equals_float64_on_integers(name):
    c, O, ref = W.BY_NAME[name], _ops(name, 'int'), _ref(name, 'int')
    bits = {}
    for v in W.VARIANTS:
        dev = W.WideDevice(c, O, v)
        dev.set_ab(O['ab'])
        with knobs(**_knobs_for(c, v)):
            if H.VARIANTS[v]['a1']:
                assert dev.forward(2) == 0          # leaves conv2's operands for the output pass
            assert dev.forward(3) == 0
        cls, reg = dev.outputs()                    # (guards, rows between the levels, outputs the tower does not have: NaN)
        for key, got in (('cls', cls), ('reg', reg)):
            assert H.equal(got, ref[key]), '%s / %s %s' % (name, v, _first_difference(c, key, got, ref[key]))
        for t in dev.x + dev.folded + dev.ab:
            t.get()
        bits[v] = (cls, reg)
    for a, b in zip(bits['fold_a1'], bits['fold']):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), 'fold_a1 and fold differ'


# ------------------------------------------------------------------------------------------------ the chain, Gaussian
@pytest.mark.parametrize('name', NAMES)
def test_five_launch_chain_with_the_wide_output_pass_on_gaussian_operands(name):
    c, O, ref = W.BY_NAME[name], _ops(name, 'gauss'), _ref(name, 'gauss')
    first = None
    for v in W.VARIANTS:
        dev = W.WideDevice(c, O, v)
        with knobs(**_knobs_for(c, v)):
            out = dev.chain()
        for k in ('partial1', 'ab1', 'partial2', 'ab2', 'cls', 'reg'):
            d, g = H.deviation(out[k], ref[k]), W.gate(name, k)
            print('%s / %s %s: deviation %.3e  gate %.3e' % (name, v, k, d, g))
            assert d <= g, '%s / %s %s: %.3e above the gate %.3e' % (name, v, k, d, g)
        if first is None:
            first = out
        for k in ('cls', 'reg'):      # every variant computes the same bits (fold_a1 those of fold among them)
            assert torch.equal(out[k].view(torch.int32), first[k].view(torch.int32)), '%s / %s: %s differs from the plain variant' % (name, v, k)


# ------------------------------------------------------------------------------------------------ argument validation
def test_wide_entry_argument_validation_without_a_launch():
    INVALID, UNSUPPORTED = -1, -4
    c, O = W.BY_NAME['w84'], _ops('w84', 'int')
    dev = W.WideDevice(c, O, 'plain')
    dev.set_ab(O['ab'])

    def desc(d0=dev.d, **kw):
        d = _lib.HeadDesc.from_buffer_copy(d0)
        for k, v in kw.items():
            setattr(d, k, v)
        return d

    def levels(**kw):
        lv = (_lib.HeadLevelPtrs * len(c['levels']))()
        C.memmove(lv, dev.lv, C.sizeof(lv))
        for k, v in kw.items():
            setattr(lv[1], k, v)
        return lv
    assert dev.forward(3, d=desc(final_cls_rows=60)) == UNSUPPORTED         # 64 rows: lfd_head_forward_f16 serves them
    assert dev.forward(3, d=desc(final_cls_rows=125, cls_channels=125)) == UNSUPPORTED      # 129 rows
    assert dev.forward(3, d=desc(num_groups=32)) == UNSUPPORTED             # groups of 4 channels: not a k_head2 case
    prev = _lib.tune('HEAD2', 0)
    try:
        assert dev.forward(3) == UNSUPPORTED
    finally:
        _lib.tune('HEAD2', prev)
    assert _lib.tune('HEAD2') == prev == H.KNOB_DEFAULTS['HEAD2']
    assert dev.forward(3, ab2=False) == INVALID
    assert dev.forward(3, lv=levels(wf_packed=None)) == INVALID
    assert dev.forward(3, d=desc(final_reg_rows=2)) == INVALID
    # the shared entry keeps refusing wide rows, and the wide one a narrow head
    assert H.Device.forward(dev, 3) == UNSUPPORTED
    torch.cuda.synchronize()
    for g in [dev.partial, dev.cls, dev.reg]:
        assert bool(torch.isnan(g.get(False)).all()), 'a rejected call wrote'
    assert dev.forward(3) == 0       # the unchanged arguments are fine
    dev.outputs()


# ------------------------------------------------------------------------------------------------ end to end
def _model(arch_or_name, num_classes=None):
    m = configs.build_model(arch_or_name, num_classes=num_classes)
    configs.perturb_weights(m)
    m.eval()
    return m, {k: v.clone() for k, v in m.state_dict().items()}


def _frames(shape, seed=3):
    return (torch.rand(shape[0], 3, shape[2], shape[3], generator=torch.Generator().manual_seed(seed)) * 2 - 1).half().float()


def _check_against_oracles(what, arch, sd, x, c, r):
    """the gates of tests/test_gpu_forward.py: the fp16-emulating oracle on the raw logits, the fp32 one on the scores"""
    with torch.no_grad():
        rc, rr, _ = net_oracle.lfd_forward_fp16(sd, arch, x)
        fc, fr, _ = net_oracle.lfd_forward(sd, arch, x)
    assert c.shape == rc.shape and r.shape == rr.shape
    ec, er = (c - rc).abs(), (r - rr).abs()
    ce = arch['classification_loss_type'] == 'CrossEntropyLoss'
    sc = (c.softmax(-1) - fc.softmax(-1)).abs().max() if ce else (c.sigmoid() - fc.sigmoid()).abs().max()
    sr = (r.sigmoid() - fr.sigmoid()).abs().max()
    print('%s: fp16 oracle max %.2e / %.2e  mean %.2e / %.2e; fp32 oracle scores %.2e / %.2e' % (what, ec.max(), er.max(), ec.mean(), er.mean(), sc, sr))
    assert float(ec.max()) < 1e-2 and float(er.max()) < 1e-2
    assert float(ec.mean()) < 1.5e-3 and float(er.mean()) < 1.5e-3
    assert float(sc) < 2.5e-3 and float(sr) < 2.5e-3


@functools.lru_cache(maxsize=None)
def _coco_s():
    """the 80-class WIDERFACE_LFD_S on the device, its frames and its logits (shared; nothing changes them)"""
    arch = dict(configs.ARCHS['WIDERFACE_LFD_S'], num_classes=80)
    m, sd = _model('WIDERFACE_LFD_S', 80)
    x = _frames((2, 3, 135, 241))
    m.cuda()
    with torch.no_grad():
        c, r = m(x.cuda())
    return arch, m, sd, x, c.clone(), r.clone()


def test_80_class_merged_head_runs_in_fp16_mode_and_matches_the_oracles():
    arch, m, sd, x, c, r = _coco_s()
    assert m.precision == 'fp16' and c.shape[2] == 80 and c.dtype == torch.float32
    # ... on the fused plan of engine.py (the layer-by-layer engine behind it is what `Unsupported` would select)
    assert m._fused_plan_ok(c.device)
    plan = engine.get_plan(m, m._backbone, m._neck, m._head, c.device)
    assert [(t.reg_rows, t.cls_rows) for t in plan.levels[0].towers] == [(4, 80)]
    _check_against_oracles('WIDERFACE_LFD_S x 80', arch, sd, x, c.cpu(), r.cpu())


def test_81_channel_separate_towers_on_two_streams(monkeypatch):
    arch = dict(configs.ARCHS['TT100K_LFD_S'], num_classes=80)
    x = _frames((1, 3, 64, 64))
    outs = []
    for flag in ('1', '0'):
        monkeypatch.setenv('LFD_TOWER_OVERLAP', flag)
        m, sd = _model(arch)
        m.cuda()
        with torch.no_grad():
            c, r = m(x.cuda())
        outs.append((c.clone(), r.clone()))
        torch.cuda.synchronize()
    c, r = outs[0]
    assert c.shape[2] == 81
    _check_against_oracles('TT100K_LFD_S x 80', arch, sd, x, c.cpu(), r.cpu())
    assert torch.equal(outs[1][0], c) and torch.equal(outs[1][1], r), 'the towers one after the other give other bits'


@pytest.mark.parametrize('classes', [61, 124])
def test_first_and_last_wide_class_count(classes):
    arch = dict(configs.ARCHS['WIDERFACE_LFD_S'], num_classes=classes)
    m, sd = _model('WIDERFACE_LFD_S', classes)
    x = _frames((1, 3, 96, 128))
    m.cuda()
    with torch.no_grad():
        c, r = m(x.cuda())
    P = sum(h * w for h, w in (m.head_indexes_to_feature_map_sizes[i] for i in range(len(arch['regression_ranges']))))
    assert tuple(c.shape) == (1, P, classes) and tuple(r.shape) == (1, P, 4)
    _check_against_oracles('WIDERFACE_LFD_S x %d' % classes, arch, sd, x, c.cpu(), r.cpu())


def test_gray_twin_of_the_80_class_model():
    """input_channels=1: the grayscale stem in front of the same plan and the same wide output pass"""
    arch = dict(configs.ARCHS['WIDERFACE_LFD_S'], num_classes=80)
    m = configs.build_model('WIDERFACE_LFD_S', input_channels=1, num_classes=80)
    configs.perturb_weights(m)
    m.eval()
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    x = (torch.rand(1, 1, 96, 128, generator=torch.Generator().manual_seed(3)) * 2 - 1).half().float()
    m.cuda()
    with torch.no_grad():
        c, r = m(x.cuda())
    assert m._fused_plan_ok(c.device) and c.shape[2] == 80
    _check_against_oracles('gray WIDERFACE_LFD_S x 80', arch, sd, x, c.cpu(), r.cpu())


def test_wide_head_is_deterministic_and_graph_replay_matches():
    arch, m, sd, x, c, r = _coco_s()
    xd = x.cuda()
    try:
        with torch.no_grad():
            a = [t.clone() for t in m(xd)]
            m.use_graph = True
            g = [t.clone() for t in m(xd)]
            h = [t.clone() for t in m(xd.clone())]
    finally:
        m.use_graph = False
    for got in (a, g, h):
        assert torch.equal(got[0], c) and torch.equal(got[1], r)


def test_get_results_of_the_80_class_model_equals_the_oracle_pipeline_on_its_logits():
    """decode + threshold + per-class NMS on the device against the oracle's on the very logits the engine produced: the same rows in
    the same order (scores: expf on the device against torch.sigmoid; boxes: the decode tolerance of the full-size parity tests)"""
    arch, m, sd, x, c, r = _coco_s()
    h, w = x.shape[2:]
    sizes = [tuple(m.head_indexes_to_feature_map_sizes[i]) for i in range(len(arch['regression_ranges']))]
    sc = c[0].sigmoid().cpu().numpy()
    thr = float(np.sort(sc.reshape(-1))[-1000])          # 999 candidates above it
    prev = m._classification_threshold
    m._classification_threshold = thr
    try:
        got = m.get_results((c[:1], r[:1]), [dict(resized_height=h, resized_width=w, resize_scale=1.0)])[0]
    finally:
        m._classification_threshold = prev
    dets, labels, _, K = net_oracle.get_results_single(c[0].cpu().numpy(), r[0].cpu().numpy(), sizes, net_oracle.strides_of(arch), arch, thr,
                                                       0.4, False, (h, w), 1.0)
    ref = net_oracle.pack_results(dets, labels)
    print('%d candidates, %d kept on the device, %d by the oracle, %d classes among them' % (K, len(got), len(ref), len(set(labels.tolist()))))
    assert 100 < K < 2000 and len(got) == len(ref) > 20 and len(set(labels.tolist())) > 10
    a, b = np.array(got, np.float64), np.array(ref, np.float64)
    assert np.array_equal(a[:, 0], b[:, 0]), 'labels differ row for row'
    assert np.abs(a[:, 1] - b[:, 1]).max() < 1e-6 + 2e-5 and np.abs(a[:, 2:] - b[:, 2:]).max() < 1e-3


def test_fp32_storage_route_of_the_80_class_model():
    arch = dict(configs.ARCHS['WIDERFACE_LFD_S'], num_classes=80)
    m, sd = _model('WIDERFACE_LFD_S', 80)
    x = _frames((1, 3, 96, 128))
    m.cuda()
    m.precision = 'fp32_storage'
    with torch.no_grad():
        c, r = m(x.cuda())
        rc, rr, _ = net_oracle.lfd_forward(sd, arch, x)
    err = max(float((c.cpu() - rc).abs().max()), float((r.cpu() - rr).abs().max()))
    print('fp32_storage, 80 classes: raw logits within %.2e of the fp32 oracle' % err)
    assert err < 1e-4
