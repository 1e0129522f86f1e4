"""The 256-channel siblings end to end on the HIP path ('fp16' mode): configs.WIDE_SIBLINGS -- R18_FCOS_FPN256 (ResNet-18, FPN 256,
the class-default FCOSHead: four GroupNorm(32, 256) tower layers, 80 classes) and LFDV2_SFPN256 (SimpleFPN 256, LFDHead of 3x3
convs) -- on a 2 x 3 x 128 x 160 batch (the FCOS entry also on 1 x 3 x 101 x 150) against what the REFERENCE classes computed on
the CPU (tests/golden/wide_sibling_<case>.npz, tests/golden/make_golden_wide_siblings.py).

  (a) every conv launch of neck and head re-derived in float64 from the tensors it read: |got - ref| <= 0.5005 ulp16(ref) +
      2^-19 sum |x||w| (the fp32-output convs: the second term alone), on the route the engine takes at this size AND on the
      other one (the crossover constant moved); every GroupNorm launch by the tolerances of tests/test_gpu_train_norms.py;
  (b) each backbone tap and neck output against the reference's, max |err| / max |ref| <= 4 sqrt(2 L) 2^-11, L the conv layers
      in front of it (the random-walk bound of tests/test_gpu_resnet.py);
  (c) sigma(cls), sigma(reg) (sigma(centerness)) against the reference: see SIGMA_MEASURED;
  (d) graph replay, frame formats, detect / detect_resident and get_results on top; fp32_storage keeps refusing."""
import functools
import hashlib
import json
import math
import os

import numpy as np
import pytest
import torch

import conv_cases as CC
import make_golden_wide_siblings as MG
import norm_cases as NC
import resnet_cases as RC
from test_sibling_oracle_golden import assert_results_equal
from lfd_amd import configs, engine, engine_sibling, ops

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = [(n, '') for n in configs.WIDE_SIBLINGS] + [('R18_FCOS_FPN256', '_odd')]
# sigma(cls) / sigma(reg) / sigma(centerness) against the fixtures as measured on the MI355X.  Every case is
# <= 2.0e-3, so the gate is the fp16 mode's stated 2.5e-3 envelope.
SIGMA_MEASURED = {'R18_FCOS_FPN256': (1.67e-3, 5.39e-4, 5.22e-4), 'R18_FCOS_FPN256_odd': (1.39e-3, 4.49e-4, 3.71e-4),
                  'LFDV2_SFPN256': (3.88e-4, 3.47e-4)}
SIGMA_GATE = 2.5e-3


def _state_sha(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def _model(name):
    m = configs.build_wide_sibling_model(name)
    m.eval()
    m.cuda()
    return m


@functools.lru_cache(maxsize=None)
def _case(name, suffix=''):
    """the model on the GPU (weights checked against the fixture's sha256), the fixture, the input, one forward's outputs"""
    gold = np.load(os.path.join(GOLDEN, 'wide_sibling_%s%s.npz' % (name, suffix)))
    m = _model(name)
    assert _state_sha(m.state_dict()) == str(gold['sha']), 'the weights are not the ones the fixture was made with'
    x = MG.frame(tuple(int(v) for v in gold['shape']), int(gold['x_seed'])).cuda()
    with torch.no_grad():
        outs = [o.clone() for o in m(x)]
    torch.cuda.synchronize()
    return dict(model=m, gold=gold, x=x, outs=outs)


def _plan(m, dev):
    return engine_sibling.get_plan(m, m._backbone, m._neck, m._head, dev)


# ------------------------------------------------------------------------------------------------ (a) every launch
def _record_launches(m, x, monkeypatch):
    """-> [(layer, (conv, norm), input clone, output clone)] of every _Conv call of one forward of a freshly built plan"""
    sources, calls = {}, []
    init, call = engine_sibling._Conv.__init__, engine_sibling._Conv.__call__

    def rec_init(self, conv, norm, relu, cin_have, dev, f32out=False):
        init(self, conv, norm, relu, cin_have, dev, f32out=f32out)
        sources[id(self)] = (conv, norm)

    def rec_call(self, xin):
        xc = xin.clone()
        y = call(self, xin)
        calls.append((self, sources[id(self)], xc, y.clone()))
        return y

    monkeypatch.setattr(engine_sibling._Conv, '__init__', rec_init)
    monkeypatch.setattr(engine_sibling._Conv, '__call__', rec_call)
    with torch.no_grad():
        plan = engine_sibling.SiblingPlan(m._backbone, m._neck, m._head, x.device)
        outs = plan.run_head(plan.run_neck(engine_sibling.backbone_taps(plan, x)))
    torch.cuda.synchronize()
    monkeypatch.setattr(engine_sibling._Conv, '__call__', call)
    return plan, calls, outs


def _conv_alone(layer, xin, pixels_say):
    """the conv launch of `layer` without its GroupNorm, on the route it takes at `pixels_say` pixels"""
    r = layer.route(pixels_say)
    relu = layer.relu and layer.gn is None
    if r == 'conv256_f32':
        return r, ops.conv256_nhwc(xin, layer.w, layer.b, layer.cout, layer.ks, relu=False, f32out=True)
    if r == 'conv256':
        return r, ops.conv256_nhwc(xin, layer.w, layer.b, layer.cout, layer.ks, relu=relu)
    assert r == 'conv_wide'
    return r, ops.conv2d_nhwc(xin, layer.w, layer.b, layer.cin, layer.cout, layer.ks, layer.stride, relu)


@pytest.mark.parametrize('name', list(configs.WIDE_SIBLINGS))
def test_every_neck_and_head_launch_rederived_in_float64(name, monkeypatch):
    cs = _case(name)
    m, x = cs['model'], cs['x']
    dev = x.device
    plan, calls, outs = _record_launches(m, x, monkeypatch)
    assert all(torch.equal(a, b) for a, b in zip([o for o in outs[:3] if o is not None], cs['outs']))
    worst, routes, ngn = [], {}, 0
    for layer, (conv, norm), xin, got in calls:
        bn = norm if isinstance(norm, torch.nn.BatchNorm2d) else None
        wf, bf = engine._fold_conv_norm(conv, bn)
        wt = torch.zeros((layer.cout, layer.cin, layer.ks, layer.ks), dtype=torch.float64, device=dev)
        wt[:wf.shape[0], :wf.shape[1]] = wf.to(dev).half().double()
        b = torch.zeros(layer.cout, dtype=torch.float64, device=dev)
        b[:bf.shape[0]] = bf.to(dev).double()
        ref = CC.conv_ref(xin, wt, b, layer.stride)
        mag = CC.conv_ref(xin.abs(), wt.abs(), b.abs(), layer.stride)
        if layer.relu and layer.gn is None:
            ref = ref.relu()
        pixels = ref.shape[0] * ref.shape[1] * ref.shape[2]
        tag = '%dx%d s%d %d->%d @%dx%d' % (layer.ks, layer.ks, layer.stride, layer.cin, layer.cout, ref.shape[1], ref.shape[2])
        ys = {}
        for say in (pixels, engine_sibling.CONV256_MIN_PIXELS if pixels < engine_sibling.CONV256_MIN_PIXELS else 1):
            r, y = _conv_alone(layer, xin, say)
            ys[r] = y
            tol = 2.0 ** -19 * mag if layer.f32out else 0.5005 * RC.ulp16(ref) + 2.0 ** -19 * mag
            err = (y.double() - ref).abs()
            ratio = float(torch.where(err == 0, torch.zeros_like(err), err / tol).nan_to_num(float('inf')).max())   # (0 <= 0)
            worst.append((ratio, r + ' ' + tag))
            routes[r] = routes.get(r, 0) + 1
            assert ratio <= 1.0, (tag, r, ratio)
        y = ys[layer.route(pixels)]
        assert not bool(y[..., layer.cout_real:].any()), 'padded channels stay zero'
        if layer.gn is None:
            assert torch.equal(y, got), tag
            continue
        # ---- the GroupNorm launches on that conv output
        ngn += 1
        n, h, w, c = y.shape
        g = layer.gn.num_groups
        stats = ops.gn_train_stats(y, g, layer.gn.eps)
        z = ops.gn_train_apply(y, g, stats, layer.gamma, layer.beta, relu=layer.relu)
        assert torch.equal(z, got), tag
        y3 = y.reshape(n, h * w, c).cpu()
        sref = NC.gn_forward_ref(y3, [h * w], g, eps=layer.gn.eps)
        st = NC.gn_stats_view(stats.cpu(), n, 1, g)
        torch.testing.assert_close(st[:, :, 0], sref[:, :, 0], rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(st[:, :, 1], sref[:, :, 1], rtol=1e-5, atol=0)
        zref, operands = NC.gn_apply_ref(y3, [h * w], g, st, layer.gamma.cpu(), layer.beta.cpu(), layer.relu)
        err = (z.reshape(n, h * w, c).cpu().double() - zref).abs()
        assert bool((err <= NC.store_bound(zref, operands)).all()), 'GroupNorm ' + tag
    print('LAUNCHES %s: %d conv calls (%s), %d GroupNorm; worst conv error over tolerance %.3f (%s)'
          % ((name, len(calls), ' '.join('%s %d' % kv for kv in sorted(routes.items())), ngn) + max(worst)))
    assert routes.get('conv256', 0) > 0 and routes.get('conv_wide', 0) > 0 and routes.get('conv256_f32', 0) > 0 and ngn > 0


# ------------------------------------------------------------------------------------------------ (b), (c) the reference
def _sampled(t_nhwc, steps, channels):
    cs, s = int(steps[0]), int(steps[1])
    return t_nhwc.float().cpu().permute(0, 3, 1, 2)[:, :channels][:, ::cs, ::s, ::s]


@pytest.mark.parametrize('name,suffix', CASES)
def test_outputs_taps_and_neck_against_the_reference(name, suffix):
    cs = _case(name, suffix)
    m, gold, x, outs = cs['model'], cs['gold'], cs['x'], cs['outs']
    nl = len(gold['sizes'])
    assert [tuple(m.head_indexes_to_feature_map_sizes[i]) for i in range(nl)] == [tuple(s) for s in gold['sizes'].tolist()]
    assert [tuple(o.shape) for o in outs] == [tuple(gold[k].shape) for k in ('cls', 'reg', 'ctr')[:len(outs)]]
    plan = _plan(m, x.device)
    with torch.no_grad():
        taps = [t.clone() for t in engine_sibling.backbone_taps(plan, x)]
        feats = plan.run_neck(engine_sibling.backbone_taps(plan, x))
    nbb = sum(isinstance(mod, torch.nn.Conv2d) for mod in m._backbone.modules())       # >= the conv layers in front of any tap
    rel, bounds = [], []
    for tag, maps, depth in (('tap', taps, lambda i: nbb), ('neck', feats, lambda i: nbb + 2 + max(0, i - len(taps) + 1))):
        assert len(maps) == len(gold[tag + '_shapes'])
        for i, t in enumerate(maps):
            real = int(gold[tag + '_shapes'][i][1])
            assert tuple(t.shape[1:3]) == tuple(gold[tag + '_shapes'][i][2:])
            ref = torch.from_numpy(gold['%s%d' % (tag, i)])
            got = _sampled(t, gold[tag + '_steps'][i], real)
            assert got.shape == ref.shape
            rel.append(float((got - ref).abs().max() / ref.abs().max()))
            bounds.append(4 * math.sqrt(2 * depth(i)) * 2.0 ** -11)
            assert not bool(t[..., real:].any()), 'padded channels stay zero'
    sig = [float((o.cpu().sigmoid() - torch.from_numpy(gold[k]).sigmoid()).abs().max()) for o, k in zip(outs, ('cls', 'reg', 'ctr'))]
    print('WIDE %s%s: sigma(cls, reg[, ctr]) %s; taps + neck max |err| / max |ref|: %s (bounds %s)'
          % (name, suffix, ' '.join('%.2e' % v for v in sig), ' '.join('%.1e' % r for r in rel), ' '.join('%.1e' % b for b in bounds)))
    assert all(r <= b for r, b in zip(rel, bounds))
    assert max(sig) <= SIGMA_GATE


# ------------------------------------------------------------------------------------------------ (d) the entry points
@pytest.mark.parametrize('name,suffix', CASES)
def test_frame_formats_and_graph_replay_agree(name, suffix):
    cs = _case(name, suffix)
    m, x, outs = cs['model'], cs['x'], cs['outs']
    with torch.no_grad():
        x16 = x.permute(0, 2, 3, 1).half().contiguous()       # the frame's values are fp16 numbers: the same operand
        assert all(torch.equal(a, b) for a, b in zip(m(x16), outs))
        m.use_graph = True
        try:
            first = [t.clone() for t in m(x)]
            again = [t.clone() for t in m(x)]                 # the second call replays
        finally:
            m.use_graph = False
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(outs, first, again))


def test_detect_resident_returns_the_rows_of_detect_of_forward():
    cs = _case('LFDV2_SFPN256')
    m, x = cs['model'], cs['x']
    meta = torch.tensor([[160., 128., 1.0]] * 2, device='cuda')
    with torch.no_grad():
        sc = cs['outs'][0].sigmoid().flatten()
        thr = float(sc.kthvalue(max(sc.numel() - 150, 1)).values)
        want = m.detect(m.forward(x), meta, thr, 0.4)
        wd, wc = want.dets.clone(), want.counts.clone()
        for graph in (False, True):
            m.use_graph = graph
            try:
                out = m.detect_resident(x, meta, score_thr=thr, iou_thr=0.4)
                torch.cuda.synchronize()
            finally:
                m.use_graph = False
            assert torch.equal(out.counts, wc)
            for i in range(2):
                k = int(wc[i, 1])
                assert k > 0 and torch.equal(out.dets[i, :k], wd[i, :k])


def test_fcos_detect_of_forward_runs_on_80_classes():
    cs = _case('R18_FCOS_FPN256')
    m, x = cs['model'], cs['x']
    meta = torch.tensor([[160., 128., 1.0]] * 2, device='cuda')
    with torch.no_grad():
        sc = (cs['outs'][0].sigmoid() * cs['outs'][2].sigmoid()).flatten()
        thr = float(sc.kthvalue(max(sc.numel() - 150, 1)).values)
        out = m.detect(m.forward(x), meta, thr, 0.4)
    assert int(out.counts[:, 1].min()) > 0


@pytest.mark.parametrize('name,suffix', CASES)
def test_get_results_on_reference_logits_equals_reference_results(name, suffix):
    """the existing sibling matching rule (tests/test_gpu_siblings.py): the reference's own logits through the device
    post-processing reproduce the reference's get_results rows"""
    cs = _case(name, suffix)
    m, g = cs['model'], cs['gold']
    n, H, W = [int(v) for v in g['shape']]
    old = (m._classification_threshold, m._nms_cfg)
    m._classification_threshold = float(g['results_thr'])
    m._nms_cfg = dict(type='nms', iou_thr=float(g['results_iou']))
    try:
        for i, hw in enumerate(g['sizes'].tolist()):
            m._head_indexes_to_feature_map_sizes[i] = tuple(hw)
        preds = tuple(torch.from_numpy(g[k]).cuda() for k in ('cls', 'reg', 'ctr') if k in g.files)
        for key, (hh, ww, sc) in (('results', (H, W, 1.0)), ('results_scaled', (H - 6, W - 10, 0.5))):
            res = m.get_results(preds, [dict(resized_height=hh, resized_width=ww, resize_scale=sc)] * n)
            ref = json.loads(str(g[key]))
            assert sum(len(r) for r in ref) > 3
            for i in range(n):
                assert_results_equal(res[i], ref[i])
        # and on the device's own logits it runs
        res = m.get_results(tuple(cs['outs']), [dict(resized_height=H, resized_width=W, resize_scale=1.0)] * n)
        assert len(res) == n and all(len(r) > 0 and len(r[0]) == 6 for r in res)
    finally:
        m._classification_threshold, m._nms_cfg = old


@pytest.mark.parametrize('name', list(configs.WIDE_SIBLINGS))
def test_fp32_storage_mode_is_refused_and_fp16_keeps_its_bits(name):
    cs = _case(name)
    m = cs['model']
    m.precision = 'fp32_storage'
    try:
        with pytest.raises(engine.Unsupported, match='more than 128 output channels|fp32-tensor kernel'):
            with torch.no_grad():
                m(cs['x'])
    finally:
        m.precision = 'fp16'
    with torch.no_grad():
        outs = m(cs['x'])
    assert all(torch.equal(a, b) for a, b in zip(outs, cs['outs']))
