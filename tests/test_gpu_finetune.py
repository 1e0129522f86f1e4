"""Fine-tuning on the all-HIP training path: LFDResNet(frozen_stages=k, norm_eval=True) models.

1. the kernels of csrc/train_bn_eval.hip against the float64 references of tests/golden/norm_eval_cases.py (per element, bounds
   derived there from the number formats and the launch geometry; every output starts as NaN bit patterns, as in
   tests/test_gpu_train_norms.py);
2. one teacher-forced training iteration of frozen / norm_eval models against the fp32 autograd route (LFD_HIP_TRAIN=0) with the
   project's teacher-forced gates, and the exact conditions of freezing: no gradient, no update, no statistics update;
3. GraphedTrainStep on such a model, bit for bit against the eager train_step;
4. an unfrozen model still runs the launches it ran before."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import norm_cases as NC
import norm_eval_cases as NE
import train_step_cases as cases
from lfd_amd import configs, ops, optim, train, train_engine

pytestmark = pytest.mark.gpu

INV = 1.0 / NC.LOSS_SCALE


@pytest.fixture
def nan_filled_outputs(monkeypatch):
    real_empty, real_like = torch.empty, torch.empty_like

    def poison(t):
        if t.is_cuda and t.dtype.is_floating_point:
            t.fill_(float('nan'))
        elif t.is_cuda and t.dtype == torch.uint8:
            t.fill_(0xFF)             # 0xFFFFFFFF is an fp32 NaN
        return t
    monkeypatch.setattr(torch, 'empty', lambda *a, **k: poison(real_empty(*a, **k)))
    monkeypatch.setattr(torch, 'empty_like', lambda *a, **k: poison(real_like(*a, **k)))
    ops.train_workspace(torch.device('cuda', torch.cuda.current_device())).fill_(0xFF)
    yield


def _within(got, ref, bound, what, keep=None):
    """per element; a NaN anywhere fails.  keep: bool mask of the elements that are compared"""
    got = got.detach().double().cpu().reshape(ref.shape)
    err = (got - ref).abs()
    bad = ~(err <= bound)
    if keep is not None:
        bad &= keep
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound).nan_to_num(float('inf'))
    print('%s: max |err| / bound = %.3g over %d elements' % (what, float(ratio.max()), err.numel()))
    assert not bool(bad.any()), '%s: %d of %d elements outside the bound (worst |err| / bound %.3g)' % (
        what, int(bad.sum()), bad.numel(), float(ratio.max()))


def _norm_module(c, rm, rv):
    bn = nn.BatchNorm2d(c, eps=NC.EPS).cuda().eval()
    with torch.no_grad():
        bn.running_mean.copy_(rm)
        bn.running_var.copy_(rv)
    return bn


# ------------------------------------------------------------------------------------------------ 1. statistics rows, fold
@pytest.mark.parametrize('name', [t[0] for t in NE.STATS_TABLES])
def test_eval_statistics_rows_from_the_running_statistics(name, nan_filled_outputs):
    widths = dict(NE.STATS_TABLES)[name]
    inputs = NE.stats_inputs(name)
    norms = [_norm_module(c, rm, rv) for c, (rm, rv) in zip(widths, inputs)]
    batch = ops.BnEvalRows(norms)
    rows, fresh = batch.run()                  # the whole table in one launch
    assert fresh and len(rows) == len(norms)
    for c, (rm, rv), row in zip(widths, inputs, rows):
        got = row.cpu()
        assert got.shape == (2 * c,)
        mean, rstd = NE.eval_stats_ref(rm, rv)
        assert torch.equal(got[:c], rm), '%s c=%d: mean is not the running mean, bit for bit' % (name, c)
        assert bool(torch.isfinite(got[c:]).all())
        torch.testing.assert_close(got[c:].double(), rstd, rtol=1e-5, atol=0)          # (_stat_close's gate for rstd)
    # cached by the buffers' version counters; the buffers themselves are never written
    assert batch.run()[1] is False
    norms[-1].running_var.mul_(4.0)
    rows2, fresh = batch.run()
    assert fresh and rows2[-1].data_ptr() == rows[-1].data_ptr()
    c = widths[-1]
    torch.testing.assert_close(rows2[-1][c:].double().cpu(), NE.eval_stats_ref(inputs[-1][0], inputs[-1][1] * 4.0)[1], rtol=1e-5, atol=0)
    for bn, (rm, _) in zip(norms, inputs):
        assert torch.equal(bn.running_mean.cpu(), rm) and int(bn.num_batches_tracked) == 0


def test_frozen_conv_and_eval_norm_fold_into_one_conv_with_bias(nan_filled_outputs):
    """lfd_conv_bn_eval_fold_f32 for several units in one launch: w' = w * gamma * rstd, b' = beta - mean * gamma * rstd, fp32 with
    two roundings (w') / three (b') of u32 relative to the magnitudes involved (bounds: 4 u32)"""
    shapes = [(64, 64, 3), (32, 32, 1), (128, 64, 3), (64, 32, 1)]
    g = torch.Generator().manual_seed(17)
    items, host = [], []
    norms = [_norm_module(co, *NC.running_stats(co, 400 + i)) for i, (co, _, _) in enumerate(shapes)]
    rows = ops.BnEvalRows(norms).run()[0]
    for i, ((co, ci, ks), row) in enumerate(zip(shapes, rows)):
        w = torch.randn(co, ci, ks, ks, generator=g) * 0.1
        gamma, beta = NC.norm_params(co, 400 + i)
        items.append((w.cuda(), gamma.cuda(), beta.cuda(), row))
        host.append((w, gamma, beta, row.cpu()))
    fb = ops.FoldBatch(items)
    packed, biases = fb.run(True)
    for (w, gamma, beta, row), wo, bo, pk in zip(host, fb.w_outs, biases, packed):
        mean, rstd = NC.split_stats(row)
        a = gamma.double() * rstd
        wref = w.double() * a.view(-1, 1, 1, 1)
        bref = beta.double() - mean * a
        _within(wo, wref, 4 * NC.U32 * wref.abs(), 'folded weight')
        _within(bo, bref, 4 * NC.U32 * (beta.double().abs() + (mean * a).abs()), 'folded bias')
        assert torch.equal(pk, ops.pack_conv_weight_train(wo))          # the batched pack of the folded weights
    # relu(conv(x, w') + b') against conv -> eval BatchNorm -> ReLU in fp32 on the fp16 input
    (w, gamma, beta, row), (co, ci, ks) = host[0], shapes[0]
    x = NC.rand16((2, 9, 11, ci), 3)
    z = ops.conv2d_nhwc(x.cuda(), packed[0], biases[0], ci, co, ks, 1, True)
    mean, rstd = NC.split_stats(row)
    yref = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), None, 1, ks // 2)
    zref = torch.relu((yref - mean.view(1, -1, 1, 1)) * (rstd * gamma.double()).view(1, -1, 1, 1) + beta.double().view(1, -1, 1, 1))
    torch.testing.assert_close(z.permute(0, 3, 1, 2).double().cpu(), zref, rtol=4e-3, atol=4e-3)     # fp16 weights and output


# ------------------------------------------------------------------------------------------------ 1. the one-pass backward
@pytest.mark.parametrize('name', [c[0] for c in NE.BWD_CASES])
def test_eval_backward_per_element_against_float64(name, nan_filled_outputs):
    d = NE.bwd_inputs(name)
    c, mode = d['c'], d['mode']
    flat = lambda t: None if t is None else t.reshape(-1, c)
    cu = lambda t: None if t is None else t.cuda()
    bn = _norm_module(c, d['running_mean'], d['running_var'])
    stats = ops.BnEvalRows([bn]).run()[0][0]
    st = stats.cpu()
    y, gamma, beta, res = cu(d['y']), cu(d['gamma']), cu(d['beta']), cu(d['res'])
    relu = mode != 'none'
    z = ops.bn_train_apply(y, stats, gamma, beta, res, relu)           # the forward of an eval-norm unit
    zref, operands, _, _ = NC.bn_apply_ref(flat(d['y']), st, d['gamma'], d['beta'], flat(d['res']), relu)
    _within(z, zref, NC.store_bound(zref, operands), name + ' z')
    mask, und = NE.mask_of(d, st, z.cpu())
    n_und = int(und.sum())
    print('%s: %d of %d recomputed masks undecided' % (name, n_und, und.numel()))
    assert n_und == 0 or und.numel() >= NE.UNDECIDED_FREE_BELOW
    assert n_und <= NE.UNDECIDED_FRACTION * sum(int(np.prod(s)) for _, s, _, _ in NE.BWD_CASES)
    r = NE.bn_eval_backward_ref(flat(d['dz']), flat(d['y']), mask, st, d['gamma'], INV)
    if d['accumulate']:
        dg, db = torch.full((c,), NE.PREV_DGAMMA, device='cuda'), torch.full((c,), NE.PREV_DBETA, device='cuda')
        pg, pb = NE.PREV_DGAMMA, NE.PREV_DBETA
    else:
        dg, db = torch.full((c,), float('nan'), device='cuda'), torch.full((c,), float('nan'), device='cuda')
        pg = pb = None
    dy, g = ops.bn_eval_backward(cu(d['dz']), y, z if mode in ('z', 'res') else None, stats, gamma, INV, dg, db, want_g=mode == 'res',
                                 accumulate=d['accumulate'], relu=relu, beta=beta)
    bounds = NE.bn_eval_backward_bounds(r, NE.chain_of(d), INV, pg, pb)
    # an undecided element may go either way in dy; in the sums it may add or leave out its own term
    extra0 = (flat(d['dz']).double().abs() * und).sum(0) * INV
    extra1 = (flat(d['dz']).double().abs() * r['xh'].abs() * und).sum(0) * INV
    _within(dy, r['dy'], bounds[0], name + ' dy', keep=~und)
    _within(dg, r['dgamma'] + (pg or 0.0), bounds[1] + extra1, name + ' dgamma')
    _within(db, r['dbeta'] + (pb or 0.0), bounds[2] + extra0, name + ' dbeta')
    if mode == 'res':                   # the residual branch's gradient: dz where the ReLU passed, exactly
        assert torch.equal(flat(g.cpu()).double(), r['g'])
    else:
        assert g is None
    # deterministic
    dg2, db2 = torch.zeros(c, device='cuda'), torch.zeros(c, device='cuda')
    dg3, db3 = torch.zeros(c, device='cuda'), torch.zeros(c, device='cuda')
    a = ops.bn_eval_backward(cu(d['dz']), y, z if mode in ('z', 'res') else None, stats, gamma, INV, dg2, db2, relu=relu, beta=beta)[0]
    b = ops.bn_eval_backward(cu(d['dz']), y, z if mode in ('z', 'res') else None, stats, gamma, INV, dg3, db3, relu=relu, beta=beta)[0]
    assert torch.equal(a.view(torch.int16), b.view(torch.int16)) and torch.equal(dg2, dg3) and torch.equal(db2, db3)


def test_eval_entry_points_return_status_codes():
    from lfd_amd import _lib
    L = _lib.lib()
    p, s = _lib.ptr, _lib.stream_ptr()
    dev = torch.device('cuda')
    y = torch.zeros(2, 4, 4, 64, dtype=torch.float16, device=dev)
    st, ga, dg, db = torch.ones(128, device=dev), torch.ones(64, device=dev), torch.zeros(64, device=dev), torch.zeros(64, device=dev)
    dy = torch.empty_like(y)
    ws = ops.train_workspace(dev)
    INVALID, WS = -1, -2
    ok = (p(y), p(y), None, 0, 32, 64, p(st), p(ga), p(ga), 1.0, 0, p(ws), ws.numel(), p(dg), p(db), p(dy), None)
    assert L.lfd_bn_eval_bwd_f16(*ok, s) == 0
    for i, v, want in ((0, None, INVALID), (1, None, INVALID), (6, None, INVALID), (7, None, INVALID), (15, None, INVALID),
                       (4, 0, INVALID), (5, 48, INVALID), (5, 512, INVALID), (5, 4, INVALID), (12, 1024, WS), (11, None, INVALID)):
        args = list(ok)
        args[i] = v
        assert L.lfd_bn_eval_bwd_f16(*args, s) == want, (i, v)
    args = list(ok)
    args[3], args[8] = 1, None                  # ReLU mask recomputed from y needs beta
    assert L.lfd_bn_eval_bwd_f16(*args, s) == INVALID
    assert L.lfd_bn_eval_stats_f32(None, 1, 64, s) == INVALID and L.lfd_bn_eval_stats_f32(None, 0, 64, s) == 0
    assert L.lfd_bn_eval_stats_f32(None, -1, 64, s) == INVALID
    assert L.lfd_conv_bn_eval_fold_f32(None, 1, 64, s) == INVALID and L.lfd_conv_bn_eval_fold_f32(None, 0, 0, s) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 2. one teacher-forced iteration
def _model(name, cin=3, **kw):
    m = configs.build_model(name, input_channels=cin, **kw)
    configs.perturb_weights(m, seed=1)
    return m.train()


class _Recorder(object):
    """ops' view of the library with every entry point it fetches appended to `calls`"""

    def __init__(self, real, calls):
        self._real, self._calls = real, calls

    def __getattr__(self, name):
        self._calls.append(name)
        return getattr(self._real(), name)


def _xs_stages():
    return len(configs.build_model('WIDERFACE_LFD_XS')._backbone._body_architecture)


ITERATION_CASES = [
    ('WIDERFACE_LFD_XS', 3, dict(frozen_stages=1)),
    ('WIDERFACE_LFD_XS', 3, dict(frozen_stages=2)),
    ('WIDERFACE_LFD_XS', 3, dict(norm_eval=True)),
    ('WIDERFACE_LFD_XS', 3, dict(frozen_stages=1, norm_eval=True)),
    ('WIDERFACE_LFD_XS', 3, dict(frozen_stages='all')),
    ('WIDERFACE_LFD_XS', 1, dict(frozen_stages=1)),
    ('TL_LFD_L', 3, dict(frozen_stages=1)),
]


@pytest.mark.parametrize('arch,cin,kw', ITERATION_CASES, ids=['%s-c%d-%s' % (a, c, '-'.join('%s=%s' % kv for kv in k.items()))
                                                            for a, c, k in ITERATION_CASES])
def test_one_teacher_forced_iteration_against_the_fp32_route(arch, cin, kw, monkeypatch):
    """Route A = fp32 autograd (LFD_HIP_TRAIN=0, convolutions without MIOpen as in test_gpu_gray_train), route B = the HIP path,
    both from identical state on the (2, C, 96, 128) batch: loss 1 %, gradient norm 3 %, 1 - cosine of the trainable parameters'
    gradient <= 0.02, training-mode running statistics 1 %.  Exactly: frozen parameters have no gradient and keep their bits
    through the optimizer step; eval-mode norms keep running_mean, running_var and num_batches_tracked."""
    monkeypatch.setattr(torch.backends.cudnn, 'enabled', False)
    kw = dict(kw)
    if kw.get('frozen_stages') == 'all':
        kw['frozen_stages'] = _xs_stages()
    ma, mb = _model(arch, cin, **kw).cuda(), _model(arch, cin, **kw).cuda()
    whole = arch != 'TL_LFD_L'
    assert train_engine.supported(mb._backbone) and train_engine.network_supported(mb) == whole
    lr, mom, wd = cases.LR, cases.MOMENTUM, cases.WEIGHT_DECAY
    oa = torch.optim.SGD([p for p in ma.parameters() if p.requires_grad], lr=lr, momentum=mom, weight_decay=wd)
    ob = optim.SGD(mb.parameters(), lr=lr, momentum=mom, weight_decay=wd)
    with torch.no_grad():
        for (ka, va), (kb, vb) in zip(ma.state_dict().items(), mb.state_dict().items()):
            assert ka == kb
            vb.copy_(va)
    x = torch.rand(2, cin, 96, 128, generator=torch.Generator().manual_seed(11)).cuda() * 2 - 1
    ann = cases.annotations('WIDERFACE_LFD_XS', configs.ARCHS[arch]['num_classes'])        # boxes for 2 x 96 x 128
    max_norm = float(cases.GRAD_CLIP['max_norm'])
    before = {k: v.detach().clone() for k, v in mb.state_dict().items()}
    frozen = {k for k, p in mb.named_parameters() if not p.requires_grad}
    eval_norms = {k for k, m_ in mb.named_modules() if isinstance(m_, nn.BatchNorm2d) and not m_.training}
    expect_frozen = kw.get('frozen_stages', -1) > 0
    assert bool(frozen) == expect_frozen and bool(eval_norms)

    monkeypatch.setenv('LFD_HIP_TRAIN', '0')
    la = ma.get_loss(ma(x), ann)
    oa.zero_grad()
    la['loss'].backward()
    ta = [p for p in ma.parameters() if p.requires_grad]
    ga = torch.cat([p.grad.reshape(-1) for p in ta]).double()
    na = float(torch.nn.utils.clip_grad_norm_(ta, max_norm, 2))
    oa.step()

    monkeypatch.setenv('LFD_HIP_TRAIN', '1')
    node = train_engine.NetworkTrainFunction if whole else train_engine.BackboneTrainFunction
    called, calls = [], []
    orig, real = node.apply, ops.lib
    monkeypatch.setattr(node, 'apply', lambda *a: called.append(1) or orig(*a))
    monkeypatch.setattr(ops, 'lib', lambda: _Recorder(real, calls))
    lb = mb.get_loss(mb(x), ann)
    ob.zero_grad()
    lb['loss'].backward()
    monkeypatch.setattr(ops, 'lib', real)
    assert called, 'the HIP training node did not run'
    tb = [p for p in mb.parameters() if p.requires_grad]
    gb = torch.cat([p.grad.reshape(-1) for p in tb]).double()
    for k, p in mb.named_parameters():
        assert (p.grad is None) == (k in frozen), k
    nb = float(ob.clip_and_step(max_norm))

    # which kernels ran: the one-pass backward exactly for the trainable eval-norm units, no batch-statistics fusion on them
    units = mb.__dict__['_lfd_train_plan'][0] if whole else mb._backbone.__dict__['_lfd_train_plan'][0]
    n_eval_trainable = sum(1 for u in units if u.eval_norm and not u.frozen)
    assert calls.count('lfd_bn_eval_bwd_f16') == n_eval_trainable
    assert calls.count('lfd_bn_eval_stats_f32') == 1
    assert calls.count('lfd_conv_bn_eval_fold_f32') == (1 if expect_frozen else 0)
    if kw.get('norm_eval') or kw.get('frozen_stages', -1) >= 1:
        assert 'lfd_conv1x1_of_bn_relu_bn_stats_nhwc_f16' not in calls and 'lfd_conv1x1_dgrad_bn_bwd_sums_nhwc_f16' not in calls
        assert 'lfd_stem_conv0_train_fwd_bn_stats' not in calls and 'lfd_stem_gray_train_fwd_bn_stats' not in calls
        assert 'lfd_stem_conv0_bn_bwd_wgrad_rows' not in calls and 'lfd_stem_gray_bn_bwd_wgrad_rows' not in calls

    va = np.array([la['loss_values'][k] for k in ('loss', 'classification_loss', 'regression_loss')], np.float64)
    vb = np.array([lb['loss_values'][k] for k in ('loss', 'classification_loss', 'regression_loss')], np.float64)
    e_loss = float((np.abs(vb - va) / np.abs(va)).max())
    e_norm = abs(nb - na) / na
    cos = float(ga @ gb / (ga.norm() * gb.norm()))
    st = 0.0
    after = mb.state_dict()
    for (k, a), (_, b) in zip(ma.state_dict().items(), after.items()):
        mod = k.rsplit('.', 1)[0]
        if mod in eval_norms:
            if k.endswith(('running_mean', 'running_var', 'num_batches_tracked')):
                assert torch.equal(b, before[k]), '%s of an eval-mode norm changed' % k
                assert torch.equal(a, before[k]), '%s changed on the fp32 route' % k
        elif k.endswith('running_mean') or k.endswith('running_var'):
            st = max(st, float((a - b).double().norm() / a.double().norm().clamp_min(1e-3)))
        elif k.endswith('num_batches_tracked'):
            assert int(b) == int(before[k]) + 1 == int(a), k
    for k in frozen:
        assert torch.equal(after[k], before[k]), 'frozen parameter %s changed in the optimizer step' % k
    changed = sum(1 for k, p in mb.named_parameters() if k not in frozen and not torch.equal(p.detach(), before[k]))
    assert changed > 0.9 * len(tb)
    print('%s c%d %s (loss, gradient norm, 1 - cos, running statistics): %.4g %.4g %.4g %.4g; norms %.5g / %.5g'
          % (arch, cin, kw, e_loss, e_norm, 1 - cos, st, na, nb))
    fails = [(w, v, g) for w, v, g in (('loss', e_loss, 0.01), ('gradient norm', e_norm, 0.03), ('1 - cosine', 1 - cos, 0.02),
                                       ('running statistics', st, 0.01)) if not v <= g]
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ 3. GraphedTrainStep
def _annotations(rng, n, hw, num_classes=1, k=5, largest=90):
    ann = []
    for _ in range(n):
        wh = np.exp(rng.uniform(np.log(8), np.log(largest), (k, 2)))
        xy = rng.uniform(0, 1, (k, 2)) * (np.array([hw[1], hw[0]]) - wh).clip(1)
        ann.append((np.concatenate([xy, wh], 1).astype(np.float32), rng.integers(0, num_classes, k).astype(np.int64)))
    return ann


def test_graphed_train_step_on_a_frozen_stem_norm_eval_model_equals_the_eager_iterations():
    """three iterations of GraphedTrainStep (eager, capture, replay) on frozen_stages=1 + norm_eval: losses, gradient norm,
    parameters and buffers bit for bit those of the eager train_step (pattern: test_graphed_train_step_equals_the_eager_iterations)"""
    rng = np.random.default_rng(3)
    torch.manual_seed(5)
    kw = dict(frozen_stages=1, norm_eval=True)
    ma = configs.build_model('WIDERFACE_LFD_XS', **kw).cuda().train()
    mb = configs.build_model('WIDERFACE_LFD_XS', **kw).cuda().train()
    configs.perturb_weights(ma, seed=2)
    mb.load_state_dict(ma.state_dict())
    okw = dict(lr=0.02, momentum=0.9, weight_decay=1e-4)
    oa, ob = optim.SGD(ma.parameters(), **okw), optim.SGD(mb.parameters(), **okw)
    clip = dict(max_norm=10, norm_type=2)
    step = train.GraphedTrainStep(mb, ob, clip, max_boxes=64)
    start = {k: v.detach().clone() for k, v in mb.state_dict().items()}
    replays = 0
    for it in range(3):
        x = torch.from_numpy(rng.normal(0, 1, (4, 3, 160, 192)).astype(np.float32)).cuda()
        ann = _annotations(rng, 4, (160, 192))
        if it % 2:
            ann[1] = (ann[1][0][:2], ann[1][1][:2])
            ann[2] = (ann[2][0][:0], ann[2][1][:0])
        lva, na = train.train_step(ma, oa, x, ann, clip, True)
        lvb, nb = step(x, ann, True)
        replays += len(step.graphs) > 0
        assert lva == lvb, (it, lva, lvb)
        assert float(na) == float(nb), it
        for (k, pa), pb in zip(ma.named_parameters(), mb.parameters()):
            assert torch.equal(pa, pb), (it, k)
        for (k, ba), bb in zip(ma.named_buffers(), mb.buffers()):
            assert torch.equal(ba, bb), (it, k)
    assert len(step.graphs) == 1 and replays >= 2 and not step._eager_only
    for k, p in mb.named_parameters():
        if not p.requires_grad:
            assert p.grad is None and torch.equal(p.detach(), start[k]), k
    for k, m_ in mb._backbone.named_modules():
        if isinstance(m_, nn.BatchNorm2d):
            assert not m_.training and int(m_.num_batches_tracked) == int(start['_backbone.%s.num_batches_tracked' % k])
            assert torch.equal(m_.running_var, start['_backbone.%s.running_var' % k])
    assert int(mb._neck.neck0[1].num_batches_tracked) == int(start['_neck.neck0.1.num_batches_tracked']) + 3


# ------------------------------------------------------------------------------------------------ 4. regression
def test_unfrozen_iteration_calls_the_entry_points_it_called_before(monkeypatch):
    """the shipped WIDERFACE_LFD_S without frozen stages: the entry points of a steady-state iteration, in order, are the recorded
    ones (tests/golden/wf_s_train_iteration_entry_points.json) -- none of the eval-mode kernels, every fusion in place"""
    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                                       'wf_s_train_iteration_entry_points.json')))['calls']
    rng = np.random.default_rng(4)
    torch.manual_seed(0)
    m = configs.build_model('WIDERFACE_LFD_S').cuda().train()
    opt = optim.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    x = torch.from_numpy(rng.normal(0, 1, (4, 3, 160, 192)).astype(np.float32)).cuda()
    ann = _annotations(rng, 4, (160, 192), 1)
    clip = dict(max_norm=10, norm_type=2)
    train.train_step(m, opt, x, ann, clip, True)
    calls = []
    real = ops.lib
    monkeypatch.setattr(ops, 'lib', lambda: _Recorder(real, calls))
    train.train_step(m, opt, x, ann, clip, True)
    monkeypatch.setattr(ops, 'lib', real)
    assert not [c for c in calls if 'bn_eval' in c]
    assert len(want) > 200 and calls == want
