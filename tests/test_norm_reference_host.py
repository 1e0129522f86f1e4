"""The float64 references, the fp32 restatement and the case tables of tests/golden/norm_cases.py, checked without a GPU: every
reference against torch's double-precision autograd of F.batch_norm / F.group_norm (run level by level, the way the reference
model runs its neck and head), the one-value-per-channel convention, and the conditions the GPU tests
(tests/test_gpu_train_norms.py) rely on for every case."""
import ast
import os

import pytest
import torch
import torch.nn.functional as F

import norm_cases as NC

RTOL = 1e-12


def _close(got, ref, what):
    scale = float(ref.abs().max()) + 1e-300
    err = float((got - ref).abs().max()) / scale
    assert err <= RTOL, '%s: %.3g relative' % (what, err)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('c', [8, 128])
def test_batchnorm_references_equal_double_autograd(c, relu):
    n, inv = 3, 1.0 / NC.LOSS_SCALE
    for l, (h, w) in enumerate(NC.BN_LEVELS):
        y, dz = NC.activations((n, h, w, c), 90 + l), NC.gradients((n, h, w, c), 90 + l)
        gamma, beta = NC.norm_params(c, 90 + l)
        rm, rv = NC.running_stats(c, 90 + l)
        res = NC.rand16((n, h, w, c), 95 + l) if l % 2 else None
        yr = _nchw(y.double()).requires_grad_(True)
        gr, br = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
        rr = _nchw(res.double()).requires_grad_(True) if res is not None else None
        trm, trv = rm.double().clone(), rv.double().clone()
        o = F.batch_norm(yr, trm, trv, gr, br, True, NC.MOMENTUM, NC.EPS)
        if rr is not None:
            o = o + rr
        if relu:
            o = F.relu(o)
        o.backward(_nchw(dz.double()))
        f = NC.bn_forward_ref(y.reshape(-1, c), NC.EPS, NC.MOMENTUM, rm, rv)
        _close(f['running_mean'], trm, 'running_mean')
        _close(f['running_var'], trv, 'running_var')
        _close(f['mean'], y.double().reshape(-1, c).mean(0), 'mean')
        _close(f['var'], y.double().reshape(-1, c).var(0, unbiased=False), 'var')
        stats = torch.cat([f['mean'], f['rstd']])
        flat = lambda t: None if t is None else t.reshape(-1, c)
        z, operands, _, _ = NC.bn_apply_ref(flat(y), stats, gamma, beta, flat(res), relu)
        _close(z, o.detach().permute(0, 2, 3, 1).reshape(-1, c), 'z')
        r = NC.bn_backward_ref(flat(dz), flat(y), (z > 0) if relu else None, stats, gamma, inv)
        _close(r['dy'], yr.grad.permute(0, 2, 3, 1).reshape(-1, c), 'dy')
        _close(r['dgamma'], gr.grad * inv, 'dgamma')
        _close(r['dbeta'], br.grad * inv, 'dbeta')
        if rr is not None:
            _close(r['g'], rr.grad.permute(0, 2, 3, 1).reshape(-1, c), 'residual gradient')


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('name', [c[0] for c in NC.GN_SEG_CASES if c[0] != 'cap_binds'] + [c[0] for c in NC.GN_PLAIN_CASES])
def test_groupnorm_references_equal_double_autograd_level_by_level(name, relu):
    d = NC.gn_seg_inputs(name) if name in [c[0] for c in NC.GN_SEG_CASES] else NC.gn_plain_inputs(name)
    n, groups, seg_hw, c, inv = d['n'], d['groups'], d['seg_hw'], d['c'], 1.0 / NC.LOSS_SCALE
    gr, br = d['gamma'].double().requires_grad_(True), d['beta'].double().requires_grad_(True)
    zs, dys, means, rstds = [], [], [], []
    o0 = 0
    for hw in seg_hw:                                    # every level a tensor of its own; parameter gradients add up
        yl = d['y'][:, o0:o0 + hw].double().permute(0, 2, 1).reshape(n, c, hw, 1).requires_grad_(True)
        o = F.group_norm(yl, groups, gr, br, NC.EPS)
        if relu:
            o = F.relu(o)
        o.backward(d['dz'][:, o0:o0 + hw].double().permute(0, 2, 1).reshape(n, c, hw, 1))
        zs.append(o.detach().reshape(n, c, hw).permute(0, 2, 1))
        dys.append(yl.grad.reshape(n, c, hw).permute(0, 2, 1))
        yg = yl.detach().reshape(n, groups, 8 * hw)
        means.append(yg.mean(2))
        rstds.append(1 / torch.sqrt(yg.var(2, unbiased=False) + NC.EPS))
        o0 += hw
    stats = NC.gn_forward_ref(d['y'], seg_hw, groups)
    assert stats.shape == (n, len(seg_hw), 2, groups)
    _close(stats[:, :, 0], torch.stack(means, 1), 'mean')
    _close(stats[:, :, 1], torch.stack(rstds, 1), 'rstd')
    z, _ = NC.gn_apply_ref(d['y'], seg_hw, groups, stats, d['gamma'], d['beta'], relu)
    _close(z, torch.cat(zs, 1), 'z')
    r = NC.gn_backward_ref(d['dz'], d['y'], (z > 0) if relu else None, seg_hw, groups, stats, d['gamma'], inv)
    _close(r['dy'], torch.cat(dys, 1), 'dy')
    _close(r['dgamma'], gr.grad * inv, 'dgamma')
    _close(r['dbeta'], br.grad * inv, 'dbeta')


def test_one_value_per_channel_follows_the_kernel_convention():
    """m == 1 (bn_stats_final_body): variance 0, rstd = 1 / sqrt(eps), running_var blended with the biased variance; finite"""
    c = 128
    y = NC.activations((1, c), 3)
    rm, rv = NC.running_stats(c, 3)
    f = NC.bn_forward_ref(y, NC.EPS, NC.MOMENTUM, rm, rv)
    assert all(bool(torch.isfinite(v).all()) for v in f.values())
    assert torch.equal(f['mean'], y.double()[0]) and torch.equal(f['var'], torch.zeros(c, dtype=torch.float64))
    assert torch.equal(f['rstd'], torch.full((c,), 1.0 / (NC.EPS ** 0.5), dtype=torch.float64))
    assert torch.equal(f['running_var'], (1 - NC.MOMENTUM) * rv.double())
    _close(f['running_mean'], (1 - NC.MOMENTUM) * rm.double() + NC.MOMENTUM * y.double()[0], 'running_mean')
    gamma, beta = NC.norm_params(c, 3)
    stats = torch.cat([f['mean'], f['rstd']]).float()
    z, operands, _, _ = NC.bn_apply_ref(y, stats, gamma, beta, None, False)
    assert torch.equal(z, beta.double().expand_as(z))
    # in fp32, b = beta - mean * a is rounded at the magnitude of mean * a (a = gamma / sqrt(eps) ~ 300): inside the store bound
    got = NC.bn_apply_f32(y, stats, gamma, beta, None, False)
    assert bool(((got.double() - z).abs() <= NC.store_bound(z, operands)).all())
    r = NC.bn_backward_ref(NC.gradients((1, c), 3), y, None, stats, gamma, 1.0 / NC.LOSS_SCALE)
    assert float(r['dy'].abs().max()) == 0.0 and bool(torch.isfinite(r['dgamma']).all())


def test_no_case_leaves_a_recomputed_relu_mask_undecided():
    total = 0
    for name, y, gamma, beta in NC.recomputed_mask_cases():
        f = NC.bn_forward_ref(y)
        _, _, pre, terms = NC.bn_apply_ref(y, torch.cat([f['mean'], f['rstd']]), gamma, beta, None, True)
        count = int(NC.undecided(pre, terms).sum())
        total += pre.numel()
        assert count == 0, '%s: %d of %d elements undecided -- choose another seed' % (name, count, pre.numel())
    assert total > 0


def _stats_shapes():
    """_STATS_SHAPES of tests/test_gpu_train_convs.py, read from its source (importing that module needs the built library)"""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'test_gpu_train_convs.py')).read()
    for node in ast.parse(src).body:
        if isinstance(node, ast.Assign) and getattr(node.targets[0], 'id', None) == '_STATS_SHAPES':
            return ast.literal_eval(node.value)
    raise AssertionError('_STATS_SHAPES not found')


def test_case_tables_are_consistent():
    shapes = _stats_shapes()
    for cin in NC.BN_PARTIALS_CIN:
        assert (cin, NC.BN_PARTIALS_COUT, 1, 1) in shapes
    assert len(NC.BN_PARTIALS_CIN) == len(NC.BN_LEVELS)
    for name, n, groups, seg_hw, _ in NC.GN_SEG_CASES:
        d = NC.gn_seg_inputs(name)
        assert 1 <= len(seg_hw) <= NC.MAX_LEVELS and n * len(seg_hw) <= 4096 and groups in (1, 2, 4, 8, 16, 32)
        assert d['y'].shape == d['dz'].shape == (n, sum(seg_hw), 8 * groups)
        assert NC.seg_group_expand(torch.zeros(n, len(seg_hw), groups), seg_hw).shape == d['y'].shape
    assert len(NC.gn_seg_case('max_levels')[3]) == NC.MAX_LEVELS
    n, g, seg = NC.gn_seg_case('cap_binds')[1:4]
    assert NC.gn_blocks(max(seg) * g, n * len(seg)) == 29 and -(-max(seg) * g // NC.THREADS) == 30
    n, g, seg = NC.gn_seg_case('pyramid')[1:4]
    assert NC.gn_blocks(max(seg) * g, n * len(seg)) == 64 and NC.gn_chain(n, seg, g) == 8 * 2 + 16
    assert [hw * 4 for hw in NC.gn_seg_case('block_edges')[3]] == [1028, 256, 4]
    starts, p = NC.bn_level_starts()
    assert starts == [0, 68, 88, 94] and p == 98 and p > sum(h * w for h, w in NC.BN_LEVELS)
    for c in (64, 128):
        d = NC.bn_level_inputs(c)
        assert d['dz'].shape == (NC.BN_LEVEL_N, p, c) and [tuple(l['y'].shape[1:3]) for l in d['levels']] == NC.BN_LEVELS
    assert sorted(m * c // 8 for _, (n, h, w, c), _ in NC.BN_PLAIN_CASES for m in [n * h * w] if c == 8) == [1, 2, 255, 256, 257]
    assert {c for _, (_, _, _, c), _ in NC.BN_PLAIN_CASES} >= {8, 16, 256} and {s[3] // 8 for _, s in NC.GN_PLAIN_CASES} >= {1, 2, 32}
    n, h, w, c = next(s for nm, s, _ in NC.BN_PLAIN_CASES if nm == 'above_grid_cap')
    assert n * h * w * c // 8 > NC.BN_MAX_BLOCKS * NC.THREADS and NC.bn_chain(n * h * w, c) == 2 + 16


def test_fp32_restatement_is_within_the_store_bound_of_float64():
    for name, n, groups, seg_hw, _ in NC.GN_SEG_CASES:
        d = NC.gn_seg_inputs(name)
        stats = NC.gn_forward_ref(d['y'], seg_hw, groups).float()
        for relu in (True, False):
            z, operands = NC.gn_apply_ref(d['y'], seg_hw, groups, stats.double(), d['gamma'], d['beta'], relu)
            got = NC.gn_apply_f32(d['y'], seg_hw, groups, stats, d['gamma'], d['beta'], relu)
            assert bool(((got.double() - z).abs() <= NC.store_bound(z, operands)).all()), (name, relu)
    for name, shape, mode in NC.BN_PLAIN_CASES:
        d = NC.bn_plain_inputs(name)
        c = d['c']
        y = d['y'].reshape(-1, c)
        f = NC.bn_forward_ref(y)
        stats = torch.cat([f['mean'], f['rstd']]).float()
        res = d['res'].reshape(-1, c) if d['res'] is not None else None
        for relu in (True, False):
            z, operands, _, _ = NC.bn_apply_ref(y, stats, d['gamma'], d['beta'], res, relu)
            got = NC.bn_apply_f32(y, stats, d['gamma'], d['beta'], res, relu)
            assert bool(((got.double() - z).abs() <= NC.store_bound(z, operands)).all()), (name, relu)
    for c in (64, 128):
        for lv in NC.bn_level_inputs(c)['levels']:
            y = lv['y'].reshape(-1, c)
            f = NC.bn_forward_ref(y)
            stats = torch.cat([f['mean'], f['rstd']]).float()
            z, operands, _, _ = NC.bn_apply_ref(y, stats, lv['gamma'], lv['beta'], None, True)
            got = NC.bn_apply_f32(y, stats, lv['gamma'], lv['beta'], None, True)
            assert bool(((got.double() - z).abs() <= NC.store_bound(z, operands)).all())
