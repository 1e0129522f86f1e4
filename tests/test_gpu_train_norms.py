"""The train-mode BatchNorm / GroupNorm kernels of csrc/train.hip -- the level-concatenated ones the default training schedule
runs, and the plain ones at the channel / group counts nothing else runs -- against the float64 references of
tests/golden/norm_cases.py.

Every comparison is per element (|got - ref| <= bound everywhere) with the bounds norm_cases derives from the number formats and
the launch geometry; the forward apply passes are also compared bit for bit with their fp32 restatement.  Every output buffer
starts as NaN bit patterns: the ones a test hands in are filled here, the ones the ops wrappers allocate come from a patched
torch.empty / torch.empty_like, and the training workspace (per-block partial rows) is re-filled before every test -- an
unwritten element, a row written past a level or a partial row read before it was written cannot pass."""
import pytest
import torch

import norm_cases as NC
from lfd_amd import ops

pytestmark = pytest.mark.gpu

EPS, MOM, INV = NC.EPS, NC.MOMENTUM, 1.0 / NC.LOSS_SCALE
SENTINEL16 = 0x7D5A               # an fp16 NaN no kernel produces (the hardware's own NaN is 0x7E00)
OUTSIDE_ROWS = float('nan')       # rows of a concatenated gradient that belong to no level


# ------------------------------------------------------------------------------------------------ plumbing
@pytest.fixture(autouse=True)
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


def _cu(t):
    return None if t is None else t.cuda()


def _nan32(n):
    return torch.full((n,), float('nan'), device='cuda')


def _sentinel16(shape):
    return torch.full(shape, SENTINEL16, dtype=torch.int16, device='cuda').view(torch.float16)


def _within(got, ref, bound, what):
    """per element; a NaN anywhere fails"""
    got = got.detach().double().cpu().reshape(ref.shape)
    err = (got - ref).abs()
    bad = ~(err <= bound)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound).nan_to_num(float('inf'))      # (0 <= 0 is inside a zero bound)
    print('%s: max |err| / bound = %.3g over %d elements' % (what, float(ratio.max()), err.numel()))
    assert not bool(bad.any()), '%s: %d of %d elements outside the bound (worst |err| / bound %.3g)' % (
        what, int(bad.sum()), bad.numel(), float(ratio.max()))


def _stat_close(got, ref, what, rtol=1e-5, atol=1e-6):
    """the project's tolerances for statistics (tests/test_gpu_train_convs.py)"""
    got = got.detach().double().cpu().reshape(ref.shape)
    assert bool(torch.isfinite(got).all()), what
    torch.testing.assert_close(got, ref, rtol=rtol, atol=atol, msg=lambda m: '%s: %s' % (what, m))


def _same_bits(got, restated, what):
    """the kernel's z against the fp32 restatement (value equality of fp16: +0 == -0, NaN equals nothing)"""
    got = got.detach().cpu().reshape(restated.shape)
    mism = int((got != restated).sum())
    print('%s: %d of %d elements differ from the fp32 restatement' % (what, mism, got.numel()))
    assert mism == 0, '%s: %d elements differ from the fp32 restatement' % (what, mism)


def _check_bn_stats(stats, y2d, what, rm=None, rv=None, rm0=None, rv0=None):
    c = y2d.size(1)
    f = NC.bn_forward_ref(y2d, EPS, MOM, rm0, rv0)
    _stat_close(stats[:c], f['mean'], what + ' mean')
    _stat_close(stats[c:], f['rstd'], what + ' rstd', atol=0)
    if rm0 is not None:
        _stat_close(rm, f['running_mean'], what + ' running_mean')
        _stat_close(rv, f['running_var'], what + ' running_var')


def _check_bn_apply(z_rows, y2d, stats, gamma, beta, res, relu, what):
    st = stats.detach().cpu()
    ref, operands, _, _ = NC.bn_apply_ref(y2d, st, gamma, beta, res, relu)
    _within(z_rows, ref, NC.store_bound(ref, operands), what + ' z')
    _same_bits(z_rows, NC.bn_apply_f32(y2d, st, gamma, beta, res, relu), what + ' z')


def _grad_buffers(c, accumulate):
    """accumulate: += onto dgamma = 2, dbeta = -1; else onto NaN"""
    if accumulate:
        return torch.full((c,), 2.0, device='cuda'), torch.full((c,), -1.0, device='cuda'), 2.0, -1.0
    return _nan32(c), _nan32(c), None, None


def _check_param_grads(dg, db, r, bounds, pg, pb, what):
    _within(dg, r['dgamma'] + (pg or 0.0), bounds[1], what + ' dgamma')
    _within(db, r['dbeta'] + (pb or 0.0), bounds[2], what + ' dbeta')


# ------------------------------------------------------------------------------------------------ A, B: GroupNorm over segments
_gn_fwd = {}


def _gn_seg_forward(d, relu, key):
    """stats, z of gn_train_stats_apply_seg for a case (kept on the device for the backward tests)"""
    if key not in _gn_fwd:
        _gn_fwd[key] = ops.gn_train_stats_apply_seg(_cu(d['y']), d['seg_hw'], d['groups'], EPS, _cu(d['gamma']), _cu(d['beta']), relu)
    return _gn_fwd[key]


def _check_gn_forward(d, stats, z, relu, what):
    n, groups, seg_hw = d['n'], d['groups'], d['seg_hw']
    ref = NC.gn_forward_ref(d['y'], seg_hw, groups)
    st = NC.gn_stats_view(stats.cpu(), n, len(seg_hw), groups)
    assert stats.numel() == ref.numel()
    _stat_close(st[:, :, 0], ref[:, :, 0], what + ' mean')
    _stat_close(st[:, :, 1], ref[:, :, 1], what + ' rstd', atol=0)
    zref, operands = NC.gn_apply_ref(d['y'], seg_hw, groups, st, d['gamma'], d['beta'], relu)
    _within(z, zref, NC.store_bound(zref, operands), what + ' z')
    _same_bits(z, NC.gn_apply_f32(d['y'], seg_hw, groups, stats.cpu(), d['gamma'], d['beta'], relu), what + ' z')


def _check_gn_backward(d, stats, z, run, what):
    """run(dz, z, dgamma, dbeta, accumulate) -> dy; both accumulate modes against one float64 reference"""
    n, groups, seg_hw, c = d['n'], d['groups'], d['seg_hw'], d['c']
    st = NC.gn_stats_view(stats.cpu(), n, len(seg_hw), groups)
    mask = None if z is None else z.cpu().reshape(d['y'].shape) > 0
    r = NC.gn_backward_ref(d['dz'], d['y'], mask, seg_hw, groups, st, d['gamma'], INV)
    chain = NC.gn_chain(n, seg_hw, groups)
    for accumulate in (True, False):
        dg, db, pg, pb = _grad_buffers(c, accumulate)
        dy = run(_cu(d['dz']), z, dg, db, accumulate)
        bounds = NC.gn_backward_bounds(r, seg_hw, chain, INV, pg, pb)
        _within(dy, r['dy'], bounds[0], '%s accumulate=%d dy' % (what, accumulate))
        _check_param_grads(dg, db, r, bounds, pg, pb, '%s accumulate=%d' % (what, accumulate))


_SEG_NAMES = [c[0] for c in NC.GN_SEG_CASES]


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('name', _SEG_NAMES)
def test_groupnorm_over_segments_forward(name, relu):
    d = NC.gn_seg_inputs(name)
    stats, z = _gn_seg_forward(d, relu, (name, relu))
    _check_gn_forward(d, stats, z, relu, 'gn_seg %s relu=%d' % (name, relu))
    if len(d['seg_hw']) == 1:          # one segment: the geometry and the launches of the plain two-launch form
        y4 = _cu(d['y']).view(d['n'], d['seg_hw'][0], 1, d['c'])
        stats2, z2 = ops.gn_train_stats_apply(y4, d['groups'], EPS, _cu(d['gamma']), _cu(d['beta']), relu)
        assert torch.equal(stats2, stats) and torch.equal(z2.view_as(z), z)


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('name', _SEG_NAMES)
def test_groupnorm_over_segments_backward(name, relu):
    """relu: the mask from the forward's own z (exact); else z=None, no ReLU"""
    d = NC.gn_seg_inputs(name)
    stats, z = _gn_seg_forward(d, relu, (name, relu))
    y, gamma = _cu(d['y']), _cu(d['gamma'])

    def run(dz, zz, dg, db, accumulate):
        return ops.gn_train_backward_seg(dz, y, zz, d['seg_hw'], d['groups'], stats, gamma, INV, dg, db, accumulate=accumulate)
    _check_gn_backward(d, stats, z if relu else None, run, 'gn_seg_bwd %s relu=%d' % (name, relu))


# ------------------------------------------------------------------------------------------------ C: BatchNorm into levels
def _check_levels_written(zc, written, starts, hws, what):
    """rows of the levels in `written` are no sentinel, every other row still holds the sentinel bits"""
    keep = torch.ones(zc.size(1), dtype=torch.bool, device=zc.device)
    for l in written:
        keep[starts[l]:starts[l] + hws[l]] = False
    bits = zc.view(torch.int16)
    assert bool((bits[:, keep] == SENTINEL16).all()), '%s: a row outside the level was written' % what
    assert not bool((bits[:, ~keep] == SENTINEL16).any()), '%s: an element of the level was not written' % what


@pytest.mark.parametrize('c,relu', NC.BN_INTO_CASES)
def test_batchnorm_apply_into_a_level_concatenated_tensor(c, relu):
    d = NC.bn_level_inputs(c)
    starts, p, n = d['starts'], d['p'], NC.BN_LEVEL_N
    hws = [h * w for h, w in NC.BN_LEVELS]
    zc = _sentinel16((n, p, c))
    order = [2, 0, 3, 1]               # not in row order: a row written past a level lands on sentinel rows
    for i, l in enumerate(order):
        lv = d['levels'][l]
        y = _cu(lv['y'])
        stats = ops.bn_train_stats(y, EPS, MOM)
        _check_bn_stats(stats, lv['y'].reshape(-1, c), 'level %d' % l)
        ops.bn_train_apply_into(y, stats, _cu(lv['gamma']), _cu(lv['beta']), relu, zc, starts[l])
        _check_levels_written(zc, order[:i + 1], starts, hws, 'apply_into level %d' % l)
        rows = zc[:, starts[l]:starts[l] + hws[l]].reshape(-1, c)
        _check_bn_apply(rows, lv['y'].reshape(-1, c), stats, lv['gamma'], lv['beta'], None, relu, 'apply_into c=%d level %d' % (c, l))


@pytest.mark.parametrize('n', [NC.BN_LEVEL_N, 1])
def test_batchnorm_of_all_levels_from_the_conv_partials(n):
    """conv2d_bn_partials -> bn_train_finish_into_levels against float64 over the stored y, and bit for bit against
    conv2d_bn_stats + bn_train_apply_into level by level (what LFD_BN_LEVELS=0 runs).  n = 1: the (1, 1) level has one value per
    channel -- variance 0, rstd = 1 / sqrt(eps), everything finite."""
    lv = NC.bn_partials_inputs(n)
    cout = NC.BN_PARTIALS_COUT
    starts, p = NC.bn_level_starts()
    hws = [h * w for h, w in NC.BN_LEVELS]
    zb = torch.zeros(cout, device='cuda')
    with_running = [True, False, False, True]
    zc, zc1 = _sentinel16((n, p, cout)), _sentinel16((n, p, cout))
    jobs, ys, rms, rvs, per_level = [], [], [], [], []
    for l, L in enumerate(lv):
        x, pk = _cu(L['x']), ops.pack_conv_weight_train(_cu(L['weight']))
        rows = _nan32(512 * 2 * cout)
        r = ops.conv2d_bn_partials(x, pk, zb, L['cin'], cout, 1, 1, rows)
        assert r is not None, 'no statistics epilogue for %d -> %d' % (L['cin'], cout)
        y, nrows = r
        assert 1 <= nrows <= 512 and torch.equal(y, ops.conv2d_nhwc(x, pk, zb, L['cin'], cout, 1, 1, False))
        rm, rv = (_cu(L['running_mean']).clone(), _cu(L['running_var']).clone()) if with_running[l] else (None, None)
        jobs.append((starts[l], y, rows, nrows, EPS, MOM, rm, rv, _cu(L['gamma']), _cu(L['beta'])))
        ys.append(y)
        rms.append(rm)
        rvs.append(rv)
        # the same unit level by level
        rm1, rv1 = (_cu(L['running_mean']).clone(), _cu(L['running_var']).clone()) if with_running[l] else (None, None)
        y1, st1 = ops.conv2d_bn_stats(x, pk, zb, L['cin'], cout, 1, 1, EPS, MOM, rm1, rv1)
        ops.bn_train_apply_into(y1, st1, _cu(L['gamma']), _cu(L['beta']), True, zc1, starts[l])
        per_level.append((y1, st1, rm1, rv1))
    sts = ops.bn_train_finish_into_levels(jobs, n, True, zc)
    _check_levels_written(zc, range(len(lv)), starts, hws, 'finish_into_levels')
    for l, L in enumerate(lv):
        y2d = ys[l].cpu().reshape(-1, cout)
        what = 'finish_into_levels n=%d level %d' % (n, l)
        if with_running[l]:
            _check_bn_stats(sts[l], y2d, what, rms[l], rvs[l], L['running_mean'], L['running_var'])
        else:
            _check_bn_stats(sts[l], y2d, what)
        if y2d.size(0) == 1:
            eps32 = float(torch.tensor(EPS, dtype=torch.float32))          # the kernel receives eps as a float
            assert torch.equal(sts[l][cout:].cpu(), torch.full((cout,), 1.0 / eps32 ** 0.5, dtype=torch.float64).float()), \
                'rstd of one value per channel'
        rows = zc[:, starts[l]:starts[l] + hws[l]].reshape(-1, cout)
        assert bool(torch.isfinite(rows).all())
        _check_bn_apply(rows, y2d, sts[l], L['gamma'], L['beta'], None, True, what)
        y1, st1, rm1, rv1 = per_level[l]
        assert torch.equal(y1, ys[l]) and torch.equal(st1, sts[l]), what + ': statistics differ from conv2d_bn_stats'
        if with_running[l]:
            assert torch.equal(rm1, rms[l]) and torch.equal(rv1, rvs[l]), what + ': running statistics differ'
    assert torch.equal(zc.view(torch.int16), zc1.view(torch.int16)), 'z differs from the level-by-level passes'


# ------------------------------------------------------------------------------------------------ D: BatchNorm from levels
def test_batchnorm_backward_from_a_level_concatenated_gradient():
    c, n = 128, NC.BN_LEVEL_N
    d = NC.bn_level_inputs(c)
    starts, p = d['starts'], d['p']
    hws = [h * w for h, w in NC.BN_LEVELS]
    dzc = torch.full((n, p, c), OUTSIDE_ROWS, dtype=torch.float16, device='cuda')
    for l in range(len(hws)):
        dzc[:, starts[l]:starts[l] + hws[l]] = _cu(d['dz'][:, starts[l]:starts[l] + hws[l]])
    ys = [_cu(lv['y']) for lv in d['levels']]
    gam, bet = [_cu(lv['gamma']) for lv in d['levels']], [_cu(lv['beta']) for lv in d['levels']]
    stats = [ops.bn_train_stats(y, EPS, MOM) for y in ys]
    refs = []
    for l, lv in enumerate(d['levels']):
        y2d = lv['y'].reshape(-1, c)
        _, _, pre, terms = NC.bn_apply_ref(y2d, stats[l].cpu(), lv['gamma'], lv['beta'], None, True)
        assert int(NC.undecided(pre, terms).sum()) == 0, 'the case leaves a ReLU mask undecided: choose another seed'
        dz2d = d['dz'][:, starts[l]:starts[l] + hws[l]].reshape(-1, c)
        refs.append(NC.bn_backward_ref(dz2d, y2d, pre > 0, stats[l].cpu(), lv['gamma'], INV))
    for accumulate in (True, False):
        outs = []
        for batched in (False, True):
            bufs = [_grad_buffers(c, accumulate) for _ in hws]
            if batched:
                dys = ops.bn_train_backward_from_levels(dzc, [(starts[l], ys[l], stats[l], gam[l], bet[l], bufs[l][0], bufs[l][1])
                                                              for l in range(len(hws))], INV, relu=True, accumulate=accumulate)
            else:
                dys = [ops.bn_train_backward_from(dzc, starts[l], ys[l], stats[l], gam[l], bet[l], INV, bufs[l][0], bufs[l][1],
                                                  relu=True, accumulate=accumulate) for l in range(len(hws))]
            for l in range(len(hws)):
                what = 'bwd_from%s accumulate=%d level %d' % ('_levels' if batched else '', accumulate, l)
                dg, db, pg, pb = bufs[l]
                bounds = NC.bn_backward_bounds(refs[l], NC.bn_chain(n * hws[l], c), INV, pg, pb)
                _within(dys[l], refs[l]['dy'], bounds[0], what + ' dy')
                _check_param_grads(dg, db, refs[l], bounds, pg, pb, what)
            outs.append(dys + [b[0] for b in bufs] + [b[1] for b in bufs])
        assert all(torch.equal(a, b) for a, b in zip(*outs)), 'the two forms differ'


# ------------------------------------------------------------------------------------------------ E: the plain kernels
@pytest.mark.parametrize('name', [c[0] for c in NC.BN_PLAIN_CASES])
def test_plain_batchnorm_kernels_at_unused_widths(name):
    d = NC.bn_plain_inputs(name)
    c, mode = d['c'], d['mode']
    y, gamma, beta, res = _cu(d['y']), _cu(d['gamma']), _cu(d['beta']), _cu(d['res'])
    flat = lambda t: None if t is None else t.reshape(-1, c)
    m = flat(d['y']).size(0)
    rm, rv = _cu(d['running_mean']).clone(), _cu(d['running_var']).clone()
    stats = ops.bn_train_stats(y, EPS, MOM, rm, rv)
    _check_bn_stats(stats, flat(d['y']), name, rm, rv, d['running_mean'], d['running_var'])
    relu = mode != 'none'
    z = ops.bn_train_apply(y, stats, gamma, beta, res, relu)
    _check_bn_apply(z, flat(d['y']), stats, d['gamma'], d['beta'], flat(d['res']), relu, name)
    st = stats.cpu()
    if mode == 'y':
        _, _, pre, terms = NC.bn_apply_ref(flat(d['y']), st, d['gamma'], d['beta'], None, True)
        assert int(NC.undecided(pre, terms).sum()) == 0, 'the case leaves a ReLU mask undecided: choose another seed'
        mask = pre > 0
    else:
        mask = flat(z.cpu()) > 0 if relu else None
    r = NC.bn_backward_ref(flat(d['dz']), flat(d['y']), mask, st, d['gamma'], INV)
    for accumulate in (True, False):
        dg, db, pg, pb = _grad_buffers(c, accumulate)
        dy, g = ops.bn_train_backward(_cu(d['dz']), y, z if mode in ('z', 'res') else None, stats, gamma, INV, dg, db,
                                      want_g=mode == 'res', accumulate=accumulate, relu=relu, beta=beta)
        bounds = NC.bn_backward_bounds(r, NC.bn_chain(m, c), INV, pg, pb)
        what = '%s accumulate=%d' % (name, accumulate)
        _within(dy, r['dy'], bounds[0], what + ' dy')
        _check_param_grads(dg, db, r, bounds, pg, pb, what)
        if mode == 'res':               # the residual branch's gradient: dz where the ReLU passed, exactly
            assert torch.equal(flat(g.cpu()).double(), r['g'])


@pytest.mark.parametrize('relu', [True, False])
@pytest.mark.parametrize('name', [c[0] for c in NC.GN_PLAIN_CASES])
def test_plain_groupnorm_kernels_at_unused_group_counts(name, relu):
    d = NC.gn_plain_inputs(name)
    n, hw, c, groups = d['n'], d['seg_hw'][0], d['c'], d['groups']
    y4, gamma, beta = _cu(d['y']).view(n, hw, 1, c), _cu(d['gamma']), _cu(d['beta'])
    stats = ops.gn_train_stats(y4, groups, EPS)
    z = ops.gn_train_apply(y4, groups, stats, gamma, beta, relu)
    _check_gn_forward(d, stats, z, relu, 'gn %s relu=%d' % (name, relu))
    stats2, z2 = ops.gn_train_stats_apply(y4, groups, EPS, gamma, beta, relu)
    assert torch.equal(stats2, stats) and torch.equal(z2, z)

    def run(dz, zz, dg, db, accumulate):
        return ops.gn_train_backward(dz.view(n, hw, 1, c), y4, zz, groups, stats, gamma, INV, dg, db, accumulate=accumulate)
    _check_gn_backward(d, stats, z if relu else None, run, 'gn_bwd %s relu=%d' % (name, relu))


# ------------------------------------------------------------------------------------------------ F: statistics against mean / std
def _rel_err(got, ref):
    return float(((got.double().cpu().reshape(ref.shape) - ref) / ref).abs().max())


def _bn_rstd_errors(shape, ratio):
    y = NC.accuracy_input(shape, ratio)
    c = shape[3]
    ref = NC.bn_forward_ref(y.reshape(-1, c))['rstd']
    yc = y.cuda()
    hip = _rel_err(ops.bn_train_stats(yc, EPS, MOM)[c:], ref)
    _, _, invstd = torch.native_batch_norm(yc.permute(0, 3, 1, 2).float().contiguous(), None, None, None, None, True, MOM, EPS)
    return hip, _rel_err(invstd, ref)


def _gn_rstd_errors(ratio):
    _, n, groups, seg_hw, _ = NC.gn_seg_case(NC.ACCURACY_GN_CASE)
    c = 8 * groups
    y = NC.accuracy_input((n, sum(seg_hw), c), ratio)
    ref = NC.gn_forward_ref(y, seg_hw, groups)[:, :, 1]
    yc = y.cuda()
    ones, zeros = torch.ones(c, device='cuda'), torch.zeros(c, device='cuda')
    stats, _ = ops.gn_train_stats_apply_seg(yc, seg_hw, groups, EPS, ones, zeros, False)
    hip = _rel_err(stats.view(n, len(seg_hw), 2, groups)[:, :, 1], ref)
    o, ts = 0, []
    for hw in seg_hw:                    # torch: every level a tensor of its own
        x = yc[:, o:o + hw].permute(0, 2, 1).float().reshape(n, c, hw, 1).contiguous()
        ts.append(torch.native_group_norm(x, None, None, n, c, hw, groups, EPS)[2].reshape(n, groups))
        o += hw
    return hip, _rel_err(torch.stack(ts, 1), ref)


@pytest.mark.parametrize('ratio', NC.ACCURACY_RATIOS_ASSERTED + NC.ACCURACY_RATIOS_PRINTED)
def test_accuracy_of_the_statistics_against_mean_over_std(ratio):
    """rstd against float64 over the stored fp16 values of N(ratio, 1) inputs.  The sums of y and y^2 are fp32 per thread and per
    block, only the final var = E[y^2] - mean^2 is fp64, so the error grows with (mean / std)^2: the project's 1e-5 is asserted
    at mean / std in {0.25, 2}; at {4, 16, 64} the error is printed next to that of torch's own fp32 batch_norm / group_norm on
    the same tensor (DESIGN.md holds the table)."""
    rows = [('bn_train_stats %s' % (s,),) + _bn_rstd_errors(s, ratio) for s in NC.ACCURACY_BN_SHAPES]
    rows.append(('gn_train_stats_apply_seg %s' % NC.ACCURACY_GN_CASE,) + _gn_rstd_errors(ratio))
    for what, hip, ref32 in rows:
        print('rstd accuracy: mean/std=%g %s: hip %.3g torch-fp32 %.3g' % (ratio, what, hip, ref32))
    if ratio in NC.ACCURACY_RATIOS_ASSERTED:
        for what, hip, _ in rows:
            assert hip <= 1e-5, '%s at mean/std=%g: %.3g' % (what, ratio, hip)
