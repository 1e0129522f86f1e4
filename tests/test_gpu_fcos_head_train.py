"""GPU tests of the FCOSHead training node (train_engine.DetectorTrainFunction): the glue kernels of csrc/fcos_out.hip per
element against float64 on the CPU, the node against the package's own route with the head under autograd (LFD_HIP_HEAD=0)
from identical state, whole FCOS_FPN iterations, and the argument checks.

Bounds of the kernel tests.  A dy element is ONE fp16 rounding of a correctly rounded fp32 value:
    |got - ref| <= 2^-11 |ref| + 2^-24 |ref|
(the gradients are drawn so that every result is a normal fp16 number: below 2^-14 fp16's spacing is absolute and the bound
above, which has no such term, would not describe the format).  A reduction is a chain of fp32 additions:
    |got - ref| <= K 2^-24 sum|addends|,   K = trips + 256 / (ROWS / 8) + 4
-- a thread adds `trips` addends (its grid-stride walk: trips = ceil(n hw (ROWS/8) / (256 blocks)), blocks = min(1024,
ceil(n hw (ROWS/8) / 256))), the block partial then adds the 256 / (ROWS/8) threads that hold the row in thread order: an addend
passes through at most trips + 256 / (ROWS/8) fp32 additions; + 1 for the rounding of the addend itself (a product, formed in
fp64 and rounded once), + 2 for the final `+=` (the fp64 total rounded to fp32, then added to what the buffer held, which is
counted among the addends), + 1 for the second-order terms and the fp64 additions of the final."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

import sibling_cases as SC
from lfd_amd import _lib, configs, ops, train_engine as te
from test_gpu_pyramid_train import _GATES

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U16, U32 = 2.0 ** -11, 2.0 ** -24
FIVE = [(13, 17), (7, 9), (4, 5), (2, 3), (1, 2)]
ONE = [(1, 1)]
BIG = [(168, 200), (3, 5)]          # 2 x 33600 pixels: more (pixel, piece) pairs than 1024 blocks x 256 threads at both row counts
CASES = [(rows, c, lv) for rows in (32, 64) for c in (1, 3, rows - 1) for lv in (FIVE, ONE)]
IDS = ['rows%d-C%d-%s' % (r, c, 'five' if lv is FIVE else 'one') for r, c, lv in CASES]

_cache = {}


def _inputs(rows, c, sizes):
    """seeded raw conv outputs (the padded rows hold values too: nothing may read them), scales, and the forward's outputs --
    computed once per case and shared, never modified"""
    key = (rows, c, tuple(sizes))
    if key in _cache:
        return _cache[key]
    g = torch.Generator().manual_seed(rows * 1000 + c * 10 + len(sizes) + sizes[0][0])
    raw_cls = [torch.randn(2, h, w, rows, generator=g) * 3 for h, w in sizes]
    raw_reg = [torch.rand(2, h, w, rows, generator=g) * 12 - 6 for h, w in sizes]
    scales = [torch.rand((), generator=g) * 0.4 + 0.8 for _ in sizes]
    starts, p = te._level_starts(sizes)
    d = dict(raw_cls=raw_cls, raw_reg=raw_reg, scales=scales, starts=starts, p=p, sizes=sizes, rows=rows, c=c)
    d['dev'] = dict(raw_cls=[t.to(DEV) for t in raw_cls], raw_reg=[t.to(DEV) for t in raw_reg], scales=[t.to(DEV) for t in scales])
    cls, reg, ctr = (torch.full((2, p, k), float('nan'), device=DEV) for k in (c, 4, 1))
    ops.fcos_out_pack_levels([dict(raw_cls=a, raw_reg=b, scale=s, point0=p0) for a, b, s, p0 in
                              zip(d['dev']['raw_cls'], d['dev']['raw_reg'], d['dev']['scales'], starts)], cls, reg, ctr)
    d['out'] = (cls, reg, ctr)
    _cache[key] = d
    return d


# ----------------------------------------------------------------------------------------------- (a) glue forward
@pytest.mark.parametrize('rows,c,sizes', CASES + [(32, 3, BIG), (64, 4, BIG)], ids=IDS + ['rows32-big', 'rows64-C4-big'])
def test_pack_levels_vs_float64(rows, c, sizes):
    """cls / ctr: the raw rows, bit for bit; reg: the bits of ops.pack_level_outputs(exp=True) (the inference kernel) on the same
    raw values, and within 4 fp32 ulp of float64 exp.  The expression both kernels evaluate is expf(fl32(raw * scale)): the
    product's fp32 rounding is part of it, so the float64 exp takes the fp32 product; against exp of the exact product the
    distance is printed (|raw * scale| <= 7.2 moves the argument by up to 2^-22, that is up to 4 more ulp of the result)."""
    d = _inputs(rows, c, sizes)
    cls, reg, ctr = (t.cpu() for t in d['out'])
    assert not bool(torch.isnan(cls).any() | torch.isnan(reg).any() | torch.isnan(ctr).any())        # every element written
    worst = worst_exact = 0.0
    inf_reg = torch.full((2, d['p'], 4), float('nan'), device=DEV)
    for l, (h, w) in enumerate(sizes):
        p0, hw = d['starts'][l], h * w
        rc, rr, s = d['raw_cls'][l].view(2, hw, rows), d['raw_reg'][l].view(2, hw, rows), d['scales'][l]
        assert torch.equal(cls[:, p0:p0 + hw], rc[..., :c]) and torch.equal(ctr[:, p0:p0 + hw, 0], rc[..., c])
        ops.pack_level_outputs(d['dev']['raw_reg'][l], inf_reg, 0, 4, p0, scale=float(s), exp=True)
        prod32 = rr[..., :4] * s
        got = reg[:, p0:p0 + hw].double()
        for ref, tag in ((torch.exp(prod32.double()), 'fp32 product'), (torch.exp(rr[..., :4].double() * s.double()), 'exact product')):
            ulp = torch.from_numpy(np.spacing(ref.float().abs().numpy())).double()
            e = float(((got - ref).abs() / ulp).max())
            if tag == 'fp32 product':
                worst = max(worst, e)
            else:
                worst_exact = max(worst_exact, e)
    assert torch.equal(d['out'][1], inf_reg)
    print('pack rows=%d C=%d: reg vs float64 exp of the fp32 product %.2f ulp, of the exact product %.2f ulp' % (rows, c, worst, worst_exact))
    assert worst <= 4.0


# ----------------------------------------------------------------------------------------------- (b) glue backward
def _gradients(d, seed):
    """random fp32 gradients, magnitudes log-uniform in [2^-10, 4] with random signs; the regression one divided by the stored
    reg so that dreg * reg * scale * loss_scale stays a normal fp16 number over reg's whole range (e^-7.2 .. e^7.2)"""
    g = torch.Generator().manual_seed(seed)
    p, c = d['p'], d['c']

    def draw(k):
        mag = torch.exp2(torch.rand(2, p, k, generator=g) * 12 - 10)
        return mag * (torch.randint(0, 2, (2, p, k), generator=g).float() * 2 - 1)
    return draw(c), draw(4) / d['out'][1].cpu(), draw(1)


def _run_grad(d, grads, loss_scale, init):
    dcls, dreg, dctr = (t.to(DEV) for t in grads)
    rows = d['rows']
    dys = [(torch.full(t.shape, float('nan'), dtype=torch.float16, device=DEV), torch.full(t.shape, float('nan'), dtype=torch.float16, device=DEV))
           for t in d['dev']['raw_reg']]
    db = [t.to(DEV).clone() for t in init[:3]]
    ds = [t.to(DEV).clone() for t in init[3]]
    ops.fcos_out_grad_levels([dict(raw_reg=r, scale=s, point0=p0, dscale=k, dy_cls=a, dy_reg=b)
                              for r, s, p0, k, (a, b) in zip(d['dev']['raw_reg'], d['dev']['scales'], d['starts'], ds, dys)],
                             dcls, dreg, dctr, d['out'][1], loss_scale, db[0], db[1], db[2])
    assert all(t[0].shape[-1] == rows for t in dys)
    return [(a.cpu(), b.cpu()) for a, b in dys], [t.cpu() for t in db], [t.cpu() for t in ds]


@pytest.mark.parametrize('loss_scale', [1.0, 1024.0])
@pytest.mark.parametrize('rows,c,sizes', CASES + [(32, 3, BIG), (64, 4, BIG)], ids=IDS + ['rows32-big', 'rows64-C4-big'])
def test_grad_levels_vs_float64(rows, c, sizes, loss_scale):
    d = _inputs(rows, c, sizes)
    grads = _gradients(d, 31 + rows + c)
    dcls, dreg, dctr = (t.double() for t in grads)
    reg = d['out'][1].cpu().double()
    g = torch.Generator().manual_seed(5)
    init = [torch.randn(c, generator=g), torch.randn(1, generator=g), torch.randn(4, generator=g), [torch.randn((), generator=g) for _ in sizes]]
    dys, db, ds = _run_grad(d, grads, loss_scale, init)
    dys2, db2, ds2 = _run_grad(d, grads, loss_scale, init)
    pieces = rows // 8
    ref_b = [init[0].double(), init[1].double(), init[2].double()]
    mag_b = [t.abs() for t in ref_b]
    kmax, worst_dy, worst_sum = 0, 0.0, 0.0
    for l, (h, w) in enumerate(sizes):
        p0, hw = d['starts'][l], h * w
        s = d['scales'][l].double()
        rr = d['raw_reg'][l].view(2, hw, rows)[..., :4].double()
        sl = slice(p0, p0 + hw)
        ref_c = torch.zeros(2, hw, rows, dtype=torch.float64)
        ref_c[..., :c] = dcls[:, sl] * loss_scale
        ref_c[..., c] = dctr[:, sl, 0] * loss_scale
        t = dreg[:, sl] * reg[:, sl] * s
        ref_r = torch.zeros(2, hw, rows, dtype=torch.float64)
        ref_r[..., :4] = t * loss_scale
        for got, ref, live in ((dys[l][0].view(2, hw, rows), ref_c, c + 1), (dys[l][1].view(2, hw, rows), ref_r, 4)):
            assert not bool(torch.isnan(got).any()) and bool(torch.isfinite(got).all())
            assert not bool(got[..., live:].any())                                   # padded rows exactly zero
            assert float(ref[..., :live].abs().min()) >= 2.0 ** -14                  # normal fp16 results (see the module docstring)
            err, bound = (got.double() - ref).abs(), (U16 + U32) * ref.abs()
            worst_dy = max(worst_dy, float((err[..., :live] / bound[..., :live]).max()))
            assert bool((err <= bound).all())
        vecs = 2 * hw * pieces
        blocks = min(1024, -(-vecs // 256))
        K = -(-vecs // (256 * blocks)) + 256 // pieces + 4
        kmax = max(kmax, K)
        ref_b[0] = ref_b[0] + dcls[:, sl].sum((0, 1))
        mag_b[0] = mag_b[0] + dcls[:, sl].abs().sum((0, 1))
        ref_b[1] = ref_b[1] + dctr[:, sl].sum((0, 1))
        mag_b[1] = mag_b[1] + dctr[:, sl].abs().sum((0, 1))
        ref_b[2] = ref_b[2] + t.sum((0, 1))
        mag_b[2] = mag_b[2] + t.abs().sum((0, 1))
        a = dreg[:, sl] * reg[:, sl] * rr
        ref_s, mag_s = init[3][l].double() + a.sum(), init[3][l].double().abs() + a.abs().sum()
        e = abs(float(ds[l]) - float(ref_s)) / (K * U32 * float(mag_s))
        worst_sum = max(worst_sum, e)
        assert e <= 1.0, ('dscale', l, e)
        assert float(ds[l]) != float(init[3][l])
    # the bias sums run over all levels: the longest chain is that of the level with the most trips
    for got, ref, mag, i0, name in zip(db, ref_b, mag_b, init[:3], ('dbias_cls', 'dbias_ctr', 'dbias_reg')):
        e = float(((got.double() - ref).abs() / (kmax * U32 * mag)).max())
        worst_sum = max(worst_sum, e)
        assert e <= 1.0, (name, e)
        assert not bool((got == i0).any())                                           # the `+=` moved every element
    print('grad rows=%d C=%d loss_scale=%g: dy max error / bound %.3f; sums max error / bound %.3f (K up to %d)'
          % (rows, c, loss_scale, worst_dy, worst_sum, kmax))
    for (a, b), (a2, b2) in zip(dys, dys2):                                          # two runs, equal bits
        assert torch.equal(a, a2) and torch.equal(b, b2)
    assert all(torch.equal(x, y) for x, y in zip(db + ds, db2 + ds2))
    if sizes is BIG:
        assert 2 * sizes[0][0] * sizes[0][1] * pieces > 1024 * 256                   # the grid-stride walk and capped partial rows ran


# ----------------------------------------------------------------------------------------------- (c) node vs autograd head
def _variant64():
    spec = dict(configs.SIBLINGS['FCOS_FPN'])
    spec['head'] = dict(spec['head'], num_head_channels=64, norm_cfg=dict(type='GroupNorm', num_groups=8))
    spec['neck'] = dict(spec['neck'], num_output_channels=64)
    return configs.build_sibling_model(spec, seed=1)


def _compare_all_gradients(pa, pb, what):
    """every parameter tensor: cosine > 0.9 and norm ratio in (0.8, 1.25) (a reference gradient that is exactly zero: the node's
    is zero too); all gradients as one vector: norm within 3 %, 1 - cosine <= 0.02"""
    worst_cos, worst_ratio, fa, fb = 1.0, 1.0, [], []
    for (k, a), (_, b) in zip(pa, pb):
        assert a.grad is not None and b.grad is not None and a.grad.shape == b.grad.shape, k
        ga, gb = a.grad.double().flatten(), b.grad.double().flatten()
        fa.append(ga)
        fb.append(gb)
        if float(gb.norm()) == 0.0:
            assert float(ga.norm()) == 0.0, k
            continue
        cos = float(ga @ gb / (ga.norm() * gb.norm()))
        ratio = float(ga.norm() / gb.norm())
        worst_cos, worst_ratio = min(worst_cos, cos), max(worst_ratio, ratio, 1 / max(ratio, 1e-300))
        assert cos > _GATES['cos'] and _GATES['ratio'][0] < ratio < _GATES['ratio'][1], (what, k, cos, ratio)
    fa, fb = torch.cat(fa), torch.cat(fb)
    e_norm = abs(float(fa.norm()) - float(fb.norm())) / float(fb.norm())
    e_cos = 1 - float(fa @ fb / (fa.norm() * fb.norm()))
    print('%s: per tensor worst cosine %.6f, worst norm ratio %.4f; whole gradient: norm %.3g, 1 - cosine %.3g'
          % (what, worst_cos, worst_ratio, e_norm, e_cos))
    assert e_norm <= _GATES['norm'] and e_cos <= _GATES['whole_cos'], (what, e_norm, e_cos)


@pytest.mark.parametrize('hw', [(96, 128), (50, 66)], ids=['96x128', 'odd-levels'])
@pytest.mark.parametrize('width', [128, 64])
def test_node_vs_the_autograd_head(width, hw, monkeypatch):
    """one forward + backward under a fixed random linear functional of the three outputs, LFD_HIP_HEAD=1 against 0 (both on the
    pyramid node) from identical state.  (50, 66): levels of 13x17 / 7x9 / 4x5 / 2x3 / 1x2."""
    ma = (configs.build_sibling_model('FCOS_FPN', seed=1) if width == 128 else _variant64()).to(DEV).train()
    mb = copy.deepcopy(ma)
    assert te.fcos_head_supported(ma._backbone, ma._neck, ma._head)
    x = (torch.rand(2, 3, hw[0], hw[1], generator=torch.Generator().manual_seed(7)) * 2 - 1).to(DEV)
    g = torch.Generator().manual_seed(9)
    outs, seeds = {}, None
    for tag, m, env in (('node', ma, '1'), ('autograd', mb, '0')):
        monkeypatch.setenv('LFD_HIP_NECK', '1')
        monkeypatch.setenv('LFD_HIP_HEAD', env)
        o = m(x)
        assert ('_lfd_detector_plan' in m._head.__dict__) == (env == '1')
        if seeds is None:
            seeds = [(torch.randn(t.shape, generator=g) / t.numel() ** 0.5).to(DEV) for t in o]
        sum((t * s).sum() for t, s in zip(o, seeds)).backward()
        outs[tag] = [t.detach() for t in o]
    if hw == (50, 66):
        assert [ma._head_indexes_to_feature_map_sizes[i] for i in range(5)] == [(13, 17), (7, 9), (4, 5), (2, 3), (1, 2)]
    assert ma._head_indexes_to_feature_map_sizes == mb._head_indexes_to_feature_map_sizes
    e_max = e_mean = 0.0
    for i, (a, b) in enumerate(zip(outs['node'], outs['autograd'])):
        assert a.shape == b.shape and a.dtype == torch.float32
        if i == 1:
            assert bool((a > 0).all())
            a, b = a.log(), b.log()
        err = (a - b).abs()
        rel = float(err.max()) / max(1.0, float(b.abs().max()))
        e_max, e_mean = max(e_max, rel), max(e_mean, float(err.mean()))
        assert rel <= _GATES['out_max'] and float(err.mean()) <= _GATES['out_mean'], (i, rel, float(err.mean()))
    print('FCOS width %d %s: cls / log(reg) / ctr max %.3g (relative to max(1, |ref|)), mean %.3g' % (width, hw, e_max, e_mean))
    _compare_all_gradients(list(ma.named_parameters()), list(mb.named_parameters()), 'FCOS width %d %s' % (width, hw))


# ----------------------------------------------------------------------------------------------- (d) whole iterations
def _batch():
    x = (torch.rand(2, 3, 128, 160, generator=torch.Generator().manual_seed(7)) * 2 - 1).to(DEV)
    return x, SC.synth_annotations(5, 2, 128, 160, configs.SIBLINGS['FCOS_FPN']['head']['num_classes'])


def _iteration(model, x, ann):
    model.zero_grad()
    lo = model.get_loss(model(x), ann)
    lo['loss'].backward()
    return float(lo['loss_values']['loss'])


def test_fcos_fpn_iteration_head_node_vs_autograd_head(monkeypatch):
    """get_loss + backward with LFD_HIP_HEAD on and off from identical state: loss 1 %, gradient norm 3 %, 1 - cosine <= 0.02"""
    ma = configs.build_sibling_model('FCOS_FPN', seed=1).to(DEV).train()
    mb = copy.deepcopy(ma)
    x, ann = _batch()
    monkeypatch.setenv('LFD_HIP_NECK', '1')
    monkeypatch.setenv('LFD_HIP_HEAD', '1')
    la = _iteration(ma, x, ann)
    assert '_lfd_detector_plan' in ma._head.__dict__ and '_lfd_pyramid_plan' in ma._neck.__dict__
    monkeypatch.setenv('LFD_HIP_HEAD', '0')
    lb = _iteration(mb, x, ann)
    assert '_lfd_detector_plan' not in mb._head.__dict__ and '_lfd_pyramid_plan' in mb._neck.__dict__
    print('FCOS_FPN loss head node %.6g autograd head %.6g (relative %.3g)' % (la, lb, abs(la - lb) / abs(lb)))
    assert abs(la - lb) <= 0.01 * abs(lb)
    fa = torch.cat([p.grad.double().flatten() for p in ma.parameters()])
    fb = torch.cat([p.grad.double().flatten() for p in mb.parameters()])
    e_norm = abs(float(fa.norm()) - float(fb.norm())) / float(fb.norm())
    e_cos = 1 - float(fa @ fb / (fa.norm() * fb.norm()))
    print('FCOS_FPN whole gradient: norm %.3g, 1 - cosine %.3g' % (e_norm, e_cos))
    assert e_norm <= 0.03 and e_cos <= 0.02
    mc = copy.deepcopy(mb)
    monkeypatch.setenv('LFD_HIP_NECK', '0')          # the head node sits on the pyramid node
    monkeypatch.setenv('LFD_HIP_HEAD', '1')
    mc.zero_grad()
    mc(x)
    assert '_lfd_detector_plan' not in mc._head.__dict__


def test_fcos_fpn_trains_on_the_head_node(monkeypatch):
    monkeypatch.setenv('LFD_HIP_NECK', '1')
    monkeypatch.setenv('LFD_HIP_HEAD', '1')
    model = configs.build_sibling_model('FCOS_FPN', seed=1).to(DEV).train()
    x, ann = _batch()
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        lo = model.get_loss(model(x), ann)
        lo['loss'].backward()
        opt.step()
        losses.append(lo['loss_values']['loss'])
    print('FCOS_FPN losses on the head node', losses)
    assert '_lfd_detector_plan' in model._head.__dict__
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())


def test_head_node_iteration_twice_gives_equal_bits(monkeypatch):
    """no atomics anywhere in the node: every parameter gradient, the head's included, and every buffer"""
    monkeypatch.setenv('LFD_HIP_NECK', '1')
    monkeypatch.setenv('LFD_HIP_HEAD', '1')
    ma = configs.build_sibling_model('FCOS_FPN', seed=1).to(DEV).train()
    mb = copy.deepcopy(ma)
    x, ann = _batch()
    la, lb = _iteration(ma, x, ann), _iteration(mb, x, ann)
    assert la == lb and '_lfd_detector_plan' in ma._head.__dict__
    for (k, a), (_, b) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(a.grad, b.grad), k
    for (k, a), (_, b) in zip(ma.named_buffers(), mb.named_buffers()):
        assert torch.equal(a, b), k


# ----------------------------------------------------------------------------------------------- (e) argument validation
def test_argument_validation_returns_status_codes():
    l = _lib.lib()
    INVALID, SMALL, UNSUPPORTED = -1, -2, -4
    rows, c, hw = 32, 3, 6
    raw = torch.zeros(1, 2, 3, rows, device=DEV)
    dy = torch.zeros(1, 2, 3, rows, dtype=torch.float16, device=DEV)
    dy2 = torch.zeros_like(dy)
    cls, reg, ctr = torch.zeros(1, hw, c, device=DEV), torch.zeros(1, hw, 4, device=DEV), torch.zeros(1, hw, 1, device=DEV)
    sc, dsc = torch.ones((), device=DEV), torch.zeros((), device=DEV)
    db = [torch.zeros(k, device=DEV) for k in (c, 1, 4)]
    ws = ops.train_workspace(torch.device(DEV))
    need = l.lfd_fcos_out_grad_workspace_bytes(1, rows)
    assert need == 1024 * 2 * rows * 4 and l.lfd_fcos_out_grad_workspace_bytes(1, 48) == 0 and ws.numel() >= l.lfd_fcos_out_grad_workspace_bytes(8, 64)
    p = ops.ptr

    def levels(k=1, **kw):
        arr = (_lib.FcosOutLevel * k)()
        for a in arr:
            a.raw_cls, a.raw_reg, a.scale, a.dscale = raw.data_ptr(), raw.data_ptr(), sc.data_ptr(), dsc.data_ptr()
            a.dy_cls, a.dy_reg, a.hw, a.point0 = dy.data_ptr(), dy2.data_ptr(), hw, 0
            for f, v in kw.items():
                setattr(a, f, v)
        return arr

    def pack(lv=None, nlev=1, n=1, rows_=rows, c_=c, P=hw, cls_=cls, reg_=reg, ctr_=ctr):
        return l.lfd_fcos_out_pack_levels_f32(lv if lv is not None else levels(), nlev, n, rows_, c_, P, p(cls_), p(reg_), p(ctr_), None)

    def grad(lv=None, nlev=1, n=1, rows_=rows, c_=c, P=hw, dcls=cls, dreg=reg, dctr=ctr, reg_=reg, dbc=db[0], wsz=None, ws_=ws):
        return l.lfd_fcos_out_grad_levels_f32(lv if lv is not None else levels(), nlev, n, rows_, c_, P, p(dcls), p(dreg), p(dctr), p(reg_),
                                              1.0, p(dbc), p(db[1]), p(db[2]), p(ws_), ws.numel() if wsz is None else wsz, None)

    assert l.lfd_fcos_out_pack_levels_f32(None, 1, 1, rows, c, hw, p(cls), p(reg), p(ctr), None) == INVALID
    assert pack(cls_=None) == INVALID and pack(reg_=None) == INVALID and pack(ctr_=None) == INVALID
    assert pack(levels(raw_cls=None)) == INVALID and pack(levels(raw_reg=None)) == INVALID and pack(levels(scale=None)) == INVALID
    assert pack(levels(raw_reg=raw.data_ptr() + 4)) == INVALID                           # misaligned
    assert pack(rows_=48) == INVALID and pack(rows_=128) == INVALID
    assert pack(c_=rows) == INVALID and pack(c_=0) == INVALID                              # C + 1 > ROWS
    assert pack(levels(9), nlev=9) == INVALID                                              # nlev > LFD_MAX_LEVELS
    assert pack(levels(point0=1)) == INVALID and pack(levels(hw=0)) == INVALID             # outside the concatenated tensor
    assert pack(levels(hw=2 ** 26), P=2 ** 26) == UNSUPPORTED                              # n * hw * ROWS = 2^31
    assert pack(levels(hw=2 ** 25), P=2 ** 25, rows_=64) == UNSUPPORTED
    assert grad(dcls=None) == INVALID and grad(dreg=None) == INVALID and grad(dctr=None) == INVALID and grad(reg_=None) == INVALID
    assert grad(dbc=None) == INVALID and grad(ws_=None) == INVALID
    assert grad(levels(dy_cls=None)) == INVALID and grad(levels(dy_reg=None)) == INVALID and grad(levels(dscale=None)) == INVALID
    assert grad(rows_=16) == INVALID and grad(c_=rows) == INVALID and grad(levels(9), nlev=9) == INVALID
    assert grad(levels(hw=2 ** 26), P=2 ** 26) == UNSUPPORTED
    assert grad(wsz=need - 1) == SMALL
    torch.cuda.synchronize()
    assert not bool(cls.any()) and not bool(reg.any()) and not bool(dy.any()) and not any(bool(t.any()) for t in db)    # nothing ran
    assert pack() == 0 and grad(wsz=need) == 0
    torch.cuda.synchronize()
    assert bool((reg == 1).all())                                                          # expf(0 * 1)
    with pytest.raises(RuntimeError):
        ops.fcos_out_pack_levels([dict(raw_cls=raw, raw_reg=raw, scale=sc, point0=0)], cls, reg.half(), ctr)
    with pytest.raises(RuntimeError):
        ops.fcos_out_pack_levels([dict(raw_cls=raw.cpu(), raw_reg=raw.cpu(), scale=sc.cpu(), point0=0)], cls.cpu(), reg.cpu(), ctr.cpu())
