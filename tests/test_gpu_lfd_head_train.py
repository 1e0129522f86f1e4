"""GPU tests of the LFDHead training node (train_engine.DetectorTrainFunction): the glue kernels of csrc/lfd_out.hip per
element against float64 on the CPU, the argument checks, the node against the package's own route with the head under autograd
(LFD_HIP_HEAD=0) from identical state, and whole LFDV2_SFPN iterations.

Bounds of the kernel tests (DESIGN 9f's).  A dy element is ONE fp16 rounding of a correctly rounded fp32 value:
    |got - ref| <= 2^-11 |ref| + 2^-24 |ref|
(the gradients are drawn so that every result is a normal fp16 number).  A reduction is a chain of fp32 additions:
    |got - ref| <= K 2^-24 sum|addends|,   K = trips + 256 / (ROWS / 8) + 4
-- a thread of csrc/lfd_out.hip is a (pixel, conv, 8-row piece) triple and adds `trips` addends per row (its grid-stride walk:
trips = ceil(vecs / (256 blocks)), vecs = n hw convs (ROWS/8), blocks = min(1024, ceil(vecs / 256))), the block partial then adds
the 256 / (convs ROWS/8) <= 256 / (ROWS/8) threads that hold the row, in thread order; + 1 for the rounding of the addend itself (a
product, formed in fp64 and rounded once), + 2 for the final `+=` (the fp64 total rounded to fp32, then added to what the buffer
held, which is counted among the addends), + 1 for the second-order terms and the fp64 additions of the final."""
import copy

import numpy as np
import pytest
import torch

import sibling_cases as SC
from lfd_amd import _lib, configs, ops, train_engine as te
from lfd_head_cases import NODE_CASES, V1_SPEC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U16, U32 = 2.0 ** -11, 2.0 ** -24
# the numbers of tests/test_gpu_pyramid_train.py::_GATES
GATES = dict(out_max=2e-2, out_mean=2e-3, cos=0.9, ratio=(0.8, 1.25), norm=0.03, whole_cos=0.02)
FIVE = [(13, 17), (7, 9), (4, 5), (2, 3), (1, 1)]
BIG = [(168, 200), (3, 5)]          # 2 x 33600 pixels x 8 pieces: more (pixel, piece) pairs than 1024 blocks x 256 threads
N = 2

# (rows, layout, C, scaled, shared, sizes)
CASES = [(rows, 'merged', c, sc, True, FIVE) for rows in (64, 128) for c in (1, 4, 5, 6, rows - 5, rows - 4) for sc in (True, False)]
CASES += [(rows, 'separate', c, sc, True, FIVE) for rows in (64, 128) for c in (1, 3, rows) for sc in (True, False)]
CASES += [(64, 'merged', 5, True, False, FIVE), (128, 'separate', 3, True, False, FIVE)]          # one bias target per level
CASES += [(64, 'merged', 5, True, True, BIG), (128, 'separate', 4, True, True, BIG), (64, 'separate', 3, False, True, BIG),
          (128, 'merged', 123, True, True, BIG)]          # (123: the regression rows straddle two pieces, nothing moves as float4)
IDS = ['rows%d-%s-C%d-%s-%s%s' % (r, lay, c, 'scale' if sc else 'noscale', 'shared' if sh else 'unshared', '-big' if lv is BIG else '')
       for r, lay, c, sc, sh, lv in CASES]

_cache = {}


def _segs(layout, c):
    """per conv of a level: [(kind, row0, channels)]"""
    return [[('cls', 0, c), ('reg', c, 4)]] if layout == 'merged' else [[('cls', 0, c)], [('reg', 0, 4)]]


def _inputs(rows, layout, c, scaled, sizes):
    """seeded raw conv outputs (the padded rows hold values too: nothing may read them), scales, and the forward's outputs --
    computed once per case and shared, never modified"""
    key = (rows, layout, c, scaled, tuple(sizes))
    if key in _cache:
        return _cache[key]
    g = torch.Generator().manual_seed(rows * 1000 + c * 10 + len(sizes) + sizes[0][0] + (layout == 'merged'))
    segs = _segs(layout, c)
    raws = [[torch.randn(N, h, w, rows, generator=g) * 3 for _ in segs] for h, w in sizes]
    scales = [(torch.rand((), generator=g) * 0.4 + 0.8) if scaled else None for _ in sizes]
    starts, p = te._level_starts(sizes)
    d = dict(raws=raws, scales=scales, starts=starts, p=p, sizes=sizes, rows=rows, c=c, segs=segs, scaled=scaled)
    d['dev'] = dict(raws=[[t.to(DEV) for t in lv] for lv in raws], scales=[None if s is None else s.to(DEV) for s in scales])
    cls, reg = (torch.full((N, p, k), float('nan'), device=DEV) for k in (c, 4))
    ops.lfdhead_out_pack_levels(_levels(d), cls, reg)
    d['out'] = (cls, reg)
    _cache[key] = d
    return d


def _levels(d, dys=None, dbias=None, dscale=None, keep_raw=True):
    """the level records of ops.lfdhead_out_*_levels; dbias: per level {kind: tensor}"""
    out = []
    for l in range(len(d['sizes'])):
        convs = []
        for ci, sg in enumerate(d['segs']):
            cv = dict(segs=[dict(kind=k, row0=r0, channels=ch) for k, r0, ch in sg])
            needs = dys is None or (d['scaled'] and any(k == 'reg' for k, _, _ in sg))
            if keep_raw or needs:
                cv['raw'] = d['dev']['raws'][l][ci]
            if dys is not None:
                cv['dy'] = dys[l][ci]
                for s in cv['segs']:
                    s['dbias'] = dbias[l][s['kind']]
            convs.append(cv)
        lv = dict(point0=d['starts'][l], convs=convs, scale=d['dev']['scales'][l])
        if dys is not None and d['scaled']:
            lv['dscale'] = dscale[l]
        out.append(lv)
    return out


def _rows_of(d, l, kind):
    """the raw rows of a level's `kind` segment as [N, hw, channels]"""
    h, w = d['sizes'][l]
    for ci, sg in enumerate(d['segs']):
        for k, r0, ch in sg:
            if k == kind:
                return d['raws'][l][ci].view(N, h * w, d['rows'])[..., r0:r0 + ch]


# ----------------------------------------------------------------------------------------------- (a) glue forward
@pytest.mark.parametrize('rows,layout,c,scaled,shared,sizes', [k for k in CASES if k[4]], ids=[i for i, k in zip(IDS, CASES) if k[4]])
def test_pack_levels_bit_for_bit(rows, layout, c, scaled, shared, sizes):
    """cls: the raw classification rows, bit for bit; reg: the fp32 product raw * scale as torch forms it (the raw rows without a
    Scale); every element written (the outputs start as NaN)"""
    d = _inputs(rows, layout, c, scaled, sizes)
    cls, reg = (t.cpu() for t in d['out'])
    assert not bool(torch.isnan(cls).any() | torch.isnan(reg).any())
    for l, (h, w) in enumerate(sizes):
        sl = slice(d['starts'][l], d['starts'][l] + h * w)
        assert torch.equal(cls[:, sl], _rows_of(d, l, 'cls')), l
        rr = _rows_of(d, l, 'reg')
        assert torch.equal(reg[:, sl], rr * d['scales'][l] if scaled else rr), l


# ----------------------------------------------------------------------------------------------- (b) glue backward
def _gradients(d, seed):
    """random fp32 gradients, magnitudes log-uniform in [2^-10, 4] with random signs"""
    g = torch.Generator().manual_seed(seed)

    def draw(k):
        mag = torch.exp2(torch.rand(N, d['p'], k, generator=g) * 12 - 10)
        return mag * (torch.randint(0, 2, (N, d['p'], k), generator=g).float() * 2 - 1)
    return draw(d['c']), draw(4)


def _run_grad(d, grads, loss_scale, init, shared, keep_raw):
    dcls, dreg = (t.to(DEV) for t in grads)
    nlev = len(d['sizes'])
    dys = [[torch.full(t.shape, float('nan'), dtype=torch.float16, device=DEV) for t in lv] for lv in d['dev']['raws']]
    nb = 1 if shared else nlev
    db = [dict(cls=init['cls'][i].to(DEV).clone(), reg=init['reg'][i].to(DEV).clone()) for i in range(nb)]
    ds = [t.to(DEV).clone() for t in init['scale']]
    ops.lfdhead_out_grad_levels(_levels(d, dys, [db[0 if shared else l] for l in range(nlev)], ds, keep_raw), dcls, dreg, loss_scale)
    return [[t.cpu() for t in lv] for lv in dys], [{k: v.cpu() for k, v in b.items()} for b in db], [t.cpu() for t in ds]


@pytest.mark.parametrize('loss_scale', [1.0, 1024.0])
@pytest.mark.parametrize('rows,layout,c,scaled,shared,sizes', CASES, ids=IDS)
def test_grad_levels_vs_float64(rows, layout, c, scaled, shared, sizes, loss_scale):
    d = _inputs(rows, layout, c, scaled, sizes)
    grads = _gradients(d, 31 + rows + c)
    dcls, dreg = (t.double() for t in grads)
    nlev, pieces, nconvs = len(sizes), rows // 8, len(d['segs'])
    g = torch.Generator().manual_seed(5)
    nb = 1 if shared else nlev
    init = dict(cls=[torch.randn(c, generator=g) for _ in range(nb)], reg=[torch.randn(4, generator=g) for _ in range(nb)],
                scale=[torch.randn((), generator=g) for _ in sizes])
    dys, db, ds = _run_grad(d, grads, loss_scale, init, shared, True)
    dys2, db2, ds2 = _run_grad(d, grads, loss_scale, init, shared, False)       # (and without the raw tensors nobody reads)
    ref_b = [dict(cls=init['cls'][i].double(), reg=init['reg'][i].double()) for i in range(nb)]
    mag_b = [{k: v.abs() for k, v in b.items()} for b in ref_b]
    k_b = [0] * nb
    worst_dy = worst_sum = 0.0
    kmax = 0
    for l, (h, w) in enumerate(sizes):
        hw = h * w
        sl = slice(d['starts'][l], d['starts'][l] + hw)
        s = d['scales'][l].double() if scaled else 1.0
        t = dreg[:, sl] * s                                                             # dL/d(raw regression rows)
        for ci, sg in enumerate(d['segs']):
            ref = torch.zeros(N, hw, rows, dtype=torch.float64)
            live = torch.zeros(rows, dtype=torch.bool)
            for k, r0, ch in sg:
                ref[..., r0:r0 + ch] = (dcls[:, sl] if k == 'cls' else t) * loss_scale
                live[r0:r0 + ch] = True
            got = dys[l][ci].view(N, hw, rows)
            assert not bool(torch.isnan(got).any()) and bool(torch.isfinite(got).all())
            assert not bool(got[..., ~live].any())                                     # padded rows exactly zero
            assert float(ref[..., live].abs().min()) >= 2.0 ** -14                     # normal fp16 results
            err, bound = (got.double() - ref).abs(), (U16 + U32) * ref.abs()
            worst_dy = max(worst_dy, float((err[..., live] / bound[..., live]).max()))
            assert bool((err <= bound).all()), (l, ci)
        vecs = N * hw * nconvs * pieces
        blocks = min(1024, -(-vecs // 256))
        K = -(-vecs // (256 * blocks)) + 256 // pieces + 4
        kmax = max(kmax, K)
        i = 0 if shared else l
        k_b[i] = max(k_b[i], K)           # a bias sum runs over the levels that share it: its longest chain is the largest K
        ref_b[i]['cls'] = ref_b[i]['cls'] + dcls[:, sl].sum((0, 1))
        mag_b[i]['cls'] = mag_b[i]['cls'] + dcls[:, sl].abs().sum((0, 1))
        ref_b[i]['reg'] = ref_b[i]['reg'] + t.sum((0, 1))
        mag_b[i]['reg'] = mag_b[i]['reg'] + t.abs().sum((0, 1))
        if scaled:
            a = dreg[:, sl] * _rows_of(d, l, 'reg').double()
            ref_s, mag_s = init['scale'][l].double() + a.sum(), init['scale'][l].double().abs() + a.abs().sum()
            e = abs(float(ds[l]) - float(ref_s)) / (K * U32 * float(mag_s))
            worst_sum = max(worst_sum, e)
            assert e <= 1.0, ('dscale', l, e)
            assert float(ds[l]) != float(init['scale'][l])                              # the `+=` moved it
        else:
            assert float(ds[l]) == float(init['scale'][l])                              # no Scale: nothing written
    for i in range(nb):
        for k in ('cls', 'reg'):
            e = float(((db[i][k].double() - ref_b[i][k]).abs() / (k_b[i] * U32 * mag_b[i][k])).max())
            worst_sum = max(worst_sum, e)
            assert e <= 1.0, ('dbias', i, k, e)
            assert not bool((db[i][k] == init[k][i]).any())                             # the `+=` moved every element
    print('grad rows=%d %s C=%d scale=%d shared=%d loss_scale=%g: dy max error / bound %.3f; sums max error / bound %.3f (K up to %d)'
          % (rows, layout, c, scaled, shared, loss_scale, worst_dy, worst_sum, kmax))
    for lv, lv2 in zip(dys, dys2):                                                      # two runs, equal bits
        assert all(torch.equal(a, b) for a, b in zip(lv, lv2))
    assert all(torch.equal(a[k], b[k]) for a, b in zip(db, db2) for k in a) and all(torch.equal(a, b) for a, b in zip(ds, ds2))
    if sizes is BIG:
        assert N * sizes[0][0] * sizes[0][1] * pieces > 1024 * 256                      # the grid-stride walk and capped partial rows ran


# ----------------------------------------------------------------------------------------------- (c) argument validation
def test_argument_validation_returns_status_codes():
    l = _lib.lib()
    INVALID, SMALL, UNSUPPORTED = -1, -2, -4
    rows, c, hw = 64, 3, 6
    raw = torch.zeros(1, 2, 3, rows, device=DEV)
    dy = torch.zeros(1, 2, 3, rows, dtype=torch.float16, device=DEV)
    cls, reg = torch.zeros(1, hw, c, device=DEV), torch.zeros(1, hw, 4, device=DEV)
    sc, dsc = torch.full((), 2.0, device=DEV), torch.zeros((), device=DEV)
    db = [torch.zeros(k, device=DEV) for k in (c, 4)]
    ws = ops.train_workspace(torch.device(DEV))
    need = l.lfd_lfdhead_out_grad_workspace_bytes(1, rows)
    assert need == 1024 * 2 * 2 * rows * 4 and ws.numel() >= l.lfd_lfdhead_out_grad_workspace_bytes(8, 128)
    p = ops.ptr

    def levels(k=1, lv=None, conv=None, seg0=None, seg1=None):
        arr = (_lib.LfdHeadOutLevel * k)()
        for a in arr:
            a.scale, a.dscale, a.hw, a.nconvs, a.point0 = sc.data_ptr(), dsc.data_ptr(), hw, 1, 0
            cv = a.convs[0]
            cv.raw, cv.dy, cv.nsegs = raw.data_ptr(), dy.data_ptr(), 2
            cv.segs[0].dbias, cv.segs[0].row0, cv.segs[0].channels, cv.segs[0].kind = db[0].data_ptr(), 0, c, 0
            cv.segs[1].dbias, cv.segs[1].row0, cv.segs[1].channels, cv.segs[1].kind = db[1].data_ptr(), c, 4, 1
            for obj, kw in ((a, lv), (cv, conv), (cv.segs[0], seg0), (cv.segs[1], seg1)):
                for f, v in (kw or {}).items():
                    setattr(obj, f, v)
        return arr

    def pack(lv=None, nlev=1, n=1, rows_=rows, c_=c, P=hw, cls_=cls, reg_=reg):
        return l.lfd_lfdhead_out_pack_levels_f32(lv if lv is not None else levels(), nlev, n, rows_, c_, P, p(cls_), p(reg_), None)

    def grad(lv=None, nlev=1, n=1, rows_=rows, c_=c, P=hw, dcls=cls, dreg=reg, wsz=None, ws_=ws):
        return l.lfd_lfdhead_out_grad_levels_f32(lv if lv is not None else levels(), nlev, n, rows_, c_, P, p(dcls), p(dreg), 1.0, p(ws_),
                                                 ws.numel() if wsz is None else wsz, None)

    import ctypes as C
    off = lambda t, k: C.c_void_p(t.data_ptr() + k)          # noqa: E731
    # null pointers
    assert l.lfd_lfdhead_out_pack_levels_f32(None, 1, 1, rows, c, hw, p(cls), p(reg), None) == INVALID
    assert pack(cls_=None) == INVALID and pack(reg_=None) == INVALID and pack(levels(conv=dict(raw=None))) == INVALID
    assert grad(dcls=None) == INVALID and grad(dreg=None) == INVALID and grad(ws_=None) == INVALID
    assert grad(levels(conv=dict(dy=None))) == INVALID and grad(levels(seg0=dict(dbias=None))) == INVALID
    assert grad(levels(seg1=dict(dbias=None))) == INVALID
    assert grad(levels(lv=dict(dscale=None))) == INVALID and grad(levels(lv=dict(scale=None))) == INVALID      # one without the other
    assert grad(levels(conv=dict(raw=None))) == INVALID                                  # a Scale gradient needs the raw rows
    # rows not 64 | 128
    assert pack(rows_=32) == INVALID and pack(rows_=96) == INVALID and grad(rows_=32) == INVALID and grad(rows_=256) == INVALID
    # a segment past `rows`, overlapping / missing / doubled segments, wrong channel counts
    assert pack(levels(seg1=dict(row0=rows - 3))) == INVALID and grad(levels(seg1=dict(row0=rows - 3))) == INVALID
    assert pack(levels(seg0=dict(row0=-1))) == INVALID and pack(levels(seg1=dict(row0=c - 1))) == INVALID
    assert pack(levels(seg1=dict(kind=0))) == INVALID and pack(levels(seg1=dict(kind=2))) == INVALID
    assert pack(levels(conv=dict(nsegs=1))) == INVALID and pack(levels(conv=dict(nsegs=3))) == INVALID
    assert pack(levels(seg1=dict(channels=3))) == INVALID and pack(c_=c + 1) == INVALID and pack(c_=0) == INVALID
    assert pack(levels(lv=dict(nconvs=0))) == INVALID and pack(levels(lv=dict(nconvs=3))) == INVALID
    # a level past points_total, level counts
    assert pack(levels(lv=dict(point0=1))) == INVALID and pack(levels(lv=dict(hw=0))) == INVALID and pack(P=hw - 1) == INVALID
    assert grad(levels(lv=dict(point0=1))) == INVALID
    assert pack(levels(9), nlev=9) == INVALID and pack(nlev=0) == INVALID and pack(n=0) == INVALID and grad(levels(9), nlev=9) == INVALID
    # misaligned pointers
    assert pack(levels(conv=dict(raw=raw.data_ptr() + 4))) == INVALID and grad(levels(conv=dict(dy=dy.data_ptr() + 2))) == INVALID
    assert l.lfd_lfdhead_out_pack_levels_f32(levels(), 1, 1, rows, c, hw, p(cls), off(reg, 4), None) == INVALID
    assert l.lfd_lfdhead_out_grad_levels_f32(levels(), 1, 1, rows, c, hw, p(cls), off(reg, 4), 1.0, p(ws), ws.numel(), None) == INVALID
    assert l.lfd_lfdhead_out_grad_levels_f32(levels(), 1, 1, rows, c, hw, p(cls), p(reg), 1.0, off(ws, 4), ws.numel() - 4, None) == INVALID
    # 32-bit indices, workspace
    assert pack(levels(lv=dict(hw=2 ** 25)), P=2 ** 25) == UNSUPPORTED                    # n * hw * ROWS = 2^31
    assert pack(levels(lv=dict(hw=2 ** 24)), P=2 ** 24, rows_=128) == UNSUPPORTED
    assert grad(levels(lv=dict(hw=2 ** 25)), P=2 ** 25) == UNSUPPORTED
    assert grad(wsz=need - 1) == SMALL
    torch.cuda.synchronize()
    assert not bool(cls.any()) and not bool(reg.any()) and not bool(dy.any()) and not any(bool(t.any()) for t in db)    # nothing ran
    raw.fill_(1.5)
    assert pack() == 0
    torch.cuda.synchronize()
    assert bool((cls == 1.5).all()) and bool((reg == 3.0).all())
    assert grad(wsz=need) == 0
    torch.cuda.synchronize()
    assert bool((db[0] == 1.5 * hw).all()) and bool((db[1] == 6.0 * hw).all()) and float(dsc) == 3.0 * 1.5 * 4 * hw
    with pytest.raises(RuntimeError):
        ops.lfdhead_out_pack_levels([dict(point0=0, scale=sc, convs=[dict(raw=raw, segs=[dict(kind='cls', row0=0, channels=c),
                                                                                          dict(kind='reg', row0=c, channels=4)])])],
                                    cls, reg.half())
    with pytest.raises(RuntimeError):
        ops.lfdhead_out_pack_levels([dict(point0=0, scale=None, convs=[dict(raw=raw.cpu(), segs=[dict(kind='cls', row0=0, channels=c),
                                                                                                   dict(kind='reg', row0=c, channels=4)])])],
                                    cls.cpu(), reg.cpu())


# ----------------------------------------------------------------------------------------------- (d) node vs autograd head
def _compare_all_gradients(pa, pb, what):
    """every parameter tensor, the head's too: cosine > 0.9 and norm ratio in (0.8, 1.25) (a reference gradient that is exactly
    zero: the node's is zero too); all gradients as one vector: norm within 3 %, 1 - cosine <= 0.02"""
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
        assert cos > GATES['cos'] and GATES['ratio'][0] < ratio < GATES['ratio'][1], (what, k, cos, ratio)
    fa, fb = torch.cat(fa), torch.cat(fb)
    e_norm = abs(float(fa.norm()) - float(fb.norm())) / float(fb.norm())
    e_cos = 1 - float(fa @ fb / (fa.norm() * fb.norm()))
    print('%s: per tensor worst cosine %.6f, worst norm ratio %.4f; whole gradient: norm %.3g, 1 - cosine %.3g'
          % (what, worst_cos, worst_ratio, e_norm, e_cos))
    assert e_norm <= GATES['norm'] and e_cos <= GATES['whole_cos'], (what, e_norm, e_cos)


@pytest.mark.parametrize('hw', [(96, 128), (50, 66)], ids=['96x128', 'odd-levels'])
@pytest.mark.parametrize('case', list(NODE_CASES))
def test_node_vs_the_autograd_head(case, hw, monkeypatch):
    """one forward + backward under a fixed random linear functional of (cls, reg), LFD_HIP_HEAD=1 against 0 (both on the pyramid
    node) from identical state.  (50, 66): levels of 13x17 / 7x9 / 4x5 / 2x3 (/ 1x2 on the five-output FPN)."""
    ma = configs.build_sibling_model(NODE_CASES[case], seed=1).to(DEV).train()
    mb = copy.deepcopy(ma)
    assert te.lfd_head_supported(ma._backbone, ma._neck, ma._head)
    x = (torch.rand(2, 3, hw[0], hw[1], generator=torch.Generator().manual_seed(7)) * 2 - 1).to(DEV)
    g = torch.Generator().manual_seed(9)
    outs, seeds = {}, None
    for tag, m, env in (('node', ma, '1'), ('autograd', mb, '0')):
        monkeypatch.setenv('LFD_HIP_NECK', '1')
        monkeypatch.setenv('LFD_HIP_HEAD', env)
        o = m(x)
        assert len(o) == 2 and ('_lfd_detector_plan' in m._head.__dict__) == (env == '1')
        if seeds is None:
            seeds = [(torch.randn(t.shape, generator=g) / t.numel() ** 0.5).to(DEV) for t in o]
        sum((t * s).sum() for t, s in zip(o, seeds)).backward()
        outs[tag] = [t.detach() for t in o]
    nlev = ma._neck._num_outputs
    if hw == (50, 66):
        assert [ma._head_indexes_to_feature_map_sizes[i] for i in range(nlev)] == [(13, 17), (7, 9), (4, 5), (2, 3), (1, 2)][:nlev]
    assert ma._head_indexes_to_feature_map_sizes == mb._head_indexes_to_feature_map_sizes
    e_max = e_mean = 0.0
    for i, (a, b) in enumerate(zip(outs['node'], outs['autograd'])):
        assert a.shape == b.shape and a.dtype == torch.float32
        err = (a - b).abs()
        rel = float(err.max()) / max(1.0, float(b.abs().max()))
        e_max, e_mean = max(e_max, rel), max(e_mean, float(err.mean()))
        assert rel <= GATES['out_max'] and float(err.mean()) <= GATES['out_mean'], (i, rel, float(err.mean()))
    assert outs['node'][0].size(2) == ma._head.num_cls_channels and outs['node'][1].size(2) == 4
    print('LFD %s %s: cls / reg max %.3g (relative to max(1, |ref|)), mean %.3g' % (case, hw, e_max, e_mean))
    _compare_all_gradients(list(ma.named_parameters()), list(mb.named_parameters()), 'LFD %s %s' % (case, hw))
    for (k, a), (_, b) in zip(ma.named_buffers(), mb.named_buffers()):
        if k.endswith('num_batches_tracked'):
            assert int(a) == int(b) == 1, k
        elif k.startswith(('_neck.', '_head.')):          # running statistics move as on the other route
            assert float((a - b).abs().max()) <= 2e-3 * max(1.0, float(b.abs().max())), k


# ----------------------------------------------------------------------------------------------- (e) whole iterations
NAME = 'LFDV2_SFPN'


def _batch():
    x = (torch.rand(2, 3, 128, 160, generator=torch.Generator().manual_seed(7)) * 2 - 1).to(DEV)
    return x, SC.synth_annotations(5, 2, 128, 160, configs.SIBLINGS[NAME]['head']['num_classes'])


def _iteration(model, x, ann):
    model.zero_grad()
    lo = model.get_loss(model(x), ann)
    lo['loss'].backward()
    return float(lo['loss_values']['loss'])


def test_lfdv2_sfpn_iteration_head_node_vs_autograd_head(monkeypatch):
    """get_loss + backward with LFD_HIP_HEAD on and off from identical state: loss 1 %, gradient norm 3 %, 1 - cosine <= 0.02;
    with the switch on the head carries its detector plan (it carries none on the parent commit, nor with the switch off)"""
    ma = configs.build_sibling_model(NAME, seed=1).to(DEV).train()
    mb = copy.deepcopy(ma)
    x, ann = _batch()
    monkeypatch.setenv('LFD_HIP_NECK', '1')
    monkeypatch.setenv('LFD_HIP_HEAD', '1')
    la = _iteration(ma, x, ann)
    assert te.lfd_head_supported(ma._backbone, ma._neck, ma._head)
    assert '_lfd_detector_plan' in ma._head.__dict__ and '_lfd_pyramid_plan' in ma._neck.__dict__
    monkeypatch.setenv('LFD_HIP_HEAD', '0')
    lb = _iteration(mb, x, ann)
    assert '_lfd_detector_plan' not in mb._head.__dict__ and '_lfd_pyramid_plan' in mb._neck.__dict__
    print('LFDV2_SFPN loss head node %.6g autograd head %.6g (relative %.3g)' % (la, lb, abs(la - lb) / abs(lb)))
    assert abs(la - lb) <= 0.01 * abs(lb)
    fa = torch.cat([p.grad.double().flatten() for p in ma.parameters()])
    fb = torch.cat([p.grad.double().flatten() for p in mb.parameters()])
    e_norm = abs(float(fa.norm()) - float(fb.norm())) / float(fb.norm())
    e_cos = 1 - float(fa @ fb / (fa.norm() * fb.norm()))
    print('LFDV2_SFPN whole gradient: norm %.3g, 1 - cosine %.3g' % (e_norm, e_cos))
    assert e_norm <= 0.03 and e_cos <= 0.02
    monkeypatch.setenv('LFD_HIP_NECK', '0')          # the head node sits on the pyramid node: LFD._forward_train asks for both
    monkeypatch.setenv('LFD_HIP_HEAD', '1')
    sw = te.switches()
    assert sw.hip_head and not sw.hip_neck


def test_lfdv2_sfpn_trains_on_the_head_node(monkeypatch):
    monkeypatch.setenv('LFD_HIP_NECK', '1')
    monkeypatch.setenv('LFD_HIP_HEAD', '1')
    model = configs.build_sibling_model(NAME, seed=1).to(DEV).train()
    x, ann = _batch()
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        lo = model.get_loss(model(x), ann)
        lo['loss'].backward()
        opt.step()
        losses.append(lo['loss_values']['loss'])
    print('LFDV2_SFPN losses on the head node', losses)
    assert '_lfd_detector_plan' in model._head.__dict__
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())


def test_head_node_iteration_twice_gives_equal_bits(monkeypatch):
    """no atomics anywhere in the node: every parameter gradient, the head's included, and every buffer"""
    monkeypatch.setenv('LFD_HIP_NECK', '1')
    monkeypatch.setenv('LFD_HIP_HEAD', '1')
    ma = configs.build_sibling_model(NAME, seed=1).to(DEV).train()
    mb = copy.deepcopy(ma)
    x, ann = _batch()
    la, lb = _iteration(ma, x, ann), _iteration(mb, x, ann)
    assert la == lb and '_lfd_detector_plan' in ma._head.__dict__
    for (k, a), (_, b) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(a.grad, b.grad), k
    for (k, a), (_, b) in zip(ma.named_buffers(), mb.named_buffers()):
        assert torch.equal(a, b), k


def test_a_head_the_node_does_not_admit_keeps_the_pyramid_route(monkeypatch):
    """LFDHeadV1 (BatchNorm towers, per-level output convs) behind the SimpleFPN: the pyramid node with the head under autograd,
    silently; the iteration completes with finite gradients"""
    monkeypatch.setenv('LFD_HIP_NECK', '1')
    monkeypatch.setenv('LFD_HIP_HEAD', '1')
    model = configs.build_sibling_model(V1_SPEC, seed=1).to(DEV).train()
    assert not te.lfd_head_supported(model._backbone, model._neck, model._head)
    x, _ = _batch()
    ann = SC.synth_annotations(5, 2, 128, 160, V1_SPEC['head']['num_classes'])
    loss = _iteration(model, x, ann)
    assert np.isfinite(loss)
    assert '_lfd_detector_plan' not in model._head.__dict__ and '_lfd_pyramid_plan' in model._neck.__dict__
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())
