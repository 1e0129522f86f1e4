"""csrc/head.hip kernel by kernel -- k_head, k_head2 and k_gn_finalize through lfd_head_forward_f16 / lfd_groupnorm_finalize[_fold] /
lfd_head_forward_decode_f16, no model around them -- against the float64 chain of tests/golden/head_cases.py (whose reference,
exactness conditions, gates and walk properties tests/test_head_reference_host.py checks on the CPU):

  * bit for bit (torch.equal) on the integer instrument: the per-tile statistics of pass 1 and pass 2 -- the atomic path of groups of
    4, 2 and 1 channels included -- and cls / reg of the output pass under supplied (a, b), on every case and every variant;
  * within the derived gates on Gaussian operands: statistics, (a, b) and the outputs of the whole five-launch chain, with every
    k_head2 variant bit-identical to the others, the walk cases run twice for the same bits, k_gn_finalize's folded filters equal
    to fp16(fp32(w) a) / hi + lo of the (a, b) it wrote, and both finalize entry points equal;
  * the decoding output pass against lfd_detect_batched on the logits of the plain one;
  * argument validation without a launch.
Every buffer a kernel writes sits between NaN guards, cls / reg with guard rows between the levels, x in front of a NaN guard.
Every knob change goes through `knobs`, which restores the previous value; the last test finds the four knobs at their defaults."""
import contextlib
import ctypes as C
import functools

import pytest
import torch

import head_cases as H
from lfd_amd import _lib, ops

pytestmark = pytest.mark.gpu
STATS = ('partial1', 'partial2')
QUANT = ('partial1', 'ab1', 'partial2', 'ab2', 'cls', 'reg')
RUNS = [(c['name'], 'head2') for c in H.H2_CASES] + [(c['name'], 'head') for c in H.HEAD_CASES]
GAUSS_RUNS = [(n, k) for n, k in RUNS if H.BY_NAME[n]['gauss']]
MEASURED = {}        # (kernel, quantity) -> largest deviation / gate seen, printed by the last test (pytest -s)


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


def _knobs_for(c, kernel, variant='plain'):
    kw = dict(H.VARIANTS[variant]['knobs'])
    if kernel == 'head' and H.uses_head2(c):
        kw['HEAD2'] = 0
    if kernel == 'head2' and c['chunk']:
        kw['H2_CHUNK'] = c['chunk']
    return kw


@functools.lru_cache(maxsize=None)
def _ops(name, kind):
    return H.operands(H.BY_NAME[name], kind)


@functools.lru_cache(maxsize=None)
def _ref(name, kind):
    c, O = H.BY_NAME[name], _ops(name, kind)
    return H.chain(c, O, 'head', ab=O.get('ab'))


def _explain(c, kernel, key, got, ref):
    """name the first element that differs and who computed it, from the restated launch geometry"""
    m = ~torch.isnan(ref)
    bad = ((got.double() != ref) & m).reshape(ref.shape[0], ref.shape[1], -1).any(-1).nonzero()
    if not len(bad):
        return '%s: unwritten / non-finite element' % key
    i, j = bad[0].tolist()
    geo = H.geometry(c)
    if key in STATS:
        l = max(k for k, ts in enumerate(geo['tile_start']) if ts <= i)
        img, t = divmod(i - geo['tile_start'][l], geo['tpi'][l])
        p, where = t * H.TPX, 'tile %d (level %d, image %d, pixels from %d), group %d' % (i, l, img, t * H.TPX, j)
    else:
        l = max(k for k, po in enumerate(geo['p_off']) if po <= j)
        img, p = i, j - geo['p_off'][l]
        where = 'image %d, level %d, pixel %d' % (img, l, p)
    if kernel == 'head2':
        r = [r for r in H.walk_head2(c)['records'] if r['level'] == l and r['image'] == img and r['g0'] <= p // H.GPX < r['g1']][0]
        who = 'block %d, iteration %d, wave %d, groups [%d, %d)' % (r['block'], r['iteration'], r['wave'], r['g0'], r['g1'])
    else:
        w = H.walk_head(c)[c['levels'][l][1]]
        r = [r for r in w['records'] if r['level'] == l and r['image'] == img and r['p0'] == p // H.TPX * H.TPX][0]
        who = 'block %d, tile %d of its range of %d, ring slot %d' % (r['block'], r['pos'], w['per'], r['slot'])
    return '%s: %d rows differ from float64, first at %s: %s' % (key, len(bad), where, who)


def _assert_equal(c, kernel, key, got, ref, what):
    assert H.equal(got, ref), '%s %s' % (what, _explain(c, kernel, key, got, ref))


def _assert_within(kernel, key, got, ref, what):
    gate = H.GATES[kernel][key]
    d = H.deviation(got, ref)
    MEASURED[(kernel, key)] = max(MEASURED.get((kernel, key), (0.0, 0.0)), (d, d / gate))
    print('%s %s: deviation %.3e  gate %.3e' % (what, key, d, gate))
    assert d <= gate, '%s %s: %.3e above the gate %.3e' % (what, key, d, gate)


def _variants(kernel, which):
    if kernel == 'head':
        return ['plain']
    return {'stats': ['plain', 'perm', 'fold_a1'], 'all': list(H.VARIANTS)}[which]


# ------------------------------------------------------------------------------------------------ statistics, exact
@pytest.mark.parametrize('name,kernel', RUNS)
def test_statistics_of_both_passes_equal_float64_on_integers(name, kernel):
    c, O, ref = H.BY_NAME[name], _ops(name, 'int'), _ref(name, 'int')
    for v in _variants(kernel, 'stats'):
        dev = H.Device(c, O, v)
        assert dev.partial_floats == dev.partial.numel == H.geometry(c)['ntiles'] * c['groups'] * 2
        dev.set_ab(O['ab'])
        with knobs(**_knobs_for(c, kernel, v)):
            for p in (1, 2):
                dev.partial.reset()
                assert dev.forward(p) == 0
                _assert_equal(c, kernel, 'partial%d' % p, dev.partial.get(), ref['partial%d' % p], '%s / %s / %s pass %d' % (name, kernel, v, p))
        for t in dev.tower1 + dev.x:
            t.get()
        dev.cls.get(False), dev.reg.get(False)
        assert bool(torch.isnan(dev.cls.t).all()) and bool(torch.isnan(dev.reg.t).all()), 'a statistics pass wrote outputs'


# ------------------------------------------------------------------------------------------------ output pass, exact
@pytest.mark.parametrize('name,kernel', RUNS)
def test_output_pass_under_supplied_affine_equals_float64_on_integers(name, kernel):
    c, O, ref = H.BY_NAME[name], _ops(name, 'int'), _ref(name, 'int')
    for v in _variants(kernel, 'all'):
        dev = H.Device(c, O, v)
        dev.set_ab(O['ab'])
        with knobs(**_knobs_for(c, kernel, v)):
            if H.VARIANTS[v]['a1']:
                assert dev.forward(2) == 0          # leaves conv2's operands for the output pass
            assert dev.forward(3) == 0
        cls, reg = dev.outputs()
        what = '%s / %s / %s' % (name, kernel, v)
        _assert_equal(c, kernel, 'cls', cls, ref['cls'], what)
        _assert_equal(c, kernel, 'reg', reg, ref['reg'], what)
        for t in dev.x + dev.folded + dev.ab:
            t.get()


# ------------------------------------------------------------------------------------------------ the chain, Gaussian
def _check_folded(dev, out, what):
    """k_gn_finalize's folded filters == the fold of the (a, b) it wrote, computed on the CPU, bit for bit"""
    for l, f in enumerate(out.get('folded', [])):
        o = dev.O['levels'][l]
        for k, w in enumerate((o['w1'], o['w2'])):
            for i in range(dev.c['n']):
                want = H.folded_filter(w, out['ab%d' % (k + 1)][l, i]).reshape(-1)
                assert torch.equal(f[k, i].view(torch.int16), want.view(torch.int16)), '%s: folded filter %d of level %d, image %d' % (what, k + 1, l, i)


@pytest.mark.parametrize('name,kernel', GAUSS_RUNS)
def test_five_launch_chain_on_gaussian_operands(name, kernel):
    c, O, ref = H.BY_NAME[name], _ops(name, 'gauss'), _ref(name, 'gauss')
    first = None
    for v in _variants(kernel, 'all'):
        dev = H.Device(c, O, v)
        what = '%s / %s / %s' % (name, kernel, v)
        with knobs(**_knobs_for(c, kernel, v)):
            out = dev.chain()
            if c in H.WALK_CASES and v in ('plain', 'fold_a1'):
                dev.cls.reset(), dev.reg.reset()
                again = dev.chain()
                same = [torch.equal(again[k].view(torch.int32), out[k].view(torch.int32)) for k in QUANT]      # (NaN between the levels)
                assert all(same), what + ': two runs, different bits'
        for k in QUANT:
            _assert_within(kernel, k, out[k], ref[k], what)
        _check_folded(dev, out, what)
        if first is None:
            first = out
        for k in QUANT:       # every k_head2 variant computes the same bits
            assert H.equal(out[k], first[k].double().masked_fill(torch.isnan(ref[k]), float('nan'))), '%s: %s differs from the plain variant' % (what, k)


@pytest.mark.parametrize('name', [c['name'] for c in H.SMALL_CASES + H.ATOMIC_CASES])
def test_both_finalize_entry_points_give_the_same_affine(name):
    c, O = H.BY_NAME[name], _ops(name, 'gauss')
    dev = H.Device(c, O, 'fold')
    with knobs(**_knobs_for(c, 'head2' if H.uses_head2(c) else 'head')):
        assert dev.forward(1) == 0
    assert dev.finalize(1, fold=False) == 0
    plain = dev.ab[0].get().clone()
    for f in dev.folded:
        assert bool(torch.isnan(f.get(False)).all()), 'lfd_groupnorm_finalize wrote folded filters'
    dev.ab[0].reset()
    assert dev.finalize(1, fold=True) == 0
    assert torch.equal(dev.ab[0].get(), plain)
    _assert_within('head2' if H.uses_head2(c) else 'head', 'ab1', plain, _ref(name, 'gauss')['ab1'], name)
    for l, f in enumerate(dev.folded):
        got = f.get(False)
        assert bool(torch.isnan(got[1]).all()) and bool(torch.isfinite(got[0].float()).all())
        for i in range(c['n']):
            want = H.folded_filter(O['levels'][l]['w1'], plain[l, i]).reshape(-1)
            assert torch.equal(got[0, i].view(torch.int16), want.view(torch.int16))


# ------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize('variant', ['plain', 'fold', 'fold_a1'])
def test_decoding_output_pass_equals_detect_batched_on_the_plain_pass(variant):
    c, O = H.BY_NAME['dec'], _ops('dec', 'gauss')
    n = c['n']
    dev = H.Device(c, O, variant)
    out = dev.chain()
    cls, reg = out['cls'].cuda(), out['reg'].cuda()
    thr = float(torch.quantile(cls.sigmoid().reshape(-1), 0.85))
    desc = ops.make_detect_desc([(17, 30), (9, 15), (5, 8), (3, 4)], [8, 16, 32, 64], [(0, 32), (32, 64), (64, 128), (128, 256)], 1, 1, 0, 0,
                                False, 512, thr, 0.5)
    meta = torch.tensor([[240.0, 136.0, 1.0]] * n).cuda()
    want = ops.detect_batched(desc, cls, reg, meta)
    torch.cuda.synchronize()
    fused = ops.detect_outputs(desc, n, cls.device)
    ops.detect_workspace_reset(desc, n, fused)
    dev.cls.reset(), dev.reg.reset()
    for _ in range(2):        # the candidate counters re-arm themselves
        assert dev.decode(desc, meta, fused) == 0
        ops.detect_from_candidates(desc, n, fused)
        torch.cuda.synchronize()
        assert torch.equal(fused.counts, want.counts) and int(want.counts[:, 2].max()) == 0
        for i in range(n):
            k = int(want.counts[i, 1])
            assert k > 3
            assert torch.equal(fused.dets[i, :k], want.dets[i, :k]) and torch.equal(fused.labels[i, :k], want.labels[i, :k])
            assert torch.equal(fused.point[i, :k], want.point[i, :k])
    dev.cls.get(False), dev.reg.get(False)
    assert bool(torch.isnan(dev.cls.t).all()) and bool(torch.isnan(dev.reg.t).all()), 'the decoding pass wrote logits'


# ------------------------------------------------------------------------------------------------ argument validation
def test_argument_validation_without_a_launch():
    c, O = H.BY_NAME['ft2_full'], _ops('ft2_full', 'int')
    dev = H.Device(c, O, 'plain')
    dev.set_ab(O['ab'])
    INVALID, UNSUPPORTED = -1, -4

    def desc(**kw):
        d = _lib.HeadDesc.from_buffer_copy(dev.d)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(d, k)[v[0]] = v[1]
            else:
                setattr(d, k, v)
        return d

    def levels(**kw):
        lv = (_lib.HeadLevelPtrs * len(c['levels']))()
        C.memmove(lv, dev.lv, C.sizeof(lv))
        for k, v in kw.items():
            setattr(lv[1], k, v)
        return lv
    for p in (1, 2, 3):
        assert dev.forward(p, d=desc(head_channels=64)) == UNSUPPORTED
        assert dev.forward(p, d=desc(num_groups=3)) == UNSUPPORTED
        assert dev.forward(p, d=desc(level_cin=(1, 32))) == UNSUPPORTED
        assert dev.forward(p, d=desc(final_reg_rows=2)) == INVALID
    assert dev.forward(3, d=desc(final_cls_rows=61)) == UNSUPPORTED
    assert dev.forward(2, lv=levels(w2_packed=None)) == INVALID and dev.forward(3, lv=levels(w2_packed=None)) == INVALID
    assert dev.forward(3, ab2=False) == INVALID
    assert dev.forward(0) == INVALID and dev.forward(4) == INVALID
    torch.cuda.synchronize()
    for g in [dev.partial, dev.cls, dev.reg]:
        assert bool(torch.isnan(g.get(False)).all()), 'a rejected call wrote'
    assert dev.forward(3) == 0       # the unchanged arguments are fine
    dev.outputs()


# ------------------------------------------------------------------------------------------------ knob hygiene (keep last)
def test_knobs_are_back_at_their_defaults():
    for (kernel, key), (d, frac) in sorted(MEASURED.items()):
        print('measured k_%s %s: %.3e = %.2f of its gate' % (kernel, key, d, frac))
    with pytest.raises(RuntimeError):
        with knobs(HEAD2=0, H2_CHUNK=4):
            assert _lib.tune('HEAD2') == 0 and _lib.tune('H2_CHUNK') == 4
            raise RuntimeError('a failing test')
    for k, v in H.KNOB_DEFAULTS.items():
        assert _lib.tune(k) == v, 'knob %s left at %d' % (k, _lib.tune(k))
