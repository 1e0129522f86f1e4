"""CPU checks of tests/golden/head_cases.py, the instrument behind tests/test_gpu_head_exact.py:

  * its float64 reference is pinned to torch's own double conv1d / group_norm chain (without the fp16 rounding points);
  * every exact case keeps the conditions under which k_head and k_head2 must reproduce float64 BIT FOR BIT -- every value stored in
    fp16 survives the store, every bound on a partial sum or sum of squares fits 24 bits, every bias is an fp16 hi + lo -- and the
    float32 emulations of both kernels' forms in two K orders equal float64;
  * the gates are re-derived from those emulations on the Gaussian cases;
  * every case has the walk properties it is in the table for, from the launch geometry restated in head_cases.py;
  * the restated constants still match csrc/head.hip and lfd_amd/_lib.py;
  * the comparisons resolve the bugs they are meant to catch: seven references wrong in exactly one way each fail them.
Prints the figures (pytest -s)."""
import functools
import os
import re

import pytest
import torch
import torch.nn.functional as F

import head_cases as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'lfd-a-light-and-fast-detector_amd')
OUT = ('cls', 'reg')
ALL = ('partial1', 'partial2', 'cls', 'reg')
NAMES = [c['name'] for c in H.ALL_CASES]
GAUSS = [c['name'] for c in H.ALL_CASES if c['gauss']]
LIGHT = [c['name'] for c in H.SMALL_CASES + H.ATOMIC_CASES]      # the wrong references run on the small cases


@functools.lru_cache(maxsize=None)
def _ops(name, kind):
    return H.operands(H.BY_NAME[name], kind)


@functools.lru_cache(maxsize=None)
def _ref(name, kind):
    c, O = H.BY_NAME[name], _ops(name, kind)
    return H.chain(c, O, 'head', ab=O.get('ab'), caps=kind == 'int')


# ------------------------------------------------------------------------------------------------ the reference is right
def test_reference_is_the_double_conv_and_group_norm_chain():
    c = H.case('tiny', 2, [(37, 64), (5, 128)], groups=8, rows=(4, 7), seed=40)
    O, geo = H.operands(c, 'gauss'), H.geometry(c)
    r = H.chain(c, O, 'head', round16=False)
    for l, ((hw, cin), o) in enumerate(zip(c['levels'], O['levels'])):
        x = o['x'].double().permute(0, 2, 1)

        def conv(t, w, b=None):
            return F.conv1d(t, w.double()[:, :, None], None if b is None else b.double())
        t = conv(x, o['wn'], o['bn']).relu()
        c1 = conv(t, o['w1'])
        t = F.group_norm(c1, 8, o['gamma1'].double(), o['beta1'].double(), H.EPS).relu()
        c2 = conv(t, o['w2'])
        t = F.group_norm(c2, 8, o['gamma2'].double(), o['beta2'].double(), H.EPS).relu()
        out = conv(t, o['wf'], o['bf']).permute(0, 2, 1)
        po = geo['p_off'][l]
        assert float((r['reg'][:, po:po + hw] - out[..., :4] * float(torch.tensor(o['scale']).float())).abs().max()) < 1e-9
        assert float((r['cls'][:, po:po + hw] - out[..., 4:]).abs().max()) < 1e-9
        # the statistics, per tile, in the layout of the partial buffer: tiles level-major, then image
        for name, cv in (('partial1', c1), ('partial2', c2)):
            for i in range(2):
                for t_ in range(geo['tpi'][l]):
                    v = cv[i, :, t_ * 64:min(t_ * 64 + 64, hw)].reshape(8, 16, -1)
                    want = torch.stack([v.sum((1, 2)), (v * v).sum((1, 2))], -1)
                    got = r[name][geo['tile_start'][l] + i * geo['tpi'][l] + t_]
                    assert float((got - want).abs().max()) < 1e-9
    assert bool(torch.isnan(r['cls'][:, geo['p_off'][0] + 37:geo['p_off'][1]]).all())
    # ... and with the rounding points it differs from that chain by fp16 roundings only
    d = H.deviation(H.chain(c, O, 'head')['cls'], r['cls'])
    assert 0 < d < 1e-2


def test_supplied_affine_and_the_second_form():
    """the two forms differ on general data (rows rounded as fp16(w a), biases as hi + lo) and by no more than those roundings"""
    c = H.BY_NAME['sizes3']
    O = _ops('sizes3', 'gauss')
    a, b = H.chain(c, O, 'head'), H.chain(c, O, 'head2')
    for k in OUT:
        assert 0 < H.deviation(b[k], a[k]) < 2e-2
    # supplied (a, b): the chain's own statistics as an argument give the chain's own outputs
    ab = torch.stack([a['ab1'], a['ab2']])
    again = H.chain(c, O, 'head', ab=ab)
    assert all(H.equal(again[k], a[k]) for k in ALL)


# ------------------------------------------------------------------------------------------------ exactness conditions
@pytest.mark.parametrize('name', NAMES)
def test_exact_conditions(name):
    c, O, r = H.BY_NAME[name], _ops(name, 'int'), _ref(name, 'int')
    assert r['round_err'] == 0.0, 'a value stored in fp16 does not survive the store'
    assert r['cap'] < 2.0 ** 24, 'a partial sum may leave the 24 bits of fp32'
    needs_lo = False
    for o in O['levels']:
        for k in ('bn', 'bf'):
            full, hi = H.hilo(o[k])
            assert torch.equal(full, o[k].double()), 'a bias is not an fp16 hi + lo'
            needs_lo = needs_lo or not torch.equal(hi, o[k].double())
    assert needs_lo, 'no bias of the case needs its lo half'
    ab = O['ab']
    assert bool((ab[..., 0].log2() == ab[..., 0].log2().round()).all()) and bool((ab[..., 1] == ab[..., 1].round()).all())
    assert c['n'] == 1 or not torch.equal(ab[:, :, 0], ab[:, :, 1]), 'every image has its own (a, b)'
    big = name not in LIGHT        # the large walk cases: one K order per form (the operands come from the same generator)
    for form in ('head', 'head2'):
        for ks in (((1,) if form == 'head' else (2,)) if big else ((None, 1, 2) if form == 'head2' else (1, 2))):
            e = H.chain(c, O, form, torch.float32 if ks else torch.float64, kseed=ks, ab=ab)
            for k in ALL:
                assert H.equal(e[k], r[k]), '%s: %s emulation (K order %s) differs from float64 in %s' % (name, form, ks, k)
    print('%s: cap 2^%.1f' % (name, torch.log2(torch.tensor(r['cap']))))


# ------------------------------------------------------------------------------------------------ gates
@functools.lru_cache(maxsize=None)
def _emulation_figures():
    fig = {}
    for name in GAUSS:
        c, O, r = H.BY_NAME[name], _ops(name, 'gauss'), _ref(name, 'gauss')
        for form in ('head', 'head2'):
            for ks in (1, 2):
                e = H.chain(c, O, form, torch.float32, kseed=ks)
                for k in H.GATES[form]:
                    fig[(form, k)] = max(fig.get((form, k), 0.0), H.deviation(e[k], r[k]))
    return fig


@pytest.mark.parametrize('form', ['head', 'head2'])
def test_gates_are_four_times_the_emulations(form):
    fig = _emulation_figures()
    for k, gate in H.GATES[form].items():
        print('%s %s: emulation %.3e  gate %.3e  (gate / figure %.2f)' % (form, k, fig[(form, k)], gate, gate / fig[(form, k)]))
    for k, gate in H.GATES[form].items():
        f = fig[(form, k)]
        assert f <= gate / 4, 'an emulation exceeds a quarter of the gate'
        assert gate <= 8 * f, 'the gate is slacker than the derivation allows'


# ------------------------------------------------------------------------------------------------ walk properties
def _by_block(recs, key='block'):
    out = {}
    for r in recs:
        out.setdefault(r[key], []).append(r)
    return out


def _h2_props(c):
    w = H.walk_head2(c)
    recs, props = w['records'], set()
    for it in _by_block(recs, 'item').values():
        imgs = set(r['image'] for r in it if r['image'] is not None)
        assert imgs, 'an item without work'
        if len(imgs) > 1:
            props.add('straddle')
        if any(r['image'] is None for r in it):
            props.add('idle')
        assert len(set(r['level'] for r in it)) == 1        # a workgroup is on one level at a time
    for b in _by_block(recs).values():
        iters = sorted(set(r['iteration'] for r in b))
        if len(iters) >= 3:
            props.add('three_items')
        lv = [next(r['level'] for r in b if r['iteration'] == i) for i in iters]
        for x, y in zip(lv, lv[1:]):
            if x != y:
                props.add('level_switch')
                if c['levels'][x][1] != c['levels'][y][1]:
                    props.add('cin_switch')
    # every group of every (level, image) exactly once, chunks start on statistics tiles
    seen = {}
    for r in recs:
        if r['image'] is not None:
            assert r['g0'] % 2 == 0 and r['g1'] > r['g0']
            for g in range(r['g0'], r['g1']):
                key = (r['level'], r['image'], g)
                assert key not in seen
                seen[key] = r['item']
    want = sum(c['n'] * ((hw + 31) // 32) for hw, _ in c['levels'])
    assert len(seen) == want == sum(r['g1'] - r['g0'] for r in recs if r['image'] is not None)
    for l, (hw, _) in enumerate(c['levels']):
        if ((hw + 31) // 32) % 2:
            props.add('odd_groups')
        if hw % 32:
            props.add('tail_group')
    props.add('chunk%d' % max(w['chunk']))
    return props, w


H2_CLAIMS = {
    'sizes3': {'straddle', 'idle', 'odd_groups', 'tail_group', 'chunk2'},
    'sizes1': {'idle', 'odd_groups', 'tail_group', 'chunk2'},
    'sizes1_c4': {'chunk4', 'idle'},
    'sizes1_c12': {'chunk12', 'idle'},
    'g8_ft2': {'straddle', 'tail_group'},
    'ft2_full': {'straddle', 'idle', 'odd_groups'},
    'walk_c2': {'three_items', 'straddle', 'odd_groups', 'tail_group', 'chunk2'},
    'walk_plan': {'chunk6', 'straddle'},
    'switch': {'level_switch', 'cin_switch', 'chunk2'},
}


@pytest.mark.parametrize('name', [c['name'] for c in H.H2_CASES])
def test_k_head2_walk_properties(name):
    c = H.BY_NAME[name]
    props, w = _h2_props(c)
    print('%s: %d items on %d blocks, chunks %s: %s' % (name, w['nitems'], w['blocks'], w['chunk'], sorted(props)))
    assert H2_CLAIMS.get(name, set()) <= props
    if name == 'walk_c2':
        assert w['nitems'] > 2 * H.H2_BLOCKS and w['nitems'] < 2 * H.H2_BLOCKS + 8      # the smallest level that gets there
    if name == 'dec':
        assert c['contiguous'] and (c['reg_rows'], c['cls_rows']) == (4, 1) and H.geometry(c)['P'] == sum(hw for hw, _ in c['levels'])


def test_k_head2_cases_cover_the_sizes_and_variants():
    sizes = set(hw for c in H.SMALL_CASES for hw, _ in c['levels'])
    assert {1, 31, 32, 33, 63, 64, 65, 96, 127, 510} <= sizes
    assert {1, 3} <= set(c['n'] for c in H.SMALL_CASES) and {8, 4, 16} <= set(c['groups'] for c in H.SMALL_CASES)
    for cin in (64, 128):
        assert {1, 33, 510} & set(hw for c in H.SMALL_CASES for hw, ci in c['levels'] if ci == cin)
    assert [ci for _, ci in H.BY_NAME['sizes1']['levels']] == [64, 64, 128, 128] == [ci for _, ci in H.BY_NAME['switch']['levels']]
    rows = set((c['reg_rows'], c['cls_rows']) for c in H.SMALL_CASES)
    assert {(4, 1), (4, 28), (4, 29), (4, 60), (0, 5), (0, 33), (4, 0)} <= rows
    assert {True, False} == set(c['scale'] for c in H.SMALL_CASES)
    assert set(H.final_tiles(c) for c in H.SMALL_CASES) == {1, 2}
    assert {32, 64, 128} == set(c['groups'] for c in H.ATOMIC_CASES)
    assert all(not H.uses_head2(c) for c in H.ATOMIC_CASES) and all(H.uses_head2(c) for c in H.H2_CASES)


def _head_props(c):
    out = {}
    for cin, w in H.walk_head(c).items():
        props, blocks = set(), _by_block(w['records'])
        assert w['per'] == max(len(b) for b in blocks.values())
        last = blocks[max(blocks)]
        if len(last) < w['per']:
            props.add('short_last')
        if len(blocks) < w['grid']:
            props.add('empty_blocks')
        for b in blocks.values():
            assert [r['pos'] for r in b] == list(range(len(b)))
            if len(set(r['image'] for r in b if r['level'] == b[0]['level'])) > 1:
                props.add('crosses_image')
            if len(set(r['level'] for r in b)) > 1:
                props.add('crosses_level')
            if len(b) > H.RING[cin]:
                props.add('ring_wraps')
        if any(r['tail'] for r in w['records']):
            props.add('tail_tile')
        out[cin] = (w['per'], props)
    return out


@pytest.mark.parametrize('name', [c['name'] for c in H.RING_CASES])
def test_k_head_walk_properties(name):
    got = _head_props(H.BY_NAME[name])
    print(name, got)
    for cin, per in zip((64, 128), H.RING_PER[name]):
        if per is None:
            assert cin not in got
            continue
        assert got[cin][0] == per
        assert 'tail_tile' in got[cin][1]
        if per > 1:
            assert {'crosses_image', 'crosses_level'} <= got[cin][1]
    if name in ('ring_per2', 'ring_per4', 'ring_per5', 'ring_per6'):
        assert 'short_last' in got[64][1]
    if name in ('ring_per5', 'ring_per6'):
        assert 'ring_wraps' in got[64][1]
    if name == 'ring_per3':
        assert 'ring_wraps' in got[128][1] and 'short_last' in got[128][1]


def test_k_head_ring_cases_cover_every_range_length():
    pers = {64: set(), 128: set()}
    for c in H.RING_CASES:
        for cin, (per, _) in _head_props(c).items():
            pers[cin].add(per)
    assert pers[64] == {1, 2, 3, 4, 5, 6} and pers[128] == {1, 2, 3}


# ------------------------------------------------------------------------------------------------ the sources
def test_restated_constants_match_the_sources():
    s = open(os.path.join(PKG, 'csrc', 'head.hip')).read()
    flat = re.sub(r'\s+', ' ', s)
    assert 'constexpr int HC = %d;' % H.HC in flat and 'constexpr int TPX = %d;' % H.TPX in flat
    assert 'constexpr int H2_CH = %d;' % H.H2_CH in flat
    assert 'const long slots = %dL * waves_per_simd;' % H.H2_SLOTS in flat
    assert 'int c = 2 * (int)((total + slots - 1) / slots); c = c < 2 ? 2 : (c > H2_CH ? H2_CH : c); if (forced >= 2) c = forced & ~1;' in flat
    assert 'const int cap = gpi[j] >= 128 ? H2_CH : (gpi[j] >= 32 ? 8 : 4); chg[j] = (forced >= 2 || c < cap) ? c : cap;' in flat
    assert 'a.grp_gpi[a.grp_n++] = (d->level_hw[i] + %d) / %d;' % (H.GPX - 1, H.GPX) in flat
    assert 'a.h2_nitems += (cpi * d->n + %d) / %d;' % (H.H2_ITEM_CHUNKS - 1, H.H2_ITEM_CHUNKS) in flat
    assert 'const int c = (item - a.h2_item_start[j]) * %d + wave;' % H.H2_ITEM_CHUNKS in flat
    assert 'for (int item = blockIdx.x; item < a.h2_nitems; item += gridDim.x)' in flat
    assert 'constexpr int cap = %d * H2_WPS(PASS); int blocks = a.h2_nitems < cap ? a.h2_nitems : cap;' % H.H2_BLOCKS in flat
    assert '#define H2_WPS(PASS) 1' in flat
    assert 'int blocks = a.grp_ntiles < %d ? a.grp_ntiles : %d;' % (H.HEAD_BLOCKS, H.HEAD_BLOCKS) in flat
    assert 'const int per = (a.grp_ntiles + (int)gridDim.x - 1) / (int)gridDim.x; const int u0 = blockIdx.x * per;' in flat
    assert 'constexpr int XBYTES = TPX * CIN * 2;' in flat and 'constexpr int NB = 32768 / XBYTES;' in flat
    for cin, nb in H.RING.items():
        assert 32768 // (H.TPX * cin * 2) == nb
    assert 'const int slot = (u - u0) % NB;' in flat
    assert 'tiles_per_img[i] = (d->level_hw[i] + TPX - 1) / TPX;' in flat
    assert 'if (head2_enabled() && gshift >= 3)' in flat
    assert 'const int ft = (d->final_reg_rows + d->final_cls_rows + 31) / 32;' in flat
    lib = open(os.path.join(PKG, 'lfd_amd', '_lib.py')).read()
    assert "TUNE_KEYS = {'HEAD2': 0, 'H2_CHUNK': 1, 'H2_AGPR': 2, 'H2_A1': 3," in lib
    assert 'HEAD_FOLDED_HALFS = 4 * 9 * 64 * 8' in lib and 'HEAD_TOWER1_GROUP_HALFS = 8 * 64 * 8' in lib
    api = open(os.path.join(PKG, 'csrc', 'api.hip')).read()
    assert 'g_tune[LFD_TUNE_COUNT] = {{%d}, {%d}, {%d}, {%d},' % tuple(H.KNOB_DEFAULTS[k] for k in ('HEAD2', 'H2_CHUNK', 'H2_AGPR', 'H2_A1')) in api


def test_plan_chunks_restates_the_planner():
    gpi = [2703, 690, 180, 48, 15]
    assert H.plan_chunks(8, gpi) == [12, 12, 12, 8, 4]          # 29088 groups -> 2 * ceil(29088 / 2048) = 30 -> 12, capped per level
    assert H.plan_chunks(2, gpi) == [8, 8, 8, 8, 4]
    assert H.plan_chunks(1, gpi) == [4, 4, 4, 4, 4]
    assert H.plan_chunks(3, [16], 12) == [12] and H.plan_chunks(3, [16], 5) == [4] and H.plan_chunks(3, [16], 1) == [2]


def test_folded_filter_layout():
    """folded_filter (what the GPU test compares k_gn_finalize's copies with) against head.hip's formula written out: element e of lane
    (m, hk) of fragment (ct, k) = W[32 ct + m][16 k + 8 (e >> 2) + 4 hk + (e & 3)] * a, k-step 8 = shift hi, lo in the lanes hk = 0"""
    g = torch.Generator().manual_seed(5)
    w = torch.randn(128, 128, generator=g).half().float()
    ab = torch.stack([torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g) * 3], -1)
    f = H.folded_filter(w, ab)
    for ct, k, lane, e in [(0, 0, 0, 0), (1, 3, 17, 5), (3, 7, 63, 7), (2, 5, 40, 2), (0, 1, 33, 4)]:
        m, hk = lane & 31, lane >> 5
        want = (w[32 * ct + m, 16 * k + 8 * (e >> 2) + 4 * hk + (e & 3)] * ab[32 * ct + m, 0]).half()
        assert f[ct, k, lane, e] == want
    hi = ab[:, 1].half()
    assert torch.equal(f[:, 8, :32, 0].reshape(-1), hi) and torch.equal(f[:, 8, :32, 1].reshape(-1), (ab[:, 1] - hi.float()).half())
    assert not bool(f[:, 8, 32:].any()) and not bool(f[:, 8, :, 2:].any())


# ------------------------------------------------------------------------------------------------ wrong references fail
def _fails(c, kind, bad, ref, form='head2'):
    """does the comparison of tests/test_gpu_head_exact.py reject `bad`?  -> the quantities it rejects"""
    if kind == 'int':
        return [k for k in ALL if not H.equal(bad[k], ref[k])]
    gates = H.GATES[form]
    return [k for k in gates if not H.within(bad[k], ref[k], gates[k])]


def _applies(c, wrong, kind):
    hws = [hw for hw, _ in c['levels']]
    if wrong == 'drop_last_group':
        return any(hw % 32 for hw in hws)
    if wrong == 'stats_full_tiles':
        return any(hw % 64 for hw in hws)
    if wrong == 'next_image_ab':
        return bool(H.straddling_ranges(c)) and H.uses_head2(c)
    if wrong == 'bias_lo_dropped':
        return kind == 'int'          # 2^-12 of a bias: below any gate on Gaussian operands; exact operands resolve it
    if wrong == 'reg_unscaled':
        return c['reg_rows'] == 4 and c['scale']
    if wrong == 'cls_shifted':
        return c['reg_rows'] == 4 and H.final_tiles(c) == 2
    return True


@pytest.mark.parametrize('wrong', H.WRONG)
def test_wrong_references_fail_the_comparisons(wrong):
    hit = 0
    for name in LIGHT:
        c = H.BY_NAME[name]
        for kind in ('int', 'gauss'):
            if not _applies(c, wrong, kind):
                continue
            O, ref = _ops(name, kind), _ref(name, kind)
            stats_only = wrong in ('drop_last_group', 'stats_full_tiles')
            # (supplied (a, b) on the integer instrument, the chain's own statistics on the Gaussian one, as on the device)
            bad = H.chain(c, O, 'head2', ab=O.get('ab'), wrong=wrong, wrong_ranges=H.straddling_ranges(c))
            rej = _fails(c, kind, bad, ref)
            print('%s / %s / %s: rejected in %s' % (wrong, name, kind, rej))
            if stats_only:       # (the second pass of a level with two pixels of padding stays inside k_head2's wide gate)
                assert 'partial1' in rej and ('partial2' in rej if kind == 'int' else 'ab1' in rej)
            elif wrong == 'unpermuted_k':
                assert 'partial2' in rej and ('cls' in rej or 'reg' in rej)
            else:
                assert 'cls' in rej or 'reg' in rej
            hit += 1
    assert hit >= 2
