"""CPU checks of tests/golden/planes_cases.py, the instrument behind tests/test_gpu_planes_walk.py:

  * its float64 reference is pinned to an independent evaluation (unfold + matmul, GroupNorm written out) and to torch's own
    double conv2d / group_norm chains;
  * every exact case keeps the three conditions under which a planes kernel must reproduce float64 BIT FOR BIT -- every stored
    tensor survives the hi/lo split, every bound on a partial sum fits 24 bits, the fixed-point GroupNorm sums are integers below
    2^24 -- and a float32 emulation of main + corr / 2048 in two shuffled channel orders equals float64;
  * every case has the walk properties it is in the table for, from the launch geometry restated in planes_cases.py;
  * the restated constants still match the sources (csrc/planes*.hip, csrc/planes_impl.h, lfd_amd/engine_p2.py);
  * the comparison resolves the bugs it is meant to catch: five references wrong in exactly one way each fail it.
Prints, per case, the properties and the caps with their headroom (pytest -s)."""
import functools
import os
import re

import pytest
import torch
import torch.nn.functional as F

import planes_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'lfd-a-light-and-fast-detector_amd')
CSRC = os.path.join(PKG, 'csrc')
GRID = {'int': 1.0, 'xlo': 1.0 / 4096, 'wlo': 1.0 / 8192}


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


# ------------------------------------------------------------------------------------------------ the reference is right
def _conv_unfold(x, w, b, ks, stride):
    n, h, wd, cin = x.shape
    cols = F.unfold(x.double().permute(0, 3, 1, 2), ks, padding=ks // 2, stride=stride)          # [n, cin k k, L]
    y = torch.einsum('ok,nkl->nlo', w.double().reshape(w.shape[0], -1), cols) + b.double()
    oh, ow = PC.out_hw(h, wd, ks, stride)
    return y.reshape(n, oh, ow, -1)


@pytest.mark.parametrize('cin,cout,ks,stride', [(64, 64, 3, 1), (64, 128, 3, 2), (128, 128, 1, 1), (32, 32, 3, 2), (3, 64, 3, 2)])
def test_reference_conv_is_the_double_convolution(cin, cout, ks, stride):
    x, w, b = PC.activations('gauss', (2, 7, 9, cin), 1), PC.filters('gauss', cout, cin, ks, 2), PC.bias('gauss', cout, 3)
    want = _conv_unfold(x, w, b, ks, stride)
    assert float((PC.ref_conv(x, w, b, ks, stride, False) - want).abs().max()) < 1e-12
    res = torch.randn(want.shape, generator=torch.Generator().manual_seed(4))
    assert float((PC.ref_conv(x, w, b, ks, stride, True, res) - (want + res.double()).relu()).abs().max()) < 1e-12


def test_reference_chains_round_through_planes_where_the_kernels_do():
    x = PC.activations('gauss', (2, 9, 11, 64), 5)
    w1, b1, w2, b2 = PC.filters('gauss', 64, 64, 3, 6), PC.bias('gauss', 64, 7), PC.filters('gauss', 64, 64, 1, 8), PC.bias('gauss', 64, 9)
    mid, out = PC.ref_chained(x, w1, b1, 3, 2, w2, b2, True)
    m = F.conv2d(x.double().permute(0, 3, 1, 2), w1.double(), b1.double(), stride=2, padding=1).relu()
    assert torch.equal(mid, m.permute(0, 2, 3, 1))
    mp = PC.from_planes(PC.to_planes(m.float())).double()
    assert 0 < float((mp - m).abs().max()) < 2.0 ** -21 * float(m.abs().max())
    assert float((out - F.conv2d(mp, w2.double(), b2.double()).relu().permute(0, 2, 3, 1)).abs().max()) < 1e-12
    w3 = PC.filters('gauss', 64, 64, 3, 10)
    bm, bo = PC.ref_block(x, w1, b1, w3, b2)
    xm = x.double().permute(0, 3, 1, 2)
    m = F.conv2d(xm, w1.double(), b1.double(), padding=1).relu()
    mp = PC.from_planes(PC.to_planes(m.float())).double()
    assert float((bo - (F.conv2d(mp, w3.double(), b2.double(), padding=1) + xm).relu().permute(0, 2, 3, 1)).abs().max()) < 1e-12
    o = PC.stem_operands('gauss', 1, 1, 13, 24)
    assert o['ref'].shape == (1, 4, 6, 64) and len(o['stages']) == 4 and o['stages'][0].shape == (1, 7, 12, 64)


def test_reference_group_norm_and_sums():
    g = torch.Generator().manual_seed(3)
    t = torch.randn(3, 37, 128, generator=g).double() * 3 + 1
    gamma, beta = torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g)
    v = t.reshape(3, 37, 16, 8)
    mean, var = v.mean((1, 3), keepdim=True), v.var((1, 3), unbiased=False, keepdim=True)
    want = (((v - mean) / (var + 1e-5).sqrt()).reshape(3, 37, 128) * gamma.double() + beta.double()).relu()
    assert float((PC.ref_group_norm(t, gamma, beta) - want).abs().max()) < 1e-12
    s = PC.ref_sums(t)
    assert float((s[..., 0] - v.sum((1, 3))).abs().max()) < 1e-9 and float((s[..., 1] - (v * v).sum((1, 3))).abs().max()) < 1e-9
    # the head chain: float64 matmuls of the values the planes hold
    L = PC.head_first_operands('gauss', 64, 2, [70, 5])
    for l in L:
        mid = (l['x'].double() @ l['w0'].double().t() + l['b0'].double()).relu()
        assert torch.equal(l['mid'], mid) and float((l['t1'] - (PC.rt(mid) @ l['w1'].double().t() + l['b1'].double())).abs().max()) < 1e-12


# ------------------------------------------------------------------------------------------------ exactness conditions
def _emulate(x, w, b, ks, stride, perm):
    """what a planes kernel computes, in float32, with the input channels visited in the order `perm`"""
    xp, wh = PC.to_planes(x), w.half().float()
    wl = ((w - wh) * PC.LO).half().float()
    xh, xl = [t.float().permute(0, 3, 1, 2)[:, perm].contiguous() for t in xp]
    wh, wl = wh[:, perm].contiguous(), wl[:, perm].contiguous()
    main = F.conv2d(xh, wh, b.float(), stride=stride, padding=ks // 2)
    corr = F.conv2d(xl, wh, None, stride=stride, padding=ks // 2) + F.conv2d(xh, wl, None, stride=stride, padding=ks // 2)
    return (main + corr / PC.LO).permute(0, 2, 3, 1)


def _check_exact_conv(kind, x, w, b, ks, stride, pre, what, grid=None):
    """conditions on ONE conv of an exact case: operands survive the split, the cap fits 24 bits, float32 emulation == float64"""
    assert PC.survives_planes(x) and PC.weight_survives_split(w), what
    xmax = float(x.abs().max())
    cap = (float(w.abs().sum((1, 2, 3)).max()) * xmax + float(b.abs().max())) / (grid or GRID[kind])
    assert cap < 2.0 ** 24, (what, cap)
    g = torch.Generator().manual_seed(11)
    for _ in range(2):
        perm = torch.randperm(x.shape[-1], generator=g)
        assert torch.equal(_emulate(x.float(), w, b, ks, stride, perm).double(), pre), what + ': float32 emulation differs from float64'
    return cap


@functools.lru_cache(maxsize=8)
def _c3(kind):
    return PC.c3_operands(kind, **PC.C3_CASE)


@pytest.mark.parametrize('kind', PC.EXACT)
def test_c3_exact_conditions(kind):
    for shape in [PC.C3_CASE] + PC.C3_EDGES:
        o = PC.c3_operands(kind, **shape)
        pre = PC.ref_conv(o['x'], o['w'], o['b'], 3, 1, False)
        cap = _check_exact_conv(kind, o['x'], o['w'], o['b'], 3, 1, pre, 'c3')
        assert PC.survives_planes(o['res']) and all(PC.survives_planes(v) for v in o['ref'].values())
        assert float(o['ref']['res'].abs().max()) / GRID[kind] < 2.0 ** 24
        print('c3 %s [%s]: lo planes x %.0f%% w(non-zero taps) %.0f%%; cap %.3g of 2^24 (headroom x%.0f); max |y| %.1f' % (
            shape, kind, 100 * PC.lo_fraction(o['x']), 100 * PC.lo_fraction(o['w'][o['w'] != 0]), cap, 2.0 ** 24 / cap,
            float(o['ref']['res'].abs().max())))
    o = _c3(kind)
    if kind == 'xlo':
        assert PC.lo_fraction(o['x']) > 0.5
    if kind == 'wlo':
        assert PC.lo_fraction(o['w'][o['w'] != 0]) > 0.5


_CONV_IDS = [(key, cout, n, h, w, v) for key, cout, n, h, w in PC.CONV_CASES + PC.CONV_EDGES for v in PC.conv_variants(key)
             if not (v == 'out32' and cout not in PC.OUT32_SPLIT) and not (v != 'out32' and cout % 32)]


@pytest.mark.parametrize('key,cout,n,h,w,variant', _CONV_IDS, ids=['%s-%s' % (PC.conv_case_id(*c[:5]), c[5]) for c in _CONV_IDS])
def test_conv_exact_conditions(key, cout, n, h, w, variant):
    cin, ks, stride, _ = key
    for kind in PC.EXACT:
        o = PC.conv_operands(kind, key, cout, n, h, w, variant)
        what = '%s %s [%s]' % (PC.conv_case_id(key, cout, n, h, w), variant, kind)
        pre = PC.ref_conv(o['x'], o['w'], o['b'], ks, stride, False)
        cap = _check_exact_conv(kind, o['x'], o['w'], o['b'], ks, stride, pre, what)
        assert PC.survives_planes(o['ref']), what
        if variant == 'res':
            assert PC.survives_planes(o['res'])
        if variant == 'tail':
            assert PC.survives_planes(o['ref_mid'])
            pre2 = PC.ref_conv(o['ref_mid'], o['w2'], o['b2'], 1, 1, False)
            cap = max(cap, _check_exact_conv(PC.later(kind), o['ref_mid'], o['w2'], o['b2'], 1, 1, pre2, what + ' chained', GRID[kind]))
        if variant == 'ds':
            assert PC.survives_planes(o['ref_ds'])
            cap = max(cap, _check_exact_conv(kind, o['x'], o['wd'], o['bd'], 1, stride, PC.ref_conv(o['x'], o['wd'], o['bd'], 1, stride, False), what + ' identity'))
        if variant == 'out32':
            assert torch.equal(o['ref'].float().double(), o['ref']) and torch.equal((o['ref'] * 1.5).float().double(), o['ref'] * 1.5)
        if PC.has_sums(key, variant) and kind == 'int':
            assert PC.sums_fixed(o['ref'].reshape(n, -1, cout))[1], what + ': GroupNorm sums not exact'
        print('%s: cap %.3g of 2^24 (headroom x%.0f); max |y| %.1f' % (what, cap, 2.0 ** 24 / cap, float(o['ref'].abs().max())))


@pytest.mark.parametrize('kind', PC.EXACT)
def test_levels_head_stem_block_exact_conditions(kind):
    n = PC.ML_CASE['n']
    for j, (h, w) in enumerate(PC.ML_CASE['sizes']):
        o = PC.conv_operands(kind, (128, 1, 1, 4), 128, n, h, w, 'gn', seed=j + 1)
        _check_exact_conv(kind, o['x'], o['w'], o['b'], 1, 1, o['ref'], 'levels %d' % j)
        assert PC.survives_planes(o['ref']) and (kind != 'int' or PC.sums_fixed(o['ref'].reshape(n, -1, 128))[1])
    hn, pixels = PC.HEAD_CASE['n'], PC.HEAD_CASE['pixels']
    hgrid = {'int': 1.0, 'xlo': 1.0 / 4096, 'wlo': 1.0 / 4096}[kind]
    for cin in (64, 128):
        for l, o in enumerate(PC.head_first_operands(kind, cin, hn, pixels)):
            x4 = o['x'].reshape(hn, -1, 1, cin)
            w0, w1 = o['w0'].reshape(128, cin, 1, 1), o['w1'].reshape(128, 128, 1, 1)
            cap = _check_exact_conv(kind, x4, w0, o['b0'], 1, 1, o['t3'].reshape(hn, -1, 1, 128), 'head neck', hgrid)
            assert PC.survives_planes(o['mid'])
            cap = max(cap, _check_exact_conv(PC.later(kind), o['mid'].reshape(hn, -1, 1, 128), w1, o['b1'], 1, 1, o['t1'].reshape(hn, -1, 1, 128),
                                             'head tower', hgrid))
            for t in (o['t1'], o['t3']):
                fixed, ok = PC.sums_fixed(t)
                assert ok and torch.equal(t.float().double(), t), 'head sums / fp32 output not exact'
            room = 2.0 ** 24 / max(float(PC.ref_sums(o['t1']).abs().max()), float(PC.ref_sums(o['t3']).abs().max()))
            print('head cin %d level %d [%s]: cap %.3g of 2^24; GroupNorm sums below 2^24 by x%.0f' % (cin, l, kind, cap, room))
    for fmt in (0, 1):
        o = PC.stem_operands(kind, fmt, **PC.STEM_CASE)
        assert torch.equal(o['frame'].float(), o['values'].permute(0, 3, 1, 2) if fmt == 0 else o['values'])          # the frame holds the values
        y, kinds = o['values'], [kind] + [PC.later(kind)] * 3
        for i, ((wt, b), (ks, s)) in enumerate(zip(zip(o['ws'], o['bs']), ((3, 2), (1, 1), (3, 2), (1, 1)))):
            pre = PC.ref_conv(y, wt, b, ks, s, False)
            cap = _check_exact_conv(kinds[i], y, wt, b, ks, s, pre, 'stem conv %d' % i, GRID[kind])
            y = o['stages'][i]
            assert PC.survives_planes(y) and torch.equal(y, pre.relu())
            print('stem fmt %d conv %d [%s]: cap %.3g of 2^24; max |y| %.1f; %.0f%% non-zero' % (fmt, i, kind, cap, float(y.abs().max()),
                                                                                              100 * float((y != 0).double().mean())))
        if kind == 'xlo' and fmt == 0:
            assert PC.lo_fraction(o['values']) > 0.5
    for n_, h, w in PC.BLOCK_CASES:
        o = PC.block_operands(kind, n_, h, w)
        pre1 = PC.ref_conv(o['x'], o['w1'], o['b1'], 3, 1, False)
        cap = _check_exact_conv(kind, o['x'], o['w1'], o['b1'], 3, 1, pre1, 'block conv1')
        pre2 = PC.ref_conv(o['ref_mid'], o['w2'], o['b2'], 3, 1, False)
        cap = max(cap, _check_exact_conv(PC.later(kind), o['ref_mid'], o['w2'], o['b2'], 3, 1, pre2, 'block conv2', GRID[kind]))
        assert PC.survives_planes(o['ref_mid']) and PC.survives_planes(o['ref']) and torch.equal(o['ref'], (pre2 + o['x'].double()).relu())
        print('block %dx%dx%d [%s]: cap %.3g of 2^24; max |y| %.1f' % (n_, h, w, kind, cap, float(o['ref'].abs().max())))


# ------------------------------------------------------------------------------------------------ walk properties
def _run_props(runs, tiles):
    """properties of a strided / contiguous walk over one map's tiles"""
    mid = [(tiles[t], k) for r in runs for k, t in enumerate(r) if k >= 1]
    return dict(
        max=max(len(r) for r in runs), min=min(len(r) for r in runs),
        full_inside=any(not t[3] and not t[4] for t, _ in mid), interior_inside=any(t[5] for t, _ in mid),
        ragged_right_inside=any(t[3] for t, _ in mid), ragged_bottom_inside=any(t[4] for t, _ in mid),
        crosses_image=any(tiles[a][0] != tiles[b][0] for r in runs for a, b in zip(r, r[1:])))


def test_c3_walk_properties():
    n, h, w = PC.C3_CASE['n'], PC.C3_CASE['h'], PC.C3_CASE['w']
    for knob in (2, 1, 0):
        if knob:
            tw, th = PC.C3_TILE
        else:
            tw, th = PC.pcfg_tile(64, 3, 1, *[PC.CONV_INSTANCES[(64, 3, 1, 2)][i] for i in (0, 2)])
        tiles = PC.image_tiles(n, h, w, tw, th)
        nt = len(tiles)
        blocks = [PC.grid_blocks(PC.C3_BLOCKS, nt)] if knob else PC.conv_blocks((64, 3, 1, 2), 64, {'res'}, nt, n * h * w)
        assert (tw, th) == ((16, 4) if knob else (16, 8)) and blocks == [256]
        for nb in blocks:
            runs = PC.walk_strided(nt, nb)
            assert PC.covered_once(runs, nt)
            p = _run_props(runs, tiles)
            print('3x3 s1 64->64 PL_C3=%d %dx%dx%d: %d tiles of %dx%d on %d workgroups: %s' % (knob, n, h, w, nt, th, tw, nb, p))
            assert p['max'] >= 4 and p['full_inside'] and p['interior_inside'] and p['ragged_right_inside'] and p['ragged_bottom_inside']
            assert p['crosses_image']


def test_c3_wide_walk_stays_inside_an_image():
    n, h, w = PC.C3_WIDE['n'], PC.C3_WIDE['h'], PC.C3_WIDE['w']
    tiles = PC.image_tiles(n, h, w, *PC.C3_TILE)
    runs = PC.walk_strided(len(tiles), PC.grid_blocks(PC.C3_BLOCKS, len(tiles)))
    assert PC.covered_once(runs, len(tiles))
    dwell = [r for r in runs if len(r) >= 3 and len({tiles[t][0] for t in r}) == 1 and sum(tiles[t][5] for t in r) >= 3]
    print('3x3 s1 64->64 %dx%dx%d: %d tiles on %d workgroups, %d..%d per run; %d runs of >= 3 interior tiles of one image' % (
        n, h, w, len(tiles), len(runs), min(map(len, runs)), max(map(len, runs)), len(dwell)))
    assert len(dwell) >= 8 and max(map(len, runs)) >= 4
    for kind in ('xlo', 'wlo'):
        o = PC.c3_operands(kind, n, h, w)
        pre = PC.ref_conv(o['x'], o['w'], o['b'], 3, 1, False)
        _check_exact_conv(kind, o['x'], o['w'], o['b'], 3, 1, pre, 'c3 wide')
        assert PC.survives_planes(o['res']) and all(PC.survives_planes(v) for v in o['ref'].values())


@pytest.mark.parametrize('key,cout,n,h,w', PC.CONV_CASES, ids=[PC.conv_case_id(*c) for c in PC.CONV_CASES])
def test_conv_walk_properties(key, cout, n, h, w):
    cin, ks, stride, nslab = key
    assert -(-cout // 32) == nslab
    oh, ow = PC.out_hw(h, w, ks, stride)
    nct, wreg, pto = PC.conv_instance(key, n * oh * ow)
    tw, th = PC.pcfg_tile(cin, ks, stride, nct, pto)
    tiles = PC.image_tiles(n, oh, ow, tw, th)
    nt = len(tiles)
    for variant in PC.conv_variants(key):
        for nb in PC.conv_blocks(key, cout, {variant}, nt, n * oh * ow):
            runs = PC.walk_strided(nt, nb)
            assert PC.covered_once(runs, nt)
            p = _run_props(runs, tiles)
            print('%s %s: out %dx%d, %d tiles of %dx%d on %d workgroups: %s' % (PC.conv_case_id(key, cout, n, h, w), variant, oh, ow, nt, th, tw, nb, p))
            assert p['max'] >= 3 and p['full_inside'] and p['ragged_right_inside'] and p['crosses_image']
            assert th == 1 or p['ragged_bottom_inside']          # (one-row tiles have no ragged bottom)
            assert ks == 1 or p['interior_inside']


def test_conv_cases_cover_every_key_option_and_both_128_channel_instances():
    assert {c[0] for c in PC.CONV_CASES} | {(64, 3, 1, 2)} == set(PC.DISPATCH)
    inst = set()
    for key, cout, n, h, w in PC.CONV_CASES:
        if key == (128, 3, 1, 4):
            inst.add(PC.conv_instance(key, n * h * w))
            assert abs(n * h * w - PC.C128_SMALL_MAX_PIXELS) < 6000        # one on each side of, and near, the threshold
        for opt in PC.DISPATCH[key]:
            assert opt in PC.conv_variants(key)
    assert inst == set(PC.CONV_INSTANCES[(128, 3, 1, 4)].values())
    # edges: single pixel, single row, more images than workgroups per XCD
    assert any(c[2:] == (1, 1, 1) for c in PC.CONV_EDGES) and any(c[3] == 1 and c[4] > 1 for c in PC.CONV_EDGES)
    assert any(c[2] > 512 // 8 for c in PC.CONV_EDGES) and any(e['n'] > 256 // 8 for e in PC.C3_EDGES)
    assert PC.C3_CASE['n'] > 256 // 8 and PC.HEAD_CASE['n'] > 512 // 8


def test_every_kernel_selector_is_covered():
    """every value of the knobs that pick a planes kernel, every mode of lfd_pl_head_levels, every frame format -- the values the
    dispatch code in the sources distinguishes"""
    planes, head, stem = _src('planes.hip'), _src('planes_head.hip'), _src('planes_stem2x.hip')
    assert 'lfd_tune(LFD_TUNE_PL_C3) == 2' in planes and 'lfd_tune(LFD_TUNE_PL_C3) != 0' in planes and set(PC.KNOBS['PL_C3']) == {0, 1, 2}
    assert 'lfd_tune(LFD_TUNE_PL_HEAD_ROLES) != 0' in head and set(PC.KNOBS['PL_HEAD_ROLES']) == {0, 1}
    assert 'lfd_tune(LFD_TUNE_PL_HEAD_OUT_REGS) != 0' in head and set(PC.KNOBS['PL_HEAD_OUT_REGS']) == {0, 1}
    assert 'lfd_tune(LFD_TUNE_PL_STEM) == 1' in stem and set(PC.KNOBS['PL_STEM']) == {0, 1} == {k for _, k in PC.STEM_KERNELS}
    assert 'if (d->mode < 0 || d->mode > 3) return LFD_ERR_INVALID_ARGUMENT;' in head
    assert 'if (d->mode == 0 && d->cin != 64 && d->cin != 128) return LFD_ERR_UNSUPPORTED;' in head
    assert set(PC.HEAD_FIRST_MODES) == {(0, 64), (0, 128), (3, 128)}        # modes 1 and 2: the tower and output pass tests
    assert {f for f, _ in PC.STEM_KERNELS} == {0, 1, 2}                     # IN_NCHW_F32, IN_NHWC_F16, IN_NHWC_U8
    assert {c for c, _, _, _ in PC.GNIN_CASES} == {128, 5, 50}              # gn_in: <128,1,1,4> with sums, <128,1,1,1>, <128,1,1,2>


def test_levels_walk_properties():
    n, sizes = PC.ML_CASE['n'], PC.ML_CASE['sizes']
    tw, th = PC.pcfg_tile(128, 1, 1, 4, 0)
    tpi = [(-(-h // th)) * (-(-w // tw)) for h, w in sizes]
    tiles = PC.level_tiles(n, tpi)
    nt = len(tiles)
    blocks = PC.conv_blocks((128, 1, 1, 4), 128, {'gn'}, nt, 1 << 30)
    assert blocks == [256, 512]
    for nb in blocks:
        runs = PC.walk_contiguous(nt, nb)
        assert PC.covered_once(runs, nt)
        lv = sum(1 for r in runs if len({tiles[t][0] for t in r}) > 1)
        print('conv2d_levels n=%d %s: %d tiles of %dx%d on %d workgroups: %d..%d per workgroup, %d runs change level, %d empty' % (
            n, sizes, nt, th, tw, nb, min(map(len, runs)), max(map(len, runs)), lv, sum(1 for r in runs if not r)))
        assert max(map(len, runs)) >= 3 and lv >= 2


def test_head_walk_properties():
    n, pixels = PC.HEAD_CASE['n'], PC.HEAD_CASE['pixels']
    assert len(pixels) >= 4 and all(p % PC.HEAD_TILE_PIXELS for p in pixels)
    tpi = [-(-p // PC.HEAD_TILE_PIXELS) for p in pixels]
    tiles = PC.level_tiles(n, tpi)
    nt = len(tiles)
    for name, cap in sorted(PC.HEAD_BLOCKS.items()):
        runs = PC.walk_contiguous(nt, PC.grid_blocks(cap, nt))
        assert PC.covered_once(runs, nt)
        img2 = sum(1 for r in runs if sum(tiles[a][:2] != tiles[b][:2] for a, b in zip(r, r[1:])) >= 2)
        lvl = sum(1 for r in runs if len({tiles[t][0] for t in r}) > 1)
        ragged_mid = sum(1 for r in runs for t in r[1:-1] if tiles[t][2] == tpi[tiles[t][0]] - 1)
        same_img = sum(1 for r in runs if len(r) >= 4 and len({tiles[t][:2] for t in r}) == 1)
        empty = sum(1 for r in runs if not r)
        print('head_levels (%s, %d workgroups) n=%d pixels %s: %d tiles, %d..%d per workgroup; runs with >= 2 image changes %d, with a level '
              'change %d, wholly inside one image %d; ragged tiles in the middle of a run %d; empty runs %d' % (
                  name, cap, n, pixels, nt, min(map(len, runs)), max(map(len, runs)), img2, lvl, same_img, ragged_mid, empty))
        assert max(map(len, runs)) >= 4 and img2 >= 1 and lvl >= 1 and ragged_mid >= 1 and empty >= 1 and same_img >= 1
    assert {c0 + c1 for c0, c1 in PC.HEAD_OUT_CHANNELS} >= {5, 32, 33, 50, 64}
    assert any(c1 == 0 for _, c1 in PC.HEAD_OUT_CHANNELS) and any(c0 == 0 for c0, _ in PC.HEAD_OUT_CHANNELS)


def test_stem_walk_properties():
    n, h, w = PC.STEM_CASE['n'], PC.STEM_CASE['h'], PC.STEM_CASE['w']
    g = PC.stem_geometry(n, h, w)
    assert w % 16 == 0, 'the row-stream kernel takes all three formats only with 16-byte rows'
    assert g['oh'] % 2 == 1 and g['ow'] % PC.STEM_TW != 0
    runs = PC.stem_runs(n, h, w)
    assert sorted(c for r in runs for c in r) == [(i, tx, cy) for i in range(n) for tx in range(g['tiles_x']) for cy in range(g['cy'])]
    wraps = sum(1 for r in runs if PC.stem_ring_rows(r, g['cy'])[-1] + 5 > PC.STEM_RING)
    strip = sum(1 for r in runs for a, b in zip(r, r[1:]) if a[0] == b[0] and a[1] != b[1])
    image = sum(1 for r in runs for a, b in zip(r, r[1:]) if a[0] != b[0])
    print('stem2x %dx%dx%d: out %dx%d, %d strips x %d row pairs, %d chunks on %d workgroups: %d..%d per run; the ring wraps in %d runs; '
          '%d strip ends and %d image ends inside runs' % (n, h, w, g['oh'], g['ow'], g['tiles_x'], g['cy'], g['total'], len(runs),
                                                           min(map(len, runs)), max(map(len, runs)), wraps, strip, image))
    assert min(map(len, runs)) >= 4 and wraps == len(runs) and strip >= 1 and image >= 1
    # the tile kernel (PL_STEM = 0, PCfg<64, 3, 2, 2>): strided walk on 256 workgroups
    tw, th = PC.pcfg_tile(64, 3, 2, 2, 0)
    tiles = PC.image_tiles(n, g['oh'], g['ow'], tw, th)
    p = _run_props(PC.walk_strided(len(tiles), PC.grid_blocks(256, len(tiles))), tiles)
    print('stem2x tile kernel: %d tiles of %dx%d: %s' % (len(tiles), th, tw, p))
    assert p['max'] >= 3 and p['ragged_right_inside'] and p['ragged_bottom_inside'] and p['interior_inside']
    assert {f for f, k in PC.STEM_KERNELS if k == 1} == {0, 1, 2} and (1, 0) in PC.STEM_KERNELS


def test_block_walk_properties():
    geo = [PC.block_geometry(*c) for c in PC.BLOCK_CASES]
    for c, g in zip(PC.BLOCK_CASES, geo):
        print('block64 %dx%dx%d: %s' % (c + (g,)))
    tall = geo[0]
    assert tall['SH'] > 2 * max(PC.BLK_NIN, PC.BLK_NMID) and tall['segs'] >= 2 and 0 < tall['last'] < tall['SH']
    assert any(g['clamped'] and g['SH'] == 4 and 0 < g['last'] < 4 for g in geo)
    assert any(c[1] < 4 and g['SH'] == c[1] and g['segs'] == 1 for c, g in zip(PC.BLOCK_CASES, geo))
    widths = {c[2] % PC.BLK_TW for c in PC.BLOCK_CASES if c[2] >= PC.BLK_TW}
    assert widths >= {0, 1, 29}


# ------------------------------------------------------------------------------------------------ restated constants vs the sources
def test_restated_constants_match_the_sources():
    planes = _src('planes.hip')
    body = planes[planes.index('switch (key)'):]
    keys = {}
    for m in re.finditer(r'case (\d+) \* 10000 \+ (\d)(\d)00 \+ (\d):(.*?)(?=case \d+ \* 10000|default:)', body, re.S):
        key = (int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4)))
        inst = [(int(a), b == 'true', int(c or 0)) for a, b, c in re.findall(r'launch_pl<\d+, \d, \d, (\d), (true|false)(?:, (\d))?>', m.group(5))]
        keys[key] = inst
    assert set(keys) == set(PC.CONV_INSTANCES) == set(PC.DISPATCH)
    for key, inst in keys.items():
        want = PC.CONV_INSTANCES[key]
        assert inst == ([want['small'], want['large']] if isinstance(want, dict) else [want]), key
    assert '<= %d) return launch_pl<128, 3, 1, 2, false, 1>' % PC.C128_SMALL_MAX_PIXELS in planes
    assert 'lfd_tune(LFD_TUNE_PL_C3) == 2' in planes and 'lfd_tune(LFD_TUNE_PL_C3) != 0' in planes
    from lfd_amd import engine_p2
    assert engine_p2._DISPATCH == PC.DISPATCH and engine_p2._LO == PC.LO
    impl = _src('planes_impl.h')
    for line in ('static constexpr int PT = PTO ? PTO : ((S == 1) ? 2 : 1);', 'static constexpr int TW = (S == 1 && !(CIN == 64 && KS == 3)) ? 32 : 16;',
                 'static constexpr int RPT = 32 / TW;', 'static constexpr int PG = 4 / NCT;', 'static constexpr int TH = PG * PT * RPT;',
                 'static constexpr int wregs = (WREG ? (KS * KS * CIN / 16) * 8 : 96) + (TAIL ? NCT * 2 * 8 : 0) + (DS ? (CIN / 16) * 8 : 0);',
                 'static constexpr bool value = !WREG || wregs > 96;', 'constexpr int per_cu = (heavy || LDSB > 80 * 1024) ? 1 : 2;',
                 'int blocks = (256 * per_cu) / cgroups;', 'if (blocks > 8 * ((a.ntiles + 7) / 8)) blocks = 8 * ((a.ntiles + 7) / 8);',
                 'const int wgs_xcd = (nblk + 7 - xcd) / 8;', 'const int t_begin = ML ? x_begin + bix * ml_chunk : x_begin + bix;',
                 'const int ml_chunk = (x_end - x_begin + wgs_xcd - 1) / (wgs_xcd > 0 ? wgs_xcd : 1);', 'const int t_step = ML ? 1 : wgs_xcd;'):
        assert line in impl, line
    assert impl.count('int blocks = (256 * per_cu) / cgroups;') == 2          # launch_pl_ and launch_pl_ml_
    for name in ('planes_c3.hip', 'planes_c3p.hip'):
        s = _src(name)
        assert 'static constexpr int TW = %d, TH = %d,' % PC.C3_TILE in s and 'int blocks = %d / cgroups;' % PC.C3_BLOCKS in s
        assert 'const int t_step = (nblk + 7 - xcd) / 8;' in s and 'int t = t_begin + bix;' in s
    head = _src('planes_head.hip')
    launches = re.findall(r'int (launch_pl_head\w*)\(PhArgs& a, hipStream_t st\) \{.*?int blocks = (\d+);', head, re.S)
    assert dict((k, int(v)) for k, v in launches) == {'launch_pl_head': PC.HEAD_BLOCKS['head'], 'launch_pl_head_out': PC.HEAD_BLOCKS['out'],
                                                       'launch_pl_head_b2': PC.HEAD_BLOCKS['b2']}
    assert head.count('tiles_per_img = (a.lv[i].P + %d) / %d;' % (PC.HEAD_TILE_PIXELS - 1, PC.HEAD_TILE_PIXELS)) == 2
    assert 'tiles_per_img = (a.lv[i].P + C::TPX - 1) / C::TPX;' in head and head.count('int TPX = %d' % PC.HEAD_TILE_PIXELS) == 3
    assert head.count('const int chunk = (x_end - x_begin + wgs_xcd - 1) / (wgs_xcd > 0 ? wgs_xcd : 1);') == 2
    assert 'const int chunk = (t_end - t_begin + wgs_xcd - 1) / (wgs_xcd > 0 ? wgs_xcd : 1);' in head and 'const int t_first = t_begin + bix * chunk;' in head
    stem = _src('planes_stem2xs.hip')
    assert 'static constexpr int TW = %d,' % PC.STEM_TW in stem and 'int blocks = %d;' % PC.STEM_BLOCKS in stem
    assert re.search(r'static constexpr int RR = %d\b' % PC.STEM_RING, stem), 'ring depth'
    assert 'const long u0 = (long)blockIdx.x * total / gridDim.x, u1 = (long)(blockIdx.x + 1) * total / gridDim.x;' in stem
    assert 'a.tiles_y = (a.OH + 1) / 2;' in stem and 'w.rc += 5;' in stem and 'w.rc += 4;' in stem
    blk = _src('planes_block.hip')
    assert 'static constexpr int TW = %d,' % PC.BLK_TW in blk and 'static constexpr int NIN = %d;' % PC.BLK_NIN in blk
    assert 'static constexpr int NMID = %d;' % PC.BLK_NMID in blk
    for line in ('int segs = (int)(256 / cols);', 'int sh = (h + segs - 1) / segs;', 'if (sh < 4) sh = 4;', 'if (sh > h) sh = h;'):
        assert line in blk, line


# ------------------------------------------------------------------------------------------------ wrong references
def _resolved(kind, bad, ref, tol=PC.TOL):
    if kind in PC.EXACT:
        return not torch.equal(PC.to_planes(bad).view(torch.int16), PC.to_planes(ref).view(torch.int16))
    return PC.gate_fails(bad, ref, tol)


@pytest.mark.parametrize('kind', PC.INSTRUMENTS)
def test_wrong_references_fail_the_comparison_conv(kind):
    """a seam pixel, the last tile of a run taken from the previous tile, the image index off by one after an image change"""
    cases = [((64, 3, 1, 2), 64, PC.C3_CASE['n'], PC.C3_CASE['h'], PC.C3_CASE['w'])] + PC.CONV_CASES
    for key, cout, n, h, w in cases:
        cin, ks, stride, _ = key
        if cout % 32:
            continue
        ref = _c3(kind)['ref']['res'] if key == (64, 3, 1, 2) else PC.conv_operands(kind, key, cout, n, h, w, 'plain')['ref']
        oh, ow = ref.shape[1:3]
        for tw, th in ({PC.C3_TILE, (16, 8)} if key == (64, 3, 1, 2) else {PC.pcfg_tile(cin, ks, stride, *[PC.conv_instance(key, n * oh * ow)[i] for i in (0, 2)])}):
            tiles = PC.image_tiles(n, oh, ow, tw, th)
            runs = PC.walk_strided(len(tiles), PC.grid_blocks(256, len(tiles)))
            run = max(runs, key=len)
            assert _resolved(kind, PC.wrong_seam_pixel(ref, tw, th), ref), (key, 'seam pixel')
            assert _resolved(kind, PC.wrong_last_tile_of_run(ref, run, tiles, tw, th), ref), (key, 'stale last tile')
            assert _resolved(kind, PC.wrong_image_after_change(ref, run, tiles, tw, th), ref), (key, 'image off by one')


@pytest.mark.parametrize('kind', PC.INSTRUMENTS)
def test_wrong_references_fail_the_comparison_levels_and_head(kind):
    """the first tile after a level change computed with the previous level's filter; a stale tile; the previous image's tile"""
    n = PC.ML_CASE['n']
    ops_ = [PC.conv_operands(kind, (128, 1, 1, 4), 128, n, h, w, 'gn', seed=j + 1) for j, (h, w) in enumerate(PC.ML_CASE['sizes'])]
    tw, th = PC.pcfg_tile(128, 1, 1, 4, 0)
    for j in range(1, len(ops_)):
        o, prev = ops_[j], ops_[j - 1]
        other = PC.ref_conv(o['x'], prev['w'], prev['b'], 1, 1, False)
        bad = o['ref'].clone()
        bad[0, :th, :tw] = other[0, :th, :tw]
        assert _resolved(kind, bad, o['ref']), ('levels', j)
    hn, pixels = PC.HEAD_CASE['n'], PC.HEAD_CASE['pixels']
    T = PC.HEAD_TILE_PIXELS
    for cin in (64, 128):
        L = PC.head_first_operands(kind, cin, hn, pixels)
        for j in range(len(L)):
            for name in ('t1', 't3'):
                ref = L[j][name]
                if j:
                    x = L[j]['x'].double()
                    if name == 't3':
                        other = x @ L[j - 1]['w0'].double().t() + L[j - 1]['b0'].double()
                    else:
                        other = PC.ref_head_first(x, L[j - 1]['w0'], L[j - 1]['b0'], L[j - 1]['w1'], L[j - 1]['b1'])[1]
                    bad = ref.clone()
                    bad[0, :T] = other[0, :T]
                    assert not torch.equal(bad.float(), ref.float()) and PC.gate_fails(bad, ref, PC.TOL_HEAD), ('head level filter', j)
                    if kind in PC.EXACT:
                        assert not torch.equal(PC.sums_fixed(bad)[0], PC.sums_fixed(ref)[0])
                bad = ref.clone()
                bad[1, :T] = ref[0, :T]                                  # the previous image's tile after an image change
                assert not torch.equal(bad.float(), ref.float()) and PC.gate_fails(bad, ref, PC.TOL_HEAD)
                if ref.shape[1] > T:
                    bad = ref.clone()
                    k = min(T, ref.shape[1] - T)
                    bad[-1, T:T + k] = ref[-1, :k]                       # the last tile of a run left as the tile before it
                    assert not torch.equal(bad.float(), ref.float()) and PC.gate_fails(bad, ref, PC.TOL_HEAD)


@pytest.mark.parametrize('kind', PC.INSTRUMENTS)
def test_wrong_references_fail_the_comparison_stem_and_block(kind):
    """the row after a ring wrap taken from the row it overwrote (stem: ring of 10 mid rows; block: ring of 4 mid rows); a seam pixel"""
    for fmt in (0, 1):
        o = PC.stem_operands(kind, fmt, **PC.STEM_CASE)
        mid = o['stages'][1].clone()
        mid[:, PC.STEM_RING, :2 * PC.STEM_TW + 1] = o['stages'][1][:, 0, :2 * PC.STEM_TW + 1]
        y = PC.ref_conv(PC.rt(mid), o['ws'][2], o['bs'][2], 3, 2, True)
        bad = PC.ref_conv(PC.rt(y), o['ws'][3], o['bs'][3], 1, 1, True)
        assert _resolved(kind, bad, o['ref']), 'stem ring row'
        assert _resolved(kind, PC.wrong_seam_pixel(o['ref'], PC.STEM_TW, 2), o['ref']), 'stem seam pixel'
    n, h, w = PC.BLOCK_CASES[0]
    o = PC.block_operands(kind, n, h, w)
    mid = o['ref_mid'].clone()
    mid[:, PC.BLK_NMID, :PC.BLK_TW] = o['ref_mid'][:, 0, :PC.BLK_TW]
    bad = PC.ref_conv(PC.rt(mid), o['w2'], o['b2'], 3, 1, True, res=o['x'])
    assert _resolved(kind, bad, o['ref'], PC.TOL_BLOCK), 'block ring row'
    g = PC.block_geometry(n, h, w)
    assert _resolved(kind, PC.wrong_seam_pixel(o['ref'], PC.BLK_TW, g['SH']), o['ref'], PC.TOL_BLOCK), 'block seam pixel'
