"""The float64 reference, the restated launch geometry and the case tables of tests/golden/wgrad_cases.py, checked without a
GPU: wgrad_ref against torch's double-precision autograd of F.conv2d, the 2^24 condition under which the integer cases of
tests/test_gpu_wgrad.py must be bit-exact, the path every table entry claims, the coverage of every reachable path by the
tables, and that the comparisons the GPU tests make do fail for a reference that is wrong at one edge."""
import pytest
import torch
import torch.nn.functional as F

import wgrad_cases as WC


def _autograd(x, dy, ks, stride):
    wt = torch.zeros((dy.size(3), x.size(3), ks, ks), dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double().permute(0, 3, 1, 2), wt, None, stride, ks // 2).backward(dy.double().permute(0, 3, 1, 2))
    return wt.grad


SMALL = [(1, 1, 1), (1, 1, 17), (1, 9, 1), (2, 8, 16), (1, 9, 17), (3, 31, 30), (2, 16, 33), (2, 37, 53)]


@pytest.mark.parametrize('ks,stride', WC.KS_STRIDE)
def test_reference_equals_double_autograd_exactly(ks, stride, monkeypatch):
    for i, (n, h, w) in enumerate(SMALL):
        cin, cout = [(8, 8), (24, 40), (32, 64), (64, 64), (128, 8)][i % 5]
        x, dy = WC.int_operands(n, h, w, cin, cout, ks, stride, seed=i)
        assert float(x.abs().max()) <= 3 and torch.equal(x, x.round())
        ref = WC.wgrad_ref(x, dy, ks, stride)
        assert ref.dtype == torch.float64 and torch.equal(ref, _autograd(x, dy, ks, stride)), (n, h, w)
        assert torch.equal(WC.abs_ref(x, dy, ks, stride), _autograd(x.abs(), dy.abs(), ks, stride))
    # row chunks (the big maps): one output row per chunk gives the same integers
    x, dy = WC.int_operands(2, 37, 53, 32, 64, ks, stride, seed=9)
    whole = WC.wgrad_ref(x, dy, ks, stride)
    monkeypatch.setattr(WC, 'REF_CHUNK_ELEMS', 1)
    assert torch.equal(WC.wgrad_ref(x, dy, ks, stride), whole)
    # Gaussian operands: equal to autograd up to the order of the float64 sums
    monkeypatch.undo()
    x, dy = WC.gauss_operands(2, 37, 53, 64, 64, ks, stride, seed=3)
    ref, auto = WC.wgrad_ref(x, dy, ks, stride), _autograd(x, dy, ks, stride)
    assert float((ref - auto).abs().max()) <= 1e-12 * float(WC.abs_ref(x, dy, ks, stride).max())


def test_stem_reference_equals_double_autograd_exactly():
    for cin in WC.STEM_CIN:
        for n, h, w in WC.STEM_MAPS[:5]:
            x = WC.int_tensor((n, cin, h, w), h).float()
            ho, wo = WC.out_hw(h, w, 3, 2)
            assert (ho, wo) == ((h + 1) // 2, (w + 1) // 2)
            dy = WC.int_tensor((n, ho, wo, 32), w).half()
            assert torch.equal(WC.wgrad_ref(x.permute(0, 2, 3, 1), dy, 3, 2), _autograd(x.permute(0, 2, 3, 1), dy, 3, 2))


def _all_conv_cases():
    """every integer case that goes through k_wgrad -> [(case, inv_scale, |preload| bound)]"""
    out = [(c, 0.25, 0) for c in WC.edge_cases()]
    out += [(c, 1.0, 0) for c, _ in WC.PATH_CASES]
    out += [((1, 8, 16 * k, 64, 64, 1, 1), s, 3) for k in WC.FINAL_ROWS for s in WC.FINAL_INV_SCALES]
    out += [(WC.ODD_CHANNEL_MAP + ch + kss, 1.0, 0) for ch in WC.ODD_CHANNELS for kss in WC.ODD_CHANNEL_KS_STRIDE]
    out += [(c, s, 3) for _, c, s in WC.DEFERRED_JOBS]
    return out


def test_integer_cases_stay_below_2_to_the_24():
    for c, inv_scale, preload in _all_conv_cases():
        g = WC.geometry(*c)
        assert WC.exact_cap(c[0] * g['ho'] * g['wo'], inv_scale, preload) < WC.EXACT_LIMIT, c
    jobs = {name: (c, s) for name, c, s in WC.DEFERRED_JOBS}
    chained = sum(c[0] * WC.geometry(*c)['ho'] * WC.geometry(*c)['wo'] for c in (jobs['level0'][0], jobs['level1'][0]))
    assert jobs['level0'][1] == jobs['level1'][1] and WC.exact_cap(chained, jobs['level0'][1], 3) < WC.EXACT_LIMIT
    for n, h, w in WC.STEM_MAPS:
        ho, wo = WC.out_hw(h, w, 3, 2)
        assert WC.exact_cap(n * ho * wo, 0.5, 3) < WC.EXACT_LIMIT
    for r in WC.DEFERRED_ROWSUMS:
        assert 3 * r['nrows'] + 3 < WC.EXACT_LIMIT and r['row_stride'] > r['count']
    # the cap really is what the data can reach: all-(+-3) operands on one of the cases
    c = (2, 8, 16, 64, 64, 3, 1)
    x, dy = torch.full((2, 8, 16, 64), 3.0).half(), torch.full((2, 8, 16, 64), -3.0).half()
    assert float(WC.wgrad_ref(x, dy, 3, 1).abs().max()) == WC.exact_cap(2 * 8 * 16)


def test_every_table_entry_is_on_the_path_it_claims():
    for c, path in WC.PATH_CASES:
        g = WC.geometry(*c)
        assert g['path'] == path, (c, g)
        assert g['tiles'] > g['rows'], (c, g)                          # the persistent loop takes a second trip
        # ragged right and bottom tiles (the 1024-row map: 512 output rows, ragged on the right only)
        assert g['wo'] % 16 and (g['ho'] % 8 or c[:3] == (1, 1024, 1000)), (c, g)
        assert g['rows'] * g['blocks'] * c[5] * c[5] <= WC.WG_MAX * 4 * 9, (c, g)      # the partials fit the workspace
    assert any(c[0] == 2 for c, _ in WC.PATH_CASES)
    # the two shapes tests/test_gpu_train_convs.py runs, the rows of the issue's table
    for c, rows, tiles in [((2, 37, 53, 64, 64, 3, 1), 40, 40), ((4, 80, 80, 64, 64, 3, 1), 40, 200),
                           ((1, 129, 257, 128, 128, 3, 1), 256, 289), ((2, 129, 257, 64, 64, 3, 1), 256, 578),
                           ((2, 297, 297, 64, 128, 3, 2), 256, 380), ((1, 1024, 1000, 64, 64, 3, 2), 341, 2048),
                           ((1, 257, 259, 128, 128, 1, 1), 128, 561), ((1, 515, 510, 128, 128, 1, 1), 256, 2080)]:
        g = WC.geometry(*c)
        assert (g['rows'], g['tiles']) == (rows, tiles), (c, g)
    for k in WC.FINAL_ROWS:
        g = WC.geometry(1, 8, 16 * k, 64, 64, 1, 1)
        assert g['path'] == '1x1_256' and g['rows'] == g['tiles'] == k and g['blocks'] == 1
    for c in WC.edge_cases():
        assert WC.geometry(*c)['path'] in ('tap_split', '1x1_256'), c
    for cin in WC.XPRO_CIN:
        assert WC.geometry(*(WC.XPRO_MAP + (cin, WC.XPRO_COUT, 1, 1)))['path'] == '1x1_256'
    blocks = [WC.geometry(*c)['blocks'] * c[5] * c[5] for _, c, _ in WC.DEFERRED_JOBS]
    assert len(set(blocks)) >= 3                                           # jobs of different block counts in one launch
    n, h, w = WC.STEM_MAPS[-1]
    for cin in WC.STEM_CIN:
        rows, ksteps = WC.stem_rows(n, h, w, cin)
        assert ksteps > 4096 and rows == WC.STEM_ROW_CAP
        assert all(WC.stem_rows(*m, cin)[0] < WC.STEM_ROW_CAP for m in WC.STEM_MAPS[:-1])


def test_the_tables_cover_every_reachable_path():
    cases = WC.edge_cases() + [c for c, _ in WC.PATH_CASES]
    for kss in WC.KS_STRIDE:
        mine = [WC.geometry(*c) for c in cases if c[5:] == kss]
        for path in WC.REACHABLE[kss]:
            assert any(g['path'] == path and g['tiles'] > g['rows'] for g in mine), (kss, path)
        assert any(g['tiles'] <= g['rows'] for g in mine), kss
        assert {g['path'] for g in mine} <= set(WC.REACHABLE[kss])
    # stride 2: every parity of (h, w)
    maps = WC.EDGE_MAPS + WC.EDGE_MAPS_S2
    assert {(h % 2, w % 2) for _, h, w in maps} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # every Gaussian case is a path case or the small map
    assert {WC.geometry(*c)['path'] for c in WC.GAUSS_CASES} == {p for v in WC.REACHABLE.values() for p in v}


def _wrong_refs(x, dy, ks, stride):
    """references that are wrong at ONE place: the bottom row of x taken for padding, the right column likewise, the last output
    pixel of the last image dropped, one tap transposed"""
    xb, xr, d = x.clone(), x.clone(), dy.clone()
    xb[:, -1] = 0
    xr[:, :, -1] = 0
    d[-1, -1, -1] = 0
    out = dict(bottom=WC.wgrad_ref(xb, dy, ks, stride), right=WC.wgrad_ref(xr, dy, ks, stride), pixel=WC.wgrad_ref(x, d, ks, stride))
    if ks == 3:
        out['taps'] = WC.wgrad_ref(x, dy, ks, stride).transpose(2, 3).contiguous()
    return out


@pytest.mark.parametrize('ks,stride', WC.KS_STRIDE)
def test_a_wrong_reference_fails_both_comparisons(ks, stride):
    """the two assertions of tests/test_gpu_wgrad.py -- torch.equal on integer operands, the elementwise bound on Gaussian ones --
    with the true result in the kernel's place and a deliberately wrong reference: each must fail.  (Odd maps: at stride 2 the
    bottom row and right column of an even map are read by no tap.)"""
    c = (2, 37, 53, 64, 64, ks, stride)
    g = WC.geometry(*c)
    x, dy = WC.small_int_operands(c)
    good = WC.wgrad_ref(x, dy, ks, stride)
    for what, bad in _wrong_refs(x, dy, ks, stride).items():
        assert not torch.equal(good.float().double(), bad), what
    x, dy = WC.gauss_operands(*c, seed=1)
    good, a = WC.wgrad_ref(x, dy, ks, stride), WC.abs_ref(x, dy, ks, stride)
    got = good.float().double()                       # a kernel that is as good as fp32 allows
    assert bool(((got - good).abs() <= WC.gauss_bound(good, a, g['tiles'], g['rows'])).all())
    for what, bad in _wrong_refs(x, dy, ks, stride).items():
        assert not bool(((got - bad).abs() <= WC.gauss_bound(bad, WC.abs_ref(x, dy, ks, stride), g['tiles'], g['rows'])).all()), what
