"""The conv weight-gradient kernels (csrc/train.hip: k_wgrad<KS, S, XPRO>, k_wgrad_final, k_wgrad_final_batched,
k_rows_sum_batched, k_conv0_wgrad_mfma + k_sum_partials; csrc/stem_gray_train.hip: the grayscale first conv) on every path
wgrad_geometry() dispatches to, against the float64 reference of tests/golden/wgrad_cases.py (checked on the CPU by
tests/test_wgrad_reference_host.py).

Integer cases: operands hold integers in [-3, 3], every partial sum stays below 2^24, so the kernels must equal the reference
BIT FOR BIT -- a missing or doubled pixel, a wrong tap, a wrong edge, a wrong row of the final sum or a wrong block mapping
changes at least one integer.  Every case also asserts that lfd_conv_wgrad_partial_rows reports the rows and blocks the restated
geometry predicts: if the thresholds move, the tables stop claiming paths they no longer reach.

Gaussian cases (rounding behaviour): |got - ref| <= L * 2^-23 * A + 2^-24 * |ref| elementwise, A = the same contraction over
|x| and |dy|, L = 128 * ceil(tiles / rows) = the pixels one workgroup accumulates in fp32 before the fp64 pass.  The factor is
2^-23 and not fp32's unit roundoff 2^-24 because the accumulation inside the MFMA may not round to nearest; how it rounds has
not been measured on this hardware.  The bound comes from that reasoning alone, not from what the kernels deliver."""
import pytest
import torch

import wgrad_cases as WC
from lfd_amd import ops

pytestmark = pytest.mark.gpu


def _check_geometry(x, dy, c):
    g = WC.geometry(*c)
    floats, rows, blocks = ops.conv_wgrad_partial_floats(x, dy, c[5], c[6])
    assert (rows, blocks) == (g['rows'], g['blocks']), (c, g, rows, blocks)
    assert floats == rows * blocks * c[5] * c[5] * 4096
    return g


def _assert_exact(got, ref, what):
    assert got.dtype == torch.float32 and got.shape == ref.shape, what
    bad = got.double() != ref
    assert not bool(bad.any()), '%s: %d of %d entries differ, first at %s: got %s, reference %s' % (
        what, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist(), float(got[bad][0]), float(ref[bad][0]))
    assert torch.equal(got.double(), ref)


def _assert_within(got, ref, bound, what):
    err = (got.double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print('%s: max error / bound %.3g (max error %.3g)' % (what, worst, float(err.max())))
    assert bool((err <= bound).all()), (what, worst)


# ------------------------------------------------------------------------------------------------ (a) edges of every path
@pytest.mark.parametrize('c', WC.edge_cases(), ids=WC.case_id)
def test_edges_of_every_path_are_exact(c):
    x, dy = (t.cuda() for t in WC.small_int_operands(c))
    _check_geometry(x, dy, c)
    got = ops.conv_wgrad(x, dy, c[5], c[6], 0.25)
    _assert_exact(got, WC.wgrad_ref(x, dy, c[5], c[6]) * 0.25, WC.case_id(c))


# ------------------------------------------------------------------------------------------------ (b) the large-operand paths
@pytest.mark.parametrize('c,path', WC.PATH_CASES, ids=[WC.case_id(c) for c, _ in WC.PATH_CASES])
def test_paths_above_the_size_thresholds_are_exact(c, path):
    x, dy = (t.cuda() for t in WC.int_operands(*c, seed=WC.case_seed(c)))
    g = _check_geometry(x, dy, c)
    assert g['path'] == path and g['tiles'] > g['rows']
    print('%s: path %s, rows %d, blocks %d, tiles %d' % (WC.case_id(c), path, g['rows'], g['blocks'], g['tiles']))
    got = ops.conv_wgrad(x, dy, c[5], c[6], 1.0)
    _assert_exact(got, WC.wgrad_ref(x, dy, c[5], c[6]), WC.case_id(c))


# ------------------------------------------------------------------------------------------------ (c) rows of the final sum
@pytest.mark.parametrize('inv_scale', WC.FINAL_INV_SCALES)
@pytest.mark.parametrize('k', WC.FINAL_ROWS)
def test_final_sum_over_every_row_count_is_exact(k, inv_scale):
    """k_wgrad_final: rows = k walks the 8-way unrolled loop (g + 56 < rows), the remainder loop and their boundaries"""
    c = (1, 8, 16 * k, 64, 64, 1, 1)
    x, dy = (t.cuda() for t in WC.int_operands(*c, seed=k))
    g = _check_geometry(x, dy, c)
    assert g['rows'] == k
    ref = WC.wgrad_ref(x, dy, 1, 1) * inv_scale
    _assert_exact(ops.conv_wgrad(x, dy, 1, 1, inv_scale), ref, 'rows %d' % k)
    pre = WC.int_preload((64, 64, 1, 1), k).cuda()
    dw = pre.clone()
    assert ops.conv_wgrad(x, dy, 1, 1, inv_scale, out=dw, accumulate=True) is dw
    _assert_exact(dw, ref + pre.double(), 'rows %d, accumulate' % k)


# ------------------------------------------------------------------------------------------------ (d) other channel counts
@pytest.mark.parametrize('ks,stride', WC.ODD_CHANNEL_KS_STRIDE)
@pytest.mark.parametrize('cin,cout', WC.ODD_CHANNELS)
def test_channel_counts_that_are_no_multiple_of_32_are_exact(cin, cout, ks, stride):
    c = WC.ODD_CHANNEL_MAP + (cin, cout, ks, stride)
    x, dy = (t.cuda() for t in WC.int_operands(*c, seed=WC.case_seed(c)))
    _check_geometry(x, dy, c)
    guard = torch.full((cout * cin * ks * ks + 128,), 7.0, device='cuda')          # nothing is written behind dW
    dw = guard[:cout * cin * ks * ks].view(cout, cin, ks, ks)
    ops.conv_wgrad(x, dy, ks, stride, 1.0, out=dw)
    _assert_exact(dw, WC.wgrad_ref(x, dy, ks, stride), WC.case_id(c))
    assert bool((guard[cout * cin * ks * ks:] == 7.0).all())


# ------------------------------------------------------------------------------------------------ (e) the deferred final stage
def test_deferred_finals_of_one_launch_are_exact():
    """ops.conv_wgrad_partials + ONE ops.WgradFinals.launch(): a 3x3 and a 1x1 job of different block counts (first_block
    lookup), two partial sets chained into one dW (a conv shared by two pyramid levels; the chain's second set is added after
    two unrelated jobs), one conv whose rows go to two parameters, two row-sum jobs.  Every target is accumulated into
    (WgradFinals always adds) and equals its float64 reference exactly; the unchained ones equal ops.conv_wgrad bit for bit."""
    fin = ops.WgradFinals(torch.device('cuda', torch.cuda.current_device()))
    jobs, keep = {}, []
    shared = WC.int_preload((64, 64, 3, 3), 77).cuda()
    shared_ref = shared.double()
    for i, (name, c, inv) in enumerate(WC.DEFERRED_JOBS):
        n, h, w, cin, cout, ks, stride = c
        x, dy = (t.cuda() for t in WC.int_operands(*c, seed=300 + i))
        g = _check_geometry(x, dy, c)
        floats, rows, blocks = ops.conv_wgrad_partial_floats(x, dy, ks, stride)
        part = torch.full((floats,), float('nan'), device='cuda')                    # every float of it is written
        ops.conv_wgrad_partials(x, dy, ks, stride, part)
        ref = WC.wgrad_ref(x, dy, ks, stride) * inv
        keep.append(part)
        if name.startswith('level'):
            fin.add_wgrad(part, rows, blocks, cin, cout, ks * ks, inv, [(shared, 0, cout)])
            shared_ref = shared_ref + ref
            continue
        slices = WC.DEFERRED_SLICES if name == 'sliced' else [(0, cout)]
        pre = [WC.int_preload((hi - lo, cin, ks, ks), 400 + i + lo).cuda() for lo, hi in slices]
        dws = [p.clone() for p in pre]
        fin.add_wgrad(part, rows, blocks, cin, cout, ks * ks, inv, [(d, lo, hi) for d, (lo, hi) in zip(dws, slices)])
        direct = ops.conv_wgrad(x, dy, ks, stride, inv, out=torch.cat(pre, 0), accumulate=True)
        jobs[name] = (dws, pre, slices, ref, direct, g)
    levels = [WC.geometry(*c) for name, c, _ in WC.DEFERRED_JOBS if name.startswith('level')]
    assert levels[0]['rows'] != levels[1]['rows'] and levels[0]['blocks'] == levels[1]['blocks']
    rows = []
    for i, r in enumerate(WC.DEFERRED_ROWSUMS):
        src = WC.int_tensor((r['nrows'], r['row_stride']), 500 + i).float().cuda()
        pre = WC.int_preload((r['count'] + 5,), 600 + i).cuda()
        dst = pre.clone()
        fin.add_rowsum(src, r['nrows'], r['row_stride'], r['count'], dst, r['accumulate'])
        rows.append((src, pre, dst, r))
    fin.launch()
    torch.cuda.synchronize()
    for name, (dws, pre, slices, ref, direct, g) in jobs.items():
        for d, p, (lo, hi) in zip(dws, pre, slices):
            _assert_exact(d, ref[lo:hi] + p.double(), '%s rows %d..%d' % (name, lo, hi))
        assert torch.equal(torch.cat(dws, 0), direct), name
    _assert_exact(shared, shared_ref, 'chained levels')
    for src, pre, dst, r in rows:
        ref = src.double()[:, :r['count']].sum(0) + (pre.double()[:r['count']] if r['accumulate'] else 0)
        _assert_exact(dst[:r['count']], ref, 'row sum of %d x %d' % (r['nrows'], r['count']))
        assert torch.equal(dst[r['count']:], pre[r['count']:])                   # nothing behind `count`


# ------------------------------------------------------------------------------------------------ (f) the re-formed operand
@pytest.mark.parametrize('cin', WC.XPRO_CIN)
def test_wgrad_of_an_unstored_bn_relu_activation_is_bit_identical(cin):
    """lfd_conv1x1_wgrad_partials_of_bn_relu_f16 (k_wgrad<1, 1, XPRO>) at 32 and 128 input channels against the plain kernel on
    the stored lfd_bn_train_apply_f16 output (tests/test_gpu_train_convs.py fixes 64)"""
    n, h, w = WC.XPRO_MAP
    g = torch.Generator().manual_seed(5 + cin)
    yin = (torch.randn(n, h, w, cin, generator=g) * 1.3 + 0.2).half().cuda()
    pg, pb = (torch.rand(cin, generator=g) + 0.5).cuda(), (torch.randn(cin, generator=g) * 0.3).cuda()
    dy = (torch.randn(n, h, w, WC.XPRO_COUT, generator=g) * 0.5).half().cuda()
    pstats = ops.bn_train_stats(yin, 1e-5, 0.1, None, None)
    z = ops.bn_train_apply(yin, pstats, pg, pb, None, True)
    _check_geometry(z, dy, WC.XPRO_MAP + (cin, WC.XPRO_COUT, 1, 1))
    floats, _, _ = ops.conv_wgrad_partial_floats(z, dy, 1, 1)
    pa, pb_ = torch.full((floats,), 1.0, device='cuda'), torch.full((floats,), 2.0, device='cuda')
    ops.conv_wgrad_partials(z, dy, 1, 1, pa)
    ops.conv1x1_wgrad_partials_of_bn_relu(yin, pstats, pg, pb, dy, pb_)
    assert float(pa.abs().max()) > 0 and torch.equal(pa, pb_)


# ------------------------------------------------------------------------------------------------ (g) the first conv
@pytest.mark.parametrize('nhw', WC.STEM_MAPS, ids=lambda m: '%dx%dx%d' % m)
@pytest.mark.parametrize('c', WC.STEM_CHANNELS)
@pytest.mark.parametrize('cin', WC.STEM_CIN)
def test_first_conv_wgrad_is_exact(cin, c, nhw):
    """ops.stem_conv0_wgrad (3-channel: k_conv0_wgrad_mfma + k_sum_partials; grayscale: csrc/stem_gray_train.hip) on
    integer-valued fp32 images against the shifted-matmul reference at stride 2, pad 1; the largest map runs the capped 1024
    partial rows"""
    n, h, w = nhw
    ho, wo = WC.out_hw(h, w, 3, 2)
    x = WC.int_tensor((n, cin, h, w), 700 + h + cin).float().cuda()
    dy = WC.int_tensor((n, ho, wo, c), 800 + w + c).half().cuda()
    ref = WC.wgrad_ref(x.permute(0, 2, 3, 1), dy, 3, 2) * 0.5
    got = ops.stem_conv0_wgrad(x, dy, 0.5)
    _assert_exact(got, ref, 'first conv %d -> %d on %s' % (cin, c, nhw))
    pre = WC.int_preload((c, cin, 3, 3), h).cuda()
    dw = pre.clone()
    ops.stem_conv0_wgrad(x, dy, 0.5, out=dw, accumulate=True)
    _assert_exact(dw, ref + pre.double(), 'first conv %d -> %d on %s, accumulate' % (cin, c, nhw))


# ------------------------------------------------------------------------------------------------ (h) rounding behaviour
@pytest.mark.parametrize('c', WC.GAUSS_CASES, ids=WC.case_id)
def test_rounding_on_gaussian_operands_stays_within_the_fp32_bound(c):
    x, dy = (t.cuda() for t in WC.gauss_operands(*c, seed=WC.case_seed(c)))
    g = _check_geometry(x, dy, c)
    got = ops.conv_wgrad(x, dy, c[5], c[6], 1.0)
    ref, a = WC.wgrad_ref(x, dy, c[5], c[6]), WC.abs_ref(x, dy, c[5], c[6])
    _assert_within(got, ref, WC.gauss_bound(ref, a, g['tiles'], g['rows']),
                   '%s: path %s, rows %d, tiles %d' % (WC.case_id(c), g['path'], g['rows'], g['tiles']))
