"""The forward conv kernels (csrc/conv_impl.h through csrc/conv.hip, conv_stats.hip, conv_acc32.hip; csrc/conv_small.hip and
csrc/dgrad_s2.hip beside them) against the float64 reference of tests/golden/conv_cases.py, on every dispatch key, at shapes
that walk the persistent tile loop (1044 tiles on 512 workgroups: first, second and third tile of a workgroup) and at maps
with interior, ragged and corner tiles.

On INTEGER operands (conv_cases.py: the instrument) the kernel must equal the reference bit for bit: every assertion on them
is torch.equal.  On Gaussian operands the gate is the one of tests/test_gpu_conv.py, 1.2e-3 * max(|ref|, 1).  Outputs that the
entry point lets the caller place are written into a view of a sentinel-filled buffer whose guards must stay untouched.
tests/test_conv_reference_host.py shows, without a GPU, that each of five wrong references (a dropped tap on the bottom row /
right column, a pixel from the previous image, transposed taps, a stale halo) fails these very comparisons on every case."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import pytest
import torch

import conv_cases as CC
from lfd_amd import _lib, ops
from lfd_amd._lib import check, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu

SENTINEL = -12344.0            # an fp16 value no case produces (|outputs| <= 2048)


def _cuda(o):
    return CC.Operands(*[None if t is None else t.cuda() for t in o])


def _packs(o):
    """-> (w, tail (w2, b2) or None, wd) packed on the device"""
    return (ops.pack_conv_weight(o.w).cuda(), None if o.w2 is None else ops.pack_conv_weight(o.w2).cuda(),
            ops.pack_conv_weight(o.wd).cuda())


class Guarded(object):
    """an output placed in the middle of a sentinel-filled buffer: one map's worth of guard on each side, 16-byte aligned"""

    def __init__(self, shape, dtype=torch.float16):
        n = 1
        for s in shape:
            n *= s
        self.guard = n // shape[0]
        assert (self.guard * torch.empty((), dtype=dtype).element_size()) % 16 == 0
        self.buf = torch.full((n + 2 * self.guard,), SENTINEL, dtype=dtype, device='cuda')
        self.view = self.buf[self.guard:self.guard + n].view(shape)
        assert self.view.data_ptr() % 16 == 0

    def untouched(self):
        g = self.guard
        return bool((self.buf[:g] == SENTINEL).all()) and bool((self.buf[-g:] == SENTINEL).all())


def _explain(got, ref, geo):
    """where an integer comparison failed: the tile, the place inside it and the workgroup iteration"""
    bad = (got.double() != ref).nonzero()
    n, oh, ow, _ = ref.shape
    lc = CC.conv_launch(n, oh, ow, geo)
    wk = CC.walk(lc.ntiles, lc.blocks)
    where = {t: (b, i) for b, tiles in enumerate(wk) for i, t in enumerate(tiles)}
    img, oy, ox, ch = bad[0].tolist()
    t = img * lc.tiles_x * lc.tiles_y + (oy // geo.TH) * lc.tiles_x + ox // geo.TW
    tiles = sorted({int(i * lc.tiles_x * lc.tiles_y + (y // geo.TH) * lc.tiles_x + x // geo.TW) for i, y, x, _ in bad[:4096].tolist()})
    return ('%d of %d elements differ; first at image %d pixel (%d, %d) channel %d: got %s, reference %s; tile %d (row %d, column %d inside '
            'it) = iteration %d of workgroup %d; iterations of the first wrong tiles: %s'
            % (bad.size(0), ref.numel(), img, oy, ox, ch, float(got[img, oy, ox, ch]), float(ref[img, oy, ox, ch]), t, oy % geo.TH, ox % geo.TW,
               where[t][1], where[t][0], [where[k][1] for k in tiles[:16]]))


def _assert_exact(got, ref, geo):
    assert got.shape == ref.shape
    assert torch.equal(got.double(), ref), _explain(got, ref, geo)


def _gate_ratio(got, ref):
    """the worst |got - ref| over the gate of tests/test_gpu_conv.py"""
    return float(((got.double() - ref).abs() / (CC.GAUSS_GATE * ref.abs().clamp(min=1.0))).max())


def _run_conv(c, o, out=None):
    """ops.conv2d_nhwc on the operands of a plain / res / tail case"""
    d = _cuda(o)
    w, w2, _ = _packs(o)
    return ops.conv2d_nhwc(d.x, w, d.b, c.cin, c.cout, c.ks, c.stride, bool(c.relu), residual=d.res if c.variant == 'res' else None,
                           tail=(w2, d.b2, bool(c.relu2)) if c.variant == 'tail' else None, out=out), d


def _walk_stats(c):
    geo = CC.key_geometry(CC.case_key(c))
    oh, ow = CC.out_hw(c.h, c.w, c.ks, c.stride)
    lc = CC.conv_launch(c.n, oh, ow, geo)
    return lc.ntiles, lc.blocks, max(len(t) for t in CC.walk(lc.ntiles, lc.blocks))


# ------------------------------------------------------------------------------------------------ lfd_conv2d_nhwc_f16
@pytest.mark.parametrize('c', CC.conv_cases(), ids=CC.case_id)
def test_conv_is_exact_on_integer_operands(c):
    """every key of conv_dispatch x (plain | residual | chained 1x1) x (walk | map): equal to the float64 reference, nothing
    written outside the output, and the walk cases the same bits on a second run"""
    o = CC.case_int_operands(c)
    oh, ow = CC.out_hw(c.h, c.w, c.ks, c.stride)
    g = Guarded((c.n, oh, ow, c.cout))
    got, d = _run_conv(c, o, out=g.view)
    torch.cuda.synchronize()
    ref = CC.case_ref(c, d)
    assert float(ref.abs().max()) <= CC.exact_cap(c)
    _assert_exact(got, ref, CC.key_geometry(CC.case_key(c)))
    assert g.untouched()
    if c.kind == 'walk':
        again, _ = _run_conv(c, o)
        assert torch.equal(again, got)


@pytest.mark.parametrize('c', CC.conv_cases(), ids=CC.case_id)
def test_conv_passes_the_gate_on_gaussian_operands(c):
    o = CC.case_gauss_operands(c)
    got, d = _run_conv(c, o)
    ref = CC.case_ref(c, d)
    ratio = _gate_ratio(got, ref)
    print('GATE %s ntiles=%d blocks=%d max_tiles_per_workgroup=%d worst_error_over_gate=%.3f' % ((CC.case_id(c),) + _walk_stats(c) + (ratio,)))
    assert ratio <= 1.0


@pytest.mark.parametrize('key', CC.DISPATCH_KEYS, ids=CC.key_id)
def test_conv_edge_shapes(key):
    """one pixel, exactly one tile, one column / one row more than a tile, odd / even / mixed inputs under stride 2, nine tiles
    on sixteen workgroups (three XCD ranges empty): integer operands exact, Gaussian operands inside the gate, guards untouched"""
    geo = CC.key_geometry(key)
    for n, h, w in CC.edge_shapes(key):
        for relu in (0, 1):
            c = CC.Case(*key, 'tail' if key[4] else 'plain', 'edge', n, h, w, relu, relu)
            o = CC.case_int_operands(c)
            oh, ow = CC.out_hw(h, w, c.ks, c.stride)
            g = Guarded((n, oh, ow, c.cout))
            got, d = _run_conv(c, o, out=g.view)
            _assert_exact(got, CC.case_ref(c, d), geo)
            assert g.untouched(), (n, h, w)
        o = CC.case_gauss_operands(c)
        got, d = _run_conv(c, o)
        assert _gate_ratio(got, CC.case_ref(c, d)) <= 1.0, (n, h, w)


# ------------------------------------------------------------------------------------------------ data-gradient packs
@pytest.mark.parametrize('fwd_stride,kind', [(1, 'walk'), (1, 'map'), (2, 'map')])
@pytest.mark.parametrize('key', CC.DGRAD_KEYS, ids=CC.key_id)
def test_data_gradient_pack_through_the_forward_kernel_is_exact(key, fwd_stride, kind):
    """the kernel of key (cin, ks, 1, cout) run as the data gradient of a conv cout -> cin (stride 1, or stride 2 through
    zero_insert2): ops.pack_conv_weight_train(w, data_gradient=True), the residual = the gradient already collected, against the
    float64 transposed convolution"""
    cin_k, ks, _, cout_k, _ = key
    n, h, w = CC.walk_shape(key) if kind == 'walk' else CC.map_shape(key)
    oh, ow = CC.out_hw(h, w, ks, fwd_stride)
    seed = cin_k + 3 * cout_k + 7 * ks + 11 * fwd_stride
    wt = CC.int_tensor((cin_k, cout_k, ks, ks), CC.W_HI, seed).float().cuda()          # the forward conv's filter: cout_k -> cin_k
    dy = CC.int_tensor((n, oh, ow, cin_k), CC.X_HI, seed + 1).half().cuda()
    acc = CC.int_tensor((n, h, w, cout_k), CC.RES_HI, seed + 2).half().cuda()
    pack = ops.pack_conv_weight_train(wt, data_gradient=True)
    assert torch.equal(pack, ops.pack_conv_weight(wt.flip(2, 3).transpose(0, 1).cpu()).cuda())
    dz = ops.zero_insert2(dy, h, w) if fwd_stride == 2 else dy
    g = Guarded((n, h, w, cout_k))
    got = ops.conv2d_nhwc(dz, pack, torch.zeros(cout_k, device='cuda'), cin_k, cout_k, ks, 1, False, residual=acc, out=g.view)
    ref = CC.dgrad_ref(dy, wt, h, w, fwd_stride, residual=acc)
    assert float(ref.abs().max()) <= CC.F16_EXACT
    _assert_exact(got, ref, CC.key_geometry(key))
    assert g.untouched()
    if kind == 'walk':
        assert torch.equal(ops.conv2d_nhwc(dz, pack, torch.zeros(cout_k, device='cuda'), cin_k, cout_k, ks, 1, False, residual=acc), got)


# ------------------------------------------------------------------------------------------------ csrc/dgrad_s2.hip
def _dgrad_s2(shape, with_res):
    n, h, w = shape
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    dy = CC.int_tensor((n, oh, ow, 64), CC.X_HI, h * 100 + w).half().cuda()
    wt = CC.int_tensor((64, 64, 3, 3), CC.W_HI, 7).float().cuda()
    res = CC.int_tensor((n, h, w, 64), CC.RES_HI, 9).half().cuda() if with_res else None
    pack = ops.pack_conv_weight_train(wt, data_gradient=True)
    got = ops.conv3x3s2_dgrad(dy, pack, h, w, residual=res)
    ref = CC.dgrad_ref(dy, wt, h, w, 2, residual=res)
    assert float(ref.abs().max()) <= CC.F16_EXACT
    _assert_exact(got, ref, CC.key_geometry((64, 3, 1, 64, 0)))       # (reported in tiles of dx; the kernel's own are 8 x 16 of dy)
    zi = ops.conv2d_nhwc(ops.zero_insert2(dy, h, w), pack, torch.zeros(64, device='cuda'), 64, 64, 3, 1, False, residual=res)
    assert torch.equal(got, zi)
    return got, (dy, pack, res)


@pytest.mark.parametrize('with_res', [False, True])
def test_stride2_data_gradient_walk(with_res):
    """174 images of 18 x 66: 1044 dy tiles on 512 workgroups -- exact, equal to the zero-inserted conv, the same bits twice"""
    n, h, w = CC.DGRAD_S2_WALK
    got, (dy, pack, res) = _dgrad_s2(CC.DGRAD_S2_WALK, with_res)
    assert torch.equal(ops.conv3x3s2_dgrad(dy, pack, h, w, residual=res), got)


@pytest.mark.parametrize('shape', CC.DGRAD_S2_EDGES, ids=lambda s: '%dx%dx%d' % s)
def test_stride2_data_gradient_edges(shape):
    for with_res in (False, True):
        _dgrad_s2(shape, with_res)


# ------------------------------------------------------------------------------------------------ csrc/conv_small.hip
_SPLITK_CHILD = '''
import sys
sys.path[:0] = [%r, %r]
import torch
import conv_cases as CC
from lfd_amd import ops
outs = []
for n, h, w in CC.SPLITK_SHAPES:
    for variant, relu in (('res', 1), ('plain', 0)):
        c = CC.Case(*CC.SPLITK_KEY, variant, 'map', n, h, w, relu, 0)
        o = CC.case_int_operands(c)
        outs.append(ops.conv2d_nhwc(o.x.cuda(), ops.pack_conv_weight(o.w).cuda(), o.b.cuda(), 128, 128, 3, 1, bool(relu),
                                    residual=o.res.cuda() if variant == 'res' else None).cpu())
torch.save(outs, sys.argv[1])
'''


def test_split_k_and_streamed_weight_kernels_are_exact_and_bit_equal():
    """128 -> 128 3x3 s1 on integer operands at 17 x 30 (1 and 8 images), 23 x 40, 16384 pixels (the last split-K size) and 16512
    (the first streamed-weight size), with residual + ReLU and bare: LFD_CONV128_SPLITK=1 and =0 (fresh child processes) both
    equal the float64 reference, hence each other, bit for bit"""
    here = os.path.dirname(os.path.abspath(__file__))
    code = _SPLITK_CHILD % (os.path.join(here, 'golden'), os.path.dirname(os.path.dirname(ops.__file__)))
    outs = []
    for flag in ('1', '0'):
        with tempfile.NamedTemporaryFile(suffix='.pt') as f:
            r = subprocess.run([sys.executable, '-c', code, f.name], env=dict(os.environ, LFD_CONV128_SPLITK=flag), capture_output=True,
                               text=True, timeout=300)
            assert r.returncode == 0, r.stderr[-2000:]
            outs.append(torch.load(f.name))
    i = 0
    geo = CC.key_geometry(CC.SPLITK_KEY)
    for n, h, w in CC.SPLITK_SHAPES:
        for variant, relu in (('res', 1), ('plain', 0)):
            c = CC.Case(*CC.SPLITK_KEY, variant, 'map', n, h, w, relu, 0)
            ref = CC.case_ref(c, _cuda(CC.case_int_operands(c)))
            assert float(ref.abs().max()) <= CC.F16_EXACT
            for k in (0, 1):
                _assert_exact(outs[k][i].cuda(), ref, geo)
            assert torch.equal(outs[0][i], outs[1][i])
            i += 1
    # the parent process itself (default switch): the kernel the threshold picks
    for n, h, w in CC.SPLITK_SHAPES[3:]:
        c = CC.Case(*CC.SPLITK_KEY, 'res', 'map', n, h, w, 1, 0)
        got, d = _run_conv(c, CC.case_int_operands(c))
        _assert_exact(got, CC.case_ref(c, d), geo)


# ------------------------------------------------------------------------------------------------ lfd_conv2d_downsample_nhwc_f16
def _run_ds(c, o):
    d = _cuda(o)
    w, _, wd = _packs(o)
    oh, ow = CC.out_hw(c.h, c.w, 3, 2)
    g, gd = Guarded((c.n, oh, ow, c.cout)), Guarded((c.n, oh, ow, c.cout))
    desc = _lib.ConvDesc(c.n, c.h, c.w, c.cin, c.cout, 3, 2, c.relu, 0, 0)
    check(lib().lfd_conv2d_downsample_nhwc_f16(C.byref(desc), ptr(d.x), ptr(g.view), ptr(w), ptr(d.b), ptr(wd), ptr(d.bd), ptr(gd.view),
                                               ptr(ops.zero_line(d.x.device)), stream_ptr()), 'lfd_conv2d_downsample_nhwc_f16')
    torch.cuda.synchronize()
    return g, gd, d, (w, wd)


@pytest.mark.parametrize('c', CC.ds_cases(), ids=CC.case_id)
def test_conv_with_downsample_branch_is_exact(c):
    """3x3 s2 and the block's 1x1 s2 identity branch from one launch, all four keys, walk and map: both outputs exact on integer
    operands and inside the gate on Gaussian ones, guards untouched, the same bits twice; ops.conv2d_downsample_nhwc (square
    keys) returns the same two tensors"""
    geo = CC.key_geometry(CC.case_key(c))
    o = CC.case_int_operands(c)
    g, gd, d, (w, wd) = _run_ds(c, o)
    ref, refd = CC.case_ref(c, d)
    assert max(float(ref.abs().max()), float(refd.abs().max())) <= CC.F16_EXACT
    _assert_exact(g.view, ref, geo)
    _assert_exact(gd.view, refd, geo)
    assert g.untouched() and gd.untouched()
    g2, gd2, _, _ = _run_ds(c, o)
    assert torch.equal(g2.view, g.view) and torch.equal(gd2.view, gd.view)
    if c.cin == c.cout:
        a, b = ops.conv2d_downsample_nhwc(d.x, w, d.b, wd, d.bd, relu=bool(c.relu))
        assert torch.equal(a, g.view) and torch.equal(b, gd.view)
    g, gd, d, _ = _run_ds(c, CC.case_gauss_operands(c))
    ref, refd = CC.case_ref(c, d)
    ratios = _gate_ratio(g.view, ref), _gate_ratio(gd.view, refd)
    print('GATE %s ntiles=%d blocks=%d max_tiles_per_workgroup=%d worst_error_over_gate=%.3f' % ((CC.case_id(c),) + _walk_stats(c) + (max(ratios),)))
    assert max(ratios) <= 1.0


# ------------------------------------------------------------------------------------------------ lfd_conv2d_nhwc_f16_acc32
@pytest.mark.parametrize('c', CC.acc32_cases(), ids=CC.case_id)
def test_fp32_output_kernels_are_exact(c):
    """every ACC32 key: conv + bias as fp32, equal to the float64 reference on integer operands (any integer below 2^24 is an
    fp32); on Gaussian operands within the bound of K + 1 fp32 additions that may not round to nearest, (K + 1) * 2^-23 * (the
    sum of the magnitudes of the terms)"""
    o = CC.case_int_operands(c)
    d = _cuda(o)
    w, _, _ = _packs(o)
    got = ops.conv2d_nhwc_f32out(d.x, w, d.b, c.cin, c.cout, c.ks, c.stride)
    ref = CC.case_ref(c, d)
    assert got.dtype == torch.float32 and float(ref.abs().max()) <= CC.exact_cap(c)
    _assert_exact(got, ref, CC.key_geometry(CC.case_key(c)))
    if c.kind == 'walk':
        assert torch.equal(ops.conv2d_nhwc_f32out(d.x, w, d.b, c.cin, c.cout, c.ks, c.stride), got)
    o = CC.case_gauss_operands(c)
    d = _cuda(o)
    got = ops.conv2d_nhwc_f32out(d.x, ops.pack_conv_weight(o.w).cuda(), d.b, c.cin, c.cout, c.ks, c.stride)
    ref = CC.conv_ref(d.x, d.w, d.b, c.stride)
    mag = CC.conv_ref(d.x.abs(), d.w.abs(), d.b.abs(), c.stride)
    k = c.ks * c.ks * c.cin
    assert bool(((got.double() - ref).abs() <= (k + 1) * 2.0 ** -23 * mag + 2.0 ** -24 * ref.abs()).all())


# ------------------------------------------------------------------------------------------------ csrc/conv_stats.hip
def _tile_rows(y, c):
    """the statistics rows the walk predicts: row b = the sums of y and y^2 over the tiles workgroup b visits, int64 [blocks, 2, cout]"""
    geo = CC.key_geometry(CC.case_key(c))
    n, oh, ow, cout = y.shape
    lc = CC.conv_launch(n, oh, ow, geo)
    owner = torch.empty(lc.ntiles, dtype=torch.int64)
    for b, tiles in enumerate(CC.walk(lc.ntiles, lc.blocks)):
        owner[tiles] = b
    img = torch.arange(n).view(n, 1, 1) * (lc.tiles_x * lc.tiles_y)
    tile = img + (torch.arange(oh).view(1, oh, 1) // geo.TH) * lc.tiles_x + torch.arange(ow).view(1, 1, ow) // geo.TW
    idx = owner[tile.reshape(-1)].to(y.device)
    yi = y.reshape(-1, cout).to(torch.int64)
    rows = torch.zeros((lc.blocks, 2, cout), dtype=torch.int64, device=y.device)
    rows[:, 0].index_add_(0, idx, yi)
    rows[:, 1].index_add_(0, idx, yi * yi)
    return rows


@pytest.mark.parametrize('c', CC.stats_cases(), ids=CC.case_id)
def test_conv_with_statistics_rows_is_exact(c):
    """every STATS key on integer operands: y bit-identical to the plain conv and to the reference; every partial row equal to the
    exact integer sums of y and y^2 over the tiles the restated walk gives that workgroup (every row stays below 2^24, so its
    fp32 sums are exact in any order), their int64 total equal to the sums over the whole of y; mean / rstd of
    ops.conv2d_bn_stats against float64 at 1e-5"""
    o = CC.case_int_operands(c)
    d = _cuda(o)
    w, _, _ = _packs(o)
    zb = torch.zeros(c.cout, device='cuda')
    y0 = ops.conv2d_nhwc(d.x, w, zb, c.cin, c.cout, c.ks, c.stride, False)
    rows = torch.full((512 * 2 * c.cout + 1024,), SENTINEL, dtype=torch.float32, device='cuda')
    y1, nrows = ops.conv2d_bn_partials(d.x, w, zb, c.cin, c.cout, c.ks, c.stride, rows)
    ref = CC.case_ref(c, d)
    assert float(ref.abs().max()) <= CC.F16_EXACT
    _assert_exact(y1, ref, CC.key_geometry(CC.case_key(c)))
    assert torch.equal(y0, y1)
    want = _tile_rows(ref, c)
    assert nrows == want.size(0) == _walk_stats(c)[1]
    assert int(want.abs().max()) < 2 ** 24
    got = rows[:nrows * 2 * c.cout].view(nrows, 2, c.cout)
    assert torch.equal(got.double(), want.double())
    assert bool((rows[nrows * 2 * c.cout:] == SENTINEL).all())
    yi = ref.reshape(-1, c.cout).to(torch.int64)
    assert torch.equal(got.to(torch.int64).sum(0), torch.stack([yi.sum(0), (yi * yi).sum(0)]))
    y2, st = ops.conv2d_bn_stats(d.x, w, zb, c.cin, c.cout, c.ks, c.stride, 1e-5, 0.1)
    assert torch.equal(y2, y1)
    yd = ref.reshape(-1, c.cout)
    torch.testing.assert_close(st[:c.cout].double(), yd.mean(0), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(st[c.cout:].double(), 1 / torch.sqrt(yd.var(0, unbiased=False) + 1e-5), rtol=1e-5, atol=0)
    if c.kind == 'walk':
        y3, st3 = ops.conv2d_bn_stats(d.x, w, zb, c.cin, c.cout, c.ks, c.stride, 1e-5, 0.1)
        assert torch.equal(y3, y2) and torch.equal(st3, st)


@pytest.mark.parametrize('c', CC.pro_cases(), ids=CC.case_id)
def test_conv1x1_of_an_unstored_bn_relu_activation(c):
    """the assertions of tests/test_gpu_train_convs.py::test_conv1x1_of_an_unstored_bn_relu_activation_is_bit_identical at
    174 x 5 x 65 (1044 tiles), 260 x 5 x 33 (1040) and at the map shape: conv output, batch statistics and running statistics bit-identical to
    lfd_bn_train_apply_f16 followed by the plain statistics conv; and the output inside the gate of the float64 conv of that
    activation"""
    n, h, w, cin, cout = c.n, c.h, c.w, c.cin, c.cout
    g = torch.Generator(device='cuda').manual_seed(5 + h + cout)
    yin = (torch.randn(n, h, w, cin, generator=g, device='cuda') * 1.3 + 0.2).half()
    pstats = ops.bn_train_stats(yin, 1e-5, 0.1, None, None)
    pg = torch.empty(cin, device='cuda').uniform_(0.5, 1.5, generator=g)
    pb = torch.empty(cin, device='cuda').normal_(0, 0.3, generator=g)
    wt = torch.randn(cout, cin, 1, 1, generator=g, device='cuda') * 0.15
    wp = ops.pack_conv_weight_train(wt)
    zb = torch.zeros(cout, device='cuda')
    rm_a, rv_a = torch.zeros(cout, device='cuda'), torch.ones(cout, device='cuda')
    rm_b, rv_b = torch.zeros(cout, device='cuda'), torch.ones(cout, device='cuda')
    z = ops.bn_train_apply(yin, pstats, pg, pb, None, True)
    ya, sa = ops.conv2d_bn_stats(z, wp, zb, cin, cout, 1, 1, 1e-5, 0.1, rm_a, rv_a)
    yb, sb = ops.conv1x1_of_bn_relu_bn_stats(yin, pstats, pg, pb, wp, zb, cout, 1e-5, 0.1, rm_b, rv_b)
    assert float(ya.float().abs().max()) > 0 and torch.equal(ya, yb)
    assert torch.equal(sa, sb) and torch.equal(rm_a, rm_b) and torch.equal(rv_a, rv_b)
    assert _gate_ratio(yb, CC.conv_ref(z, wt.half().float())) <= 1.0
    yc, sc = ops.conv1x1_of_bn_relu_bn_stats(yin, pstats, pg, pb, wp, zb, cout, 1e-5, 0.1)
    assert torch.equal(yc, yb) and torch.equal(sc, sb)


@pytest.mark.parametrize('c', CC.bsum_cases(), ids=CC.case_id)
def test_batchnorm_backward_sums_in_the_data_gradient_conv(c):
    """the assertions of tests/test_gpu_train_convs.py::test_batchnorm_backward_sums_in_the_data_gradient_convs_epilogue at
    174 x 5 x 65 (1044 tiles), 260 x 5 x 33 (1040) and at the map shape: dz bit for bit the plain conv, dgamma / dbeta to fp32 summation order, dy
    within an fp16 ulp"""
    n, h, w = c.n, c.h, c.w
    ch = 64
    g = torch.Generator(device='cuda').manual_seed(9 + h)
    y_u = (torch.randn(n, h, w, ch, generator=g, device='cuda') * 1.2 + 0.1).half()
    stats = ops.bn_train_stats(y_u, 1e-5, 0.1, None, None)
    gamma = torch.empty(ch, device='cuda').uniform_(0.5, 1.5, generator=g)
    beta = torch.empty(ch, device='cuda').normal_(0, 0.3, generator=g)
    dyv = (torch.randn(n, h, w, ch, generator=g, device='cuda') * 0.5).half()
    wt = torch.randn(ch, ch, 1, 1, generator=g, device='cuda') * 0.15
    wp = ops.pack_conv_weight_train(wt, data_gradient=True)
    zb = torch.zeros(ch, device='cuda')
    inv = 1.0 / 64
    dz_a = ops.conv2d_nhwc(dyv, wp, zb, ch, ch, 1, 1, False)
    dga, dba = torch.zeros(ch, device='cuda'), torch.zeros(ch, device='cuda')
    dy_a, _ = ops.bn_train_backward(dz_a, y_u, None, stats, gamma, inv, dga, dba, want_g=False, accumulate=True, relu=True, beta=beta)
    dz_b, rows = ops.conv1x1_dgrad_bn_bwd_sums(dyv, wp, zb, y_u, stats, gamma, beta)
    sums_b = ops.train_workspace(dyv.device)[:rows * 2 * ch * 4].clone()          # the rows of partial sums, fp32 [rows][2][64]
    dgb, dbb = torch.zeros(ch, device='cuda'), torch.zeros(ch, device='cuda')
    dy_b = ops.bn_train_backward_rows(dz_b, y_u, stats, gamma, beta, inv, dgb, dbb, rows)
    torch.cuda.synchronize()
    assert rows == _walk_stats(c)[1] and float(dz_a.float().abs().max()) > 0 and torch.equal(dz_a, dz_b)
    assert _gate_ratio(dz_b, CC.dgrad_ref(dyv, wt.half().float(), h, w, 1)) <= 1.0
    dz_c, rows_c = ops.conv1x1_dgrad_bn_bwd_sums(dyv, wp, zb, y_u, stats, gamma, beta)
    assert rows_c == rows and torch.equal(dz_c, dz_b) and torch.equal(ops.train_workspace(dyv.device)[:rows * 2 * ch * 4], sums_b)
    # the rows against float64: sum g and sum g * xhat over everything, g = dz * [gamma * xhat + beta > 0] on the stored fp16 dz
    xh = (y_u.double() - stats[:ch].double()) * stats[ch:].double()
    gm = dz_b.double() * ((gamma.double() * xh + beta.double()) > 0)
    want = torch.stack([gm.reshape(-1, ch).sum(0), (gm * xh).reshape(-1, ch).sum(0)])
    mag = torch.stack([gm.abs().reshape(-1, ch).sum(0), (gm * xh).abs().reshape(-1, ch).sum(0)])
    got = sums_b.view(torch.float32).view(rows, 2, ch).double().sum(0)
    # bound: xhat and the products are formed in fp32 (a few 2^-24 each) and at most a dozen fp32 additions lie between a term
    # and its row: 1e-5 of the sum of the magnitudes; an element whose pre-activation is within 1e-5 of zero may fall on either
    # side of the ReLU in fp32, so its whole term is allowed for
    near = ((gamma.double() * xh + beta.double()).abs() < 1e-5) * dz_b.double().abs()
    slack = torch.stack([near.reshape(-1, ch).sum(0), (near * xh.abs()).reshape(-1, ch).sum(0)])
    assert bool(((got - want).abs() <= 1e-5 * mag + slack).all())

    def rel(a, b):
        return float((a - b).norm() / (b.norm() + 1e-30))
    assert rel(dgb, dga) < 2e-6 and rel(dbb, dba) < 2e-6
    tol = dy_a.float().abs() * 2.0 ** -10 + 2e-6 * float(dy_a.float().abs().max()) + 1e-7
    assert bool(((dy_a.float() - dy_b.float()).abs() <= tol).all())
    assert float((dy_a != dy_b).float().mean()) < 2e-3


# ------------------------------------------------------------------------------------------------ loudness
def test_unsupported_requests_are_loud():
    z = lambda *s: torch.zeros(s, dtype=torch.float16, device='cuda')       # noqa: E731
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device='cuda')       # noqa: E731
    with pytest.raises(RuntimeError, match='unsupported'):                   # no key 64 -> 96
        ops.conv2d_nhwc(z(1, 8, 8, 64), z(3, 36, 64, 8), f(96), 64, 96, 3, 1, True)
    with pytest.raises(RuntimeError, match='unsupported'):                   # no 1x1 s2 key 128 -> 64
        ops.conv2d_nhwc(z(1, 8, 8, 128), z(2, 8, 64, 8), f(64), 128, 64, 1, 2, True)
    with pytest.raises(RuntimeError, match='unsupported'):                   # a residual on a stride-2 key
        ops.conv2d_nhwc(z(1, 8, 8, 64), z(2, 36, 64, 8), f(64), 64, 64, 3, 2, True, residual=z(1, 4, 4, 64))
    with pytest.raises(RuntimeError, match='unsupported'):                   # a residual with a chained 1x1
        ops.conv2d_nhwc(z(1, 8, 8, 64), z(2, 36, 64, 8), f(64), 64, 64, 3, 2, True, residual=z(1, 4, 4, 64), tail=(z(2, 4, 64, 8), f(64), True))
    with pytest.raises(RuntimeError, match='unsupported'):                   # no chained 1x1 behind a stride-1 conv
        ops.conv2d_nhwc(z(1, 8, 8, 64), z(2, 36, 64, 8), f(64), 64, 64, 3, 1, True, tail=(z(2, 4, 64, 8), f(64), True))
    with pytest.raises(RuntimeError, match='unsupported'):                   # no fp32-output key 32 -> 32 3x3 s1
        ops.conv2d_nhwc_f32out(z(1, 8, 8, 32), z(1, 18, 64, 8), f(32), 32, 32, 3, 1)
    # no statistics kernel for 128 -> 128 3x3 s1: the partials entry point says so (None), it does not fall back
    assert ops.conv2d_bn_partials(z(1, 8, 8, 128), z(4, 72, 64, 8), f(128), 128, 128, 3, 1, f(512 * 2 * 128)) is None
    # the downsample entry point on a stride-1 descriptor
    desc = _lib.ConvDesc(1, 8, 8, 64, 64, 3, 1, 1, 0, 0)
    x, o1, o2, w3, w1, b = z(1, 8, 8, 64), z(1, 8, 8, 64), z(1, 8, 8, 64), z(2, 36, 64, 8), z(2, 4, 64, 8), f(64)
    rc = lib().lfd_conv2d_downsample_nhwc_f16(C.byref(desc), ptr(x), ptr(o1), ptr(w3), ptr(b), ptr(w1), ptr(b), ptr(o2),
                                              ptr(ops.zero_line(x.device)), stream_ptr())
    assert rc != 0
