"""The hi/lo-plane kernels of the 'fp32_storage' mode at shapes where every workgroup walks a RUN of tiles, chunks or rows
(tests/golden/planes_cases.py; the walk properties of every case are asserted on the CPU by tests/test_planes_reference_host.py):
k_pl_c3p / k_pl_c3 / the k_pl_conv<...> family / k_pl_conv_ml / k_pl_head<0|1|2|3> / k_pl_head_b2 / k_pl_head_out / k_pl_stem2xs /
k_pl_stem2x / k_pl_blk64 against the float64 reference of the same chain

  * bit for bit (planes as int16 == to_planes(reference), fp32 outputs ==) on the three exact instruments -- integer operands, a
    non-zero lo plane in the activations, a non-zero lo plane in the filters; the fixed-point GroupNorm sums == round(ref * 2^24) as
    int64 on the integer instrument, where every square is an integer -- with a lo plane the sum is still exact but the kernels
    square in fp32, so the sum of squares is held to 2^-22 relative + 1 unit (heads) or the project's bounds (convs);
  * at the project's gates on Gaussian operands (4e-6 of max(1, max |y|) a conv, 2.5 x that the head chain, 1e-5 the block);

with every tensor on a plane stride LARGER than the tensor, NaN (or a sentinel) in all padding and guards, each launch run twice
for the same bits, one launch over all levels == one launch per level, and k_pl_blk64 == two k_pl_c3p launches."""
import ctypes as C
import functools

import pytest
import torch

import planes_cases as PC
from lfd_amd import _lib, engine_p2, ops
from lfd_amd._lib import check, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
GUARD, PAD = 64, 72         # halfs (floats) in front of a tensor; extra halfs per plane (a multiple of 8)
SENTINEL = -7.0
NAN = float('nan')


# ------------------------------------------------------------------------------------------------ guarded buffers
class Planes(object):
    """planes [2, N, H, W, C] fp16 on the device inside a NaN-filled buffer: GUARD halfs, then two planes PAD halfs apart"""

    def __init__(self, shape, values=None):
        self.shape, self.numel = tuple(shape), 1
        for s in shape:
            self.numel *= s
        self.plane = self.numel + PAD
        self.buf = torch.full((GUARD + 2 * self.plane + GUARD,), NAN, dtype=torch.float16, device='cuda')
        self.two = self.buf[GUARD:GUARD + 2 * self.plane].view(2, self.plane)
        if values is not None:
            self.two[:, :self.numel] = engine_p2.to_planes(values.float()).reshape(2, -1).cuda()

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + 2 * GUARD)

    def get(self):
        """the planes on the host, after checking that nothing outside them was written"""
        b = self.buf.cpu()
        two = b[GUARD:GUARD + 2 * self.plane].view(2, self.plane)
        assert bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[GUARD + 2 * self.plane:]).all()), 'guard overwritten'
        assert bool(torch.isnan(two[:, self.numel:]).all()), 'plane padding overwritten'
        out = two[:, :self.numel].reshape((2,) + self.shape).contiguous()
        assert not bool(torch.isnan(out).any()), 'unwritten output'
        return out

    def reset(self):
        self.buf.fill_(NAN)


class F32(object):
    """fp32 [rows, c] inside a NaN-guarded buffer (head modes 0 / 1 / 3 outputs, mode 1 / 2 inputs)"""

    def __init__(self, shape, values=None):
        self.shape, self.numel = tuple(shape), 1
        for s in shape:
            self.numel *= s
        self.buf = torch.full((GUARD + self.numel + GUARD,), NAN, dtype=torch.float32, device='cuda')
        if values is not None:
            self.buf[GUARD:GUARD + self.numel] = values.float().reshape(-1).cuda()

    @property
    def ptr(self):
        return self.buf.data_ptr() + 4 * GUARD

    def get(self):
        b = self.buf.cpu()
        assert bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[GUARD + self.numel:]).all()), 'guard overwritten'
        out = b[GUARD:GUARD + self.numel].reshape(self.shape)
        assert not bool(torch.isnan(out).any()), 'unwritten output'
        return out


def _bits(planes):
    return planes.contiguous().view(torch.int16)


def _assert_planes_exact(got, ref, what):
    want = engine_p2.to_planes(ref.float())
    if not torch.equal(_bits(got), _bits(want)):
        bad = (_bits(got) != _bits(want)).any(0).any(-1).nonzero()
        raise AssertionError('%s: %d pixels differ from float64, first at (image, row, column) %s' % (what, len(bad), bad[0].tolist()))


def _assert_close(got, ref, tol, what):
    err, mag = float((got.double() - ref).abs().max()), float(ref.abs().max())
    print('%s: err %.2e (max |y| %.2f)  error / gate %.2f' % (what, err, mag, err / (tol * max(1.0, mag))))
    assert err <= tol * max(1.0, mag), what


def _check_sums(sums, v):
    """tests/test_gpu_planes.py::_check_sums: the fixed-point sums of the stored values v [n, pixels, c] within its bounds"""
    n, c = v.shape[0], v.shape[-1]
    vg = v.double().reshape(n, -1, c // 8, 8)
    s, q = vg.sum((1, 3)), (vg * vg).sum((1, 3))
    sabs = float(vg.abs().sum((1, 3)).max())
    got = sums.cpu().sum(0).double() / 2.0 ** 24
    assert float((got[..., 0] - s).abs().max()) <= 2e-6 * sabs + 1e-5
    assert float((got[..., 1] - q).abs().max()) <= 2e-6 * float(q.abs().max()) + 1e-5


def _sums_agree(a, b, tiles_per_img, exact):
    """the fixed-point sums of two launches over the same values with different grids.  A workgroup keeps an image's sums in
    fp64 over its run and rounds them to a multiple of 2^-24 ONCE, when it leaves the image: at most one rounding of half a unit per
    tile of the image and launch, so two grids agree to tiles_per_img + 1 units (the fp32 steps in front are per pixel and the same
    on every grid).  On the exact instruments every partial sum is a whole number of units: the sums are then equal."""
    d = int((a - b).abs().max())
    assert d <= (0 if exact else tiles_per_img + 1), 'GroupNorm sums of the two grids differ by %d units of 2^-24' % d


def _head_sums_vs_float64(sums, ref, what):
    """lo-plane instruments through k_pl_head*: the sum is exact; the squares are formed four at a time in fp32 (three fused
    multiply-adds on a product: four roundings of 2^-24 relative), so the sum of squares is within 2^-22 of float64, plus a unit"""
    fixed, ok = PC.sums_fixed(ref)
    assert ok and torch.equal(sums[..., 0], fixed[..., 0]), what + ': fixed-point GroupNorm sum'
    d = (sums[..., 1] - fixed[..., 1]).abs().double()
    assert bool((d <= fixed[..., 1].double() * 2.0 ** -22 + 1).all()), what + ': fixed-point sum of squares off by %g units' % float(d.max())


def _new_sums(n, groups=16):
    return torch.zeros((_lib.PL_GN_REPLICAS, n, groups, 2), dtype=torch.int64, device='cuda')


def _sums_as_input(t):
    """the fixed-point sums of a float32 tensor [n, p, c] the way a producer would have left them (all in replica 0)"""
    s = torch.zeros((_lib.PL_GN_REPLICAS,) + tuple(t.shape[:1]) + (t.shape[-1] // 8, 2), dtype=torch.int64)
    s[0] = (PC.ref_sums(t) * 2.0 ** 24).round().long()
    return s.cuda()


@functools.lru_cache(maxsize=4)
def _zero():
    return ops.zero_line(torch.device('cuda'))


class _Knob(object):
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.prev = _lib.tune(self.name, self.value)

    def __exit__(self, *a):
        _lib.tune(self.name, self.prev)


# ------------------------------------------------------------------------------------------------ lfd_pl_conv2d
def _w(w):
    return engine_p2.pack_planes_weight(w).cuda()


def _b(b):
    return engine_p2._pad_bias(b, 128).cuda()


def _conv(xin, w, b, ks, stride, relu, res=None, tail=None, ds=None, gn=None, out32=None, gnin=None):
    """one lfd_pl_conv2d launch on guarded, stride-padded tensors.  Returns (out Planes | None, ds Planes | None)"""
    n, h, wd, cin = xin.shape
    cout = w.shape[0]
    oh, ow = PC.out_hw(h, wd, ks, stride)
    d = _lib.PlConvDesc()
    d.n, d.h, d.w, d.cin, d.cout, d.ks, d.stride, d.relu = n, h, wd, cin, cout, ks, stride, int(relu)
    d.in_plane_halfs = xin.plane
    keep = [_w(w), _b(b)]
    out = dsd = None
    tw = tb = dw = db = None
    f0 = f1 = sc = None
    if out32 is not None:
        d.out_mode = 2
        t0, t1, c0, c1, off, prow, scale = out32
        d.f_c0, d.f_c1, d.f_image_stride0, d.f_image_stride1 = c0, c1, prow * c0, prow * c1
        f0 = C.c_void_p(t0.data_ptr() + off * c0 * 4) if c0 else None
        f1 = C.c_void_p(t1.data_ptr() + off * c1 * 4) if c1 else None
        sc = scale
    else:
        d.out_mode = 1 if gn is not None else 0
        out = Planes((n, oh, ow, cout))
        d.out_plane_halfs = out.plane
    if res is not None:
        d.res_plane_halfs = res.plane
    if tail is not None:
        d.tail_cout, d.tail_relu = cout, int(tail[2])
        tw, tb = _w(tail[0]), _b(tail[1])
    if ds is not None:
        dw, db = _w(ds[0]), _b(ds[1])
        dsd = Planes((n, oh, ow, cout))
        d.ds_plane_halfs = dsd.plane
    gs = gg = gb = None
    if gnin is not None:
        gs, gg, gb = gnin
        d.gn_in_eps = 1e-5
    check(lib().lfd_pl_conv2d(C.byref(d), xin.ptr, out.ptr if out else None, ptr(keep[0]), ptr(keep[1]), res.ptr if res else None,
                              ptr(tw), ptr(tb), ptr(dw), ptr(db), dsd.ptr if dsd else None, ptr(gn), f0, f1, ptr(sc), ptr(gs), ptr(gg), ptr(gb),
                              ptr(_zero()), stream_ptr()), 'lfd_pl_conv2d')
    torch.cuda.synchronize()
    return out, dsd


def _compare(kind, got, ref, what, tol=PC.TOL):
    if kind in PC.EXACT:
        _assert_planes_exact(got, ref, '%s [%s]' % (what, kind))
    else:
        _assert_close(engine_p2.from_planes(got), ref, tol, '%s [gauss]' % what)


@functools.lru_cache(maxsize=8)
def _c3_ops(kind, n, h, w):
    return PC.c3_operands(kind, n, h, w)


def _c3_case(kind, knob, n, h, w):
    o = _c3_ops(kind, n, h, w)
    x, res = Planes((n, h, w, 64), o['x']), Planes((n, h, w, 64), o['res'])
    with _Knob('PL_C3', knob):
        for name, use_res, relu in PC.C3_MODES:
            out, _ = _conv(x, o['w'], o['b'], 3, 1, relu, res=res if use_res else None)
            got = out.get()
            _compare(kind, got, o['ref'][name], 'PL_C3=%d %s %dx%dx%d' % (knob, name, n, h, w))
            again, _ = _conv(x, o['w'], o['b'], 3, 1, relu, res=res if use_res else None)
            assert torch.equal(_bits(again.get()), _bits(got)), 'second launch differs'


@pytest.mark.parametrize('kind', PC.INSTRUMENTS)
@pytest.mark.parametrize('knob', PC.KNOBS['PL_C3'])
def test_c3_walk_vs_float64(knob, kind):
    """3x3 stride-1 64 -> 64 behind every value of PL_C3, plain / residual + ReLU / residual: >= 4 tiles per workgroup, full,
    ragged-right and ragged-bottom tiles inside runs, runs that cross images"""
    _c3_case(kind, knob, **PC.C3_CASE)


@pytest.mark.parametrize('kind', ['xlo', 'wlo', 'gauss'])
@pytest.mark.parametrize('knob', PC.KNOBS['PL_C3'])
def test_c3_walk_inside_one_image_vs_float64(knob, kind):
    """runs of 3-4 interior tiles of the same image (both input buffers and both exchange buffers used twice without an image change)"""
    _c3_case(kind, knob, **PC.C3_WIDE)


@pytest.mark.parametrize('knob', PC.KNOBS['PL_C3'])
def test_c3_edges_vs_float64(knob):
    for e in PC.C3_EDGES:
        for kind in ('xlo', 'wlo', 'gauss'):
            _c3_case(kind, knob, **e)


def _conv_case(kind, key, cout, n, h, w, variant):
    cin, ks, stride, _ = key
    o = PC.conv_operands(kind, key, cout, n, h, w, variant)
    x = Planes((n, h, w, cin), o['x'])
    oh, ow = PC.out_hw(h, w, ks, stride)
    what = '%s %s' % (PC.conv_case_id(key, cout, n, h, w), variant)
    if variant == 'out32':
        c0, c1 = PC.OUT32_SPLIT[cout]
        hw, off = oh * ow, 5
        prow = hw + 11                       # rows of other levels before and after this level's, in every image
        scale = torch.tensor([1.5 if kind != 'gauss' else 1.37])
        for sc in (scale.cuda(), None):
            t0 = torch.full((n, prow, c0), SENTINEL, device='cuda')
            t1 = torch.full((n, prow, c1), SENTINEL, device='cuda')
            _conv(x, o['w'], o['b'], ks, stride, False, out32=(t0, t1, c0, c1, off, prow, sc))
            first = (t0.clone(), t1.clone())
            _conv(x, o['w'], o['b'], ks, stride, False, out32=(t0, t1, c0, c1, off, prow, sc))
            assert torch.equal(t0, first[0]) and torch.equal(t1, first[1]), 'second launch differs'
            r = o['ref'].reshape(n, hw, cout)
            for t, rr, nm in ((t0.cpu(), r[..., :c0], 'cls'), (t1.cpu(), r[..., c0:c0 + c1] * (float(scale) if sc is not None else 1.0), 'reg')):
                assert bool((t[:, :off] == SENTINEL).all()) and bool((t[:, off + hw:] == SENTINEL).all()), 'rows of other levels written'
                g = t[:, off:off + hw]
                if kind in PC.EXACT:
                    assert torch.equal(g, rr.float()) and torch.equal(g.double(), rr), '%s %s [%s]' % (what, nm, kind)
                else:
                    _assert_close(g, rr, PC.TOL, '%s %s scale=%d' % (what, nm, sc is not None))
        return
    res = Planes((n, oh, ow, cout), o['res']) if variant == 'res' else None
    tail = (o['w2'], o['b2'], o['relu2']) if variant == 'tail' else None
    ds = (o['wd'], o['bd']) if variant == 'ds' else None
    runs = []
    for _ in range(2):
        gn = _new_sums(n, cout // 8) if PC.has_sums(key, variant) else None
        out, dsd = _conv(x, o['w'], o['b'], ks, stride, o['relu'], res=res, tail=tail, ds=ds, gn=gn)
        runs.append((out.get(), dsd.get() if dsd else None, gn.sum(0).cpu() if gn is not None else None))
    got, gds, sums = runs[0]
    assert torch.equal(_bits(got), _bits(runs[1][0])), 'second launch differs'
    _compare(kind, got, o['ref'], what)
    if gds is not None:
        assert torch.equal(_bits(gds), _bits(runs[1][1]))
        _compare(kind, gds, o['ref_ds'], what + ' identity branch')
    if sums is not None:
        assert torch.equal(sums, runs[1][2])
        fixed, ok = PC.sums_fixed(o['ref'].reshape(n, -1, cout))
        if kind == 'int':
            assert ok and torch.equal(sums, fixed), what + ': fixed-point GroupNorm sums'
        else:
            _check_sums(sums[None], engine_p2.from_planes(got).reshape(n, -1, cout))


_CONV_PARAMS = [pytest.param(key, cout, n, h, w, v, id='%s-%s' % (PC.conv_case_id(key, cout, n, h, w), v))
                for key, cout, n, h, w in PC.CONV_CASES for v in PC.conv_variants(key)
                if not (v == 'out32' and cout not in PC.OUT32_SPLIT) and not (v != 'out32' and cout % 32)]


@pytest.mark.parametrize('key,cout,n,h,w,variant', _CONV_PARAMS)
def test_conv_walk_vs_float64(key, cout, n, h, w, variant):
    """every key of lfd_pl_conv2d's switch with every option it is dispatched with, >= 3 tiles on some workgroup, ragged edges"""
    for kind in PC.INSTRUMENTS:
        _conv_case(kind, key, cout, n, h, w, variant)


def test_conv_edges_vs_float64():
    for key, cout, n, h, w in PC.CONV_EDGES:
        for kind in ('xlo', 'wlo', 'gauss'):
            _conv_case(kind, key, cout, n, h, w, 'plain')


@pytest.mark.parametrize('cout,n,h,w', PC.GNIN_CASES)
def test_conv_gn_in_walk_vs_float64(cout, n, h, w):
    """GroupNorm + ReLU applied by the consumer to the tile it fetched, then the 1x1: the second tower conv (planes + sums) and the
    output convs (fp32), >= 3 tiles per workgroup with an image change -- a reload of mean / rstd -- at almost every tile"""
    o = PC.gnin_operands(cout, n, h, w)
    x = Planes((n, h, w, 128), o['t'])
    gnin = (_sums_as_input(o['t'].reshape(n, h * w, 128)), o['gamma'].cuda(), o['beta'].cuda())
    what = 'gn_in 128 -> %d %dx%dx%d' % (cout, n, h, w)
    if cout == 128:
        runs = []
        for _ in range(2):
            sums = _new_sums(n)
            out, _ = _conv(x, o['w'], o['b'], 1, 1, False, gn=sums, gnin=gnin)
            runs.append((out.get(), sums.sum(0).cpu()))
        assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(runs[0][1], runs[1][1]), 'second launch differs'
        _assert_close(engine_p2.from_planes(runs[0][0]), o['ref'], PC.TOL, what)
        _check_sums(runs[0][1][None], engine_p2.from_planes(runs[0][0]).reshape(n, -1, 128))
        return
    c0, c1 = PC.OUT32_SPLIT[cout]
    hw, off = h * w, 5
    prow = hw + 11
    t0, t1 = torch.full((n, prow, c0), SENTINEL, device='cuda'), torch.full((n, prow, c1), SENTINEL, device='cuda')
    _conv(x, o['w'], o['b'], 1, 1, False, out32=(t0, t1, c0, c1, off, prow, None), gnin=gnin)
    r = o['ref'].reshape(n, hw, cout)
    for t, rr, nm in ((t0.cpu(), r[..., :c0], 'cls'), (t1.cpu(), r[..., c0:], 'reg')):
        assert bool((t[:, :off] == SENTINEL).all()) and bool((t[:, off + hw:] == SENTINEL).all()), 'rows of other levels written'
        _assert_close(t[:, off:off + hw], rr, PC.TOL_GNIN_OUT, '%s %s' % (what, nm))


# ------------------------------------------------------------------------------------------------ lfd_pl_conv2d_levels
@pytest.mark.parametrize('kind', PC.INSTRUMENTS)
def test_conv_levels_walk_vs_float64_and_one_launch_per_level(kind):
    """128 -> 128 1x1 with GroupNorm sums over five levels in one launch: contiguous runs with level changes inside"""
    n, sizes = PC.ML_CASE['n'], PC.ML_CASE['sizes']
    key = (128, 1, 1, 4)
    arr = (_lib.PlLevel * len(sizes))()
    keep = []
    for j, (h, w) in enumerate(sizes):
        o = PC.conv_operands(kind, key, 128, n, h, w, 'gn', seed=j + 1)
        x, out, sums = Planes((n, h, w, 128), o['x']), Planes((n, h, w, 128)), _new_sums(n)
        wp, bp = _w(o['w']), _b(o['b'])
        lv = arr[j]
        lv.in_, lv.out, lv.w_packed, lv.bias, lv.gn_sums = x.ptr.value, out.ptr.value, wp.data_ptr(), bp.data_ptr(), sums.data_ptr()
        lv.h, lv.w, lv.in_plane_halfs, lv.out_plane_halfs = h, w, x.plane, out.plane
        keep.append((o, x, out, sums, wp, bp))
    d = _lib.PlConvDesc()
    d.n, d.cin, d.cout, d.ks, d.stride, d.relu, d.out_mode = n, 128, 128, 1, 1, 0, 1
    first = None
    for rep in range(2):
        for k in keep:
            k[2].reset()
            k[3].zero_()
        check(lib().lfd_pl_conv2d_levels(C.byref(d), arr, len(sizes), ptr(_zero()), stream_ptr()), 'lfd_pl_conv2d_levels')
        torch.cuda.synchronize()
        got = [(k[2].get(), k[3].sum(0).cpu()) for k in keep]
        if first is None:
            first = got
        else:
            assert all(torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(a[1], b[1]) for a, b in zip(first, got)), 'second launch differs'
    for j, ((h, w), (o, x, _, _, _, _), (got, sums)) in enumerate(zip(sizes, keep, first)):
        _compare(kind, got, o['ref'], 'levels: level %d %dx%d' % (j, h, w))
        if kind == 'int':
            fixed, ok = PC.sums_fixed(o['ref'].reshape(n, -1, 128))
            assert ok and torch.equal(sums, fixed)
        else:
            _check_sums(sums[None], engine_p2.from_planes(got).reshape(n, -1, 128))
        one_sums = _new_sums(n)
        one, _ = _conv(x, o['w'], o['b'], 1, 1, False, gn=one_sums)
        assert torch.equal(_bits(one.get()), _bits(got)), 'one launch per level differs'
        _sums_agree(one_sums.sum(0).cpu(), sums, -(-h // 2) * -(-w // 32), kind in PC.EXACT)


# ------------------------------------------------------------------------------------------------ lfd_pl_head_levels
def _head_launch(mode, n, cin, levels, f=(0, 0, 0, 0), eps=1e-5):
    d = _lib.PlHeadDesc()
    d.mode, d.n, d.cin, d.relu0, d.gn_in_eps = mode, n, cin, 1, eps
    d.f_c0, d.f_c1, d.f_image_stride0, d.f_image_stride1 = f
    arr = (_lib.PlHeadLevel * len(levels))(*levels)
    check(lib().lfd_pl_head_levels(C.byref(d), arr, len(levels), ptr(_zero()), stream_ptr()), 'lfd_pl_head_levels mode %d' % mode)
    torch.cuda.synchronize()


def _pk(w):
    return engine_p2.pack_planes_weight(w.reshape(w.shape[0], w.shape[1], 1, 1)).cuda()


@functools.lru_cache(maxsize=4)
def _head_first_ops(kind, cin):
    return PC.head_first_operands(kind, cin, PC.HEAD_CASE['n'], PC.HEAD_CASE['pixels'])


@pytest.mark.parametrize('kind', PC.INSTRUMENTS)
@pytest.mark.parametrize('mode,cin', PC.HEAD_FIRST_MODES)
def test_head_first_pass_walk_vs_float64(mode, cin, kind):
    """modes 0 and 3 over five levels in one launch (runs of 4 tiles, image and level changes and ragged tiles inside runs,
    empty runs): fp32 output and fixed-point GroupNorm sums against float64; == one launch per level"""
    n, pixels = PC.HEAD_CASE['n'], PC.HEAD_CASE['pixels']
    ops_ = _head_first_ops(kind, cin)
    keep, levels = [], []
    for o, p in zip(ops_, pixels):
        x, out, sums = Planes((n, p, 1, cin), o['x'].reshape(n, p, 1, cin)), F32((n, p, 128)), _new_sums(n)
        ws = [_pk(o['w0']), _b(o['b0']), _pk(o['w1']), _b(o['b1'])]
        lv = _lib.PlHeadLevel()
        lv.in_, lv.out, lv.w0, lv.b0, lv.gn_sums = x.ptr.value, out.ptr, ws[0].data_ptr(), ws[1].data_ptr(), sums.data_ptr()
        if mode == 0:
            lv.w1, lv.b1 = ws[2].data_ptr(), ws[3].data_ptr()
        lv.in_plane_halfs, lv.pixels = x.plane, p
        keep.append((x, out, sums, ws))
        levels.append(lv)
    results = []
    for launches in ([levels], [levels], [[lv] for lv in levels]):        # one launch, again, one launch per level
        for _, out, sums, _ in keep:
            out.buf.fill_(NAN)
            sums.zero_()
        for group in launches:
            _head_launch(mode, n, cin, group)
        results.append([(out.get(), sums.sum(0).cpu()) for _, out, sums, _ in keep])
    for p, a, b, c in zip(pixels, *results):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), 'second launch differs'
        assert torch.equal(a[0], c[0]), 'one launch per level differs'
        _sums_agree(a[1], c[1], -(-p // PC.HEAD_TILE_PIXELS), kind in PC.EXACT)
    for l, (o, (got, sums)) in enumerate(zip(ops_, results[0])):
        ref = o['t1'] if mode == 0 else o['t3']
        what = 'head mode %d cin %d level %d' % (mode, cin, l)
        if kind in PC.EXACT:
            assert torch.equal(got.double(), ref), what + ' [%s]: differs from float64' % kind
            if kind == 'int':
                fixed, ok = PC.sums_fixed(ref)
                assert ok and torch.equal(sums, fixed), what + ' [int]: fixed-point GroupNorm sums'
            else:
                _head_sums_vs_float64(sums, ref, what + ' [%s]' % kind)
        else:
            _assert_close(got, ref, PC.TOL_HEAD if mode == 0 else PC.TOL, what + ' [gauss]')
            _check_sums(sums[None], got)


@functools.lru_cache(maxsize=1)
def _head_chain():
    """the Gaussian tower behind mode 0, per level: t1 (fp32, what mode 0 stores), its GroupNorm + ReLU, the second tower conv t2
    in float64 and as fp32, and the normalised t2 the output convs read"""
    n, pixels = PC.HEAD_CASE['n'], PC.HEAD_CASE['pixels']
    first, par = PC.head_first_operands('gauss', 64, n, pixels), PC.head_chain_operands(n, pixels, (1, 4))
    out = []
    for o, q in zip(first, par):
        t1 = o['t1'].float()
        t2 = PC.ref_head_tower(t1.double(), q['ga1'], q['be1'], q['w2'], q['b2'])
        t2f = t2.float()
        y2 = PC.rt(PC.ref_group_norm(t2f.double(), q['ga2'], q['be2']))
        out.append(dict(q, t1=t1, t2=t2, t2f=t2f, y2=y2))
    return out


@pytest.mark.parametrize('roles', PC.KNOBS['PL_HEAD_ROLES'])
def test_head_tower_pass_walk_vs_float64(roles):
    """mode 1 (GroupNorm + ReLU -> tower 1x1 -> fp32 + sums): k_pl_head_b2 (PL_HEAD_ROLES = 1: runs of 7 tiles on 256 workgroups, two
    tiles held ahead in registers) and k_pl_head<1> (0), all levels in one launch == one per level"""
    n, pixels = PC.HEAD_CASE['n'], PC.HEAD_CASE['pixels']
    keep, levels = [], []
    for q, p in zip(_head_chain(), pixels):
        tin, out, sin, sums = F32((n, p, 128), q['t1']), F32((n, p, 128)), _sums_as_input(q['t1']), _new_sums(n)
        ws = [_pk(q['w2']), _b(q['b2']), q['ga1'].cuda(), q['be1'].cuda()]
        lv = _lib.PlHeadLevel()
        lv.in_, lv.out, lv.w0, lv.b0, lv.gn_sums = tin.ptr, out.ptr, ws[0].data_ptr(), ws[1].data_ptr(), sums.data_ptr()
        lv.gn_in_sums, lv.gn_in_gamma, lv.gn_in_beta, lv.pixels = sin.data_ptr(), ws[2].data_ptr(), ws[3].data_ptr(), p
        keep.append((tin, out, sin, sums, ws))
        levels.append(lv)
    results = []
    with _Knob('PL_HEAD_ROLES', roles):
        for launches in ([levels], [levels], [[lv] for lv in levels]):
            for k in keep:
                k[1].buf.fill_(NAN)
                k[3].zero_()
            for group in launches:
                _head_launch(1, n, 128, group)
            results.append([(k[1].get(), k[3].sum(0).cpu()) for k in keep])
    for p, a, b, c in zip(pixels, *results):
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), 'second launch differs'
        assert torch.equal(a[0], c[0]), 'one launch per level differs'
        _sums_agree(a[1], c[1], -(-p // PC.HEAD_TILE_PIXELS), False)
    for l, (q, (got, sums)) in enumerate(zip(_head_chain(), results[0])):
        _assert_close(got, q['t2'], PC.TOL_HEAD, 'head mode 1 roles %d level %d' % (roles, l))
        _check_sums(sums[None], got)


@functools.lru_cache(maxsize=1)
def _head_out_inputs():
    n = PC.HEAD_CASE['n']
    return [(F32((n, p, 128), q['t2f']), _sums_as_input(q['t2f'])) for q, p in zip(_head_chain(), PC.HEAD_CASE['pixels'])]


@pytest.mark.parametrize('scale', [True, False])
@pytest.mark.parametrize('c0,c1', PC.HEAD_OUT_CHANNELS)
@pytest.mark.parametrize('regs', PC.KNOBS['PL_HEAD_OUT_REGS'])
def test_head_output_pass_walk_vs_float64(regs, c0, c1, scale):
    """mode 2 (GroupNorm + ReLU -> cls | reg 1x1 (+ Scale) into the level-concatenated fp32 tensors): k_pl_head_out (PL_HEAD_OUT_REGS =
    1) and k_pl_head<2> (0) at every channel split, all levels in one launch == one per level; other rows untouched"""
    n, pixels = PC.HEAD_CASE['n'], PC.HEAD_CASE['pixels']
    ptot = sum(pixels)
    prow, ct = ptot + 3, c0 + c1                 # three rows between the images that no level owns
    par = PC.head_chain_operands(n, pixels, (c0, c1))
    cls = torch.empty((n, prow, max(c0, 1)), device='cuda')
    reg = torch.empty((n, prow, max(c1, 1)), device='cuda')
    keep, levels, off = [], [], 0
    for (tin, sin), q, q3, p in zip(_head_out_inputs(), _head_chain(), par, pixels):
        ws = [_pk(q3['w3']), _b(q3['b3']), q['ga2'].cuda(), q['be2'].cuda(), q3['scale'].cuda()]
        lv = _lib.PlHeadLevel()
        lv.in_, lv.w0, lv.b0, lv.pixels = tin.ptr, ws[0].data_ptr(), ws[1].data_ptr(), p
        lv.gn_in_sums, lv.gn_in_gamma, lv.gn_in_beta = sin.data_ptr(), ws[2].data_ptr(), ws[3].data_ptr()
        if c0:
            lv.f_out0 = cls.data_ptr() + off * c0 * 4
        if c1:
            lv.f_out1 = reg.data_ptr() + off * c1 * 4
        if scale:
            lv.scale1 = ws[4].data_ptr()
        keep.append((tin, sin, ws))
        levels.append(lv)
        off += p
    results = []
    with _Knob('PL_HEAD_OUT_REGS', regs):
        for launches in ([levels], [levels], [[lv] for lv in levels]):
            cls.fill_(SENTINEL)
            reg.fill_(SENTINEL)
            for group in launches:
                _head_launch(2, n, 128, group, (c0, c1, prow * c0, prow * c1))
            results.append((cls.cpu().clone(), reg.cpu().clone()))
    assert torch.equal(results[0][0], results[1][0]) and torch.equal(results[0][1], results[1][1]), 'second launch differs'
    assert torch.equal(results[0][0], results[2][0]) and torch.equal(results[0][1], results[2][1]), 'one launch per level differs'
    gc, gr = results[0]
    if c0:
        assert bool((gc[:, ptot:] == SENTINEL).all()), 'rows between the images written'
    else:
        assert bool((gc == SENTINEL).all())
    if c1:
        assert bool((gr[:, ptot:] == SENTINEL).all()), 'rows between the images written'
    else:
        assert bool((gr == SENTINEL).all())
    off = 0
    for l, (q, q3, p) in enumerate(zip(_head_chain(), par, pixels)):
        o3 = q['y2'] @ q3['w3'].double().t() + q3['b3'].double()
        what = 'head mode 2 regs %d %d+%d scale %d level %d' % (regs, c0, c1, scale, l)
        if c0:
            _assert_close(gc[:, off:off + p], o3[..., :c0], PC.TOL_HEAD, what + ' cls')
        if c1:
            _assert_close(gr[:, off:off + p], o3[..., c0:ct] * (float(q3['scale']) if scale else 1.0), PC.TOL_HEAD, what + ' reg')
        off += p


# ------------------------------------------------------------------------------------------------ lfd_pl_stem2x
def _stem(o, n, h, w):
    g = PC.stem_geometry(n, h, w)
    out = Planes((n, g['oh'], g['ow'], 64))
    ws, bs = o['ws'], o['bs']
    keep = [engine_p2.pack_planes_stem2x_weight(ws[0], bs[0]).cuda(), engine_p2.pack_planes_stem2x_tail_weight(ws[1]).cuda(),
            engine_p2._pad_bias(bs[1]).cuda(), _w(ws[2]), _b(bs[2]), _w(ws[3]), _b(bs[3])]
    xd = o['frame'].cuda()
    check(lib().lfd_pl_stem2x(ptr(xd), o['fmt'], n, h, w, *[ptr(k) for k in keep], out.ptr, out.plane, ptr(_zero()), stream_ptr()), 'lfd_pl_stem2x')
    torch.cuda.synchronize()
    return out.get()


def _stem_case(kind, fmt, knob, n, h, w):
    o = PC.stem_operands(kind, fmt, n, h, w)
    with _Knob('PL_STEM', knob):
        got = _stem(o, n, h, w)
        assert torch.equal(_bits(_stem(o, n, h, w)), _bits(got)), 'second launch differs'
    _compare(kind, got, o['ref'], 'stem2x fmt %d PL_STEM=%d %dx%dx%d' % (fmt, knob, n, h, w))


@pytest.mark.parametrize('fmt,knob,kind', [(f, k, kind) for f, k in PC.STEM_KERNELS for kind in PC.stem_instruments(f)])
def test_stem2x_walk_vs_float64(fmt, knob, kind):
    """the row-stream kernel on all three frame formats (runs of 4-5 chunks: the ring of 10 rows wraps, runs cross strip and image
    ends, the last row pair is half empty, the last strip 4 columns wide) and the tile kernel on fp16 frames"""
    _stem_case(kind, fmt, knob, **PC.STEM_CASE)


def test_stem2x_edges_vs_float64():
    for e in PC.STEM_EDGES:
        for kind in ('xlo', 'gauss'):
            for fmt in (1, 0):
                _stem_case(kind, fmt, 1, **e)


# ------------------------------------------------------------------------------------------------ lfd_pl_block64
def _block(x, packed):
    n, h, w, _ = x.shape
    out = Planes(x.shape)
    check(lib().lfd_pl_block64(n, h, w, x.ptr, x.plane, out.ptr, out.plane, *[ptr(k) for k in packed], ptr(_zero()), stream_ptr()),
          'lfd_pl_block64')
    torch.cuda.synchronize()
    return out.get()


@pytest.mark.parametrize('kind', PC.INSTRUMENTS)
@pytest.mark.parametrize('n,h,w', PC.BLOCK_CASES)
def test_block64_walk_vs_float64_and_two_conv_launches(n, h, w, kind):
    """segments taller than twice the input ring with a ragged last one, the SH = 4 clamp, h < 4, widths 30 k + {0, 1, 29}"""
    o = PC.block_operands(kind, n, h, w)
    x = Planes((n, h, w, 64), o['x'])
    got = _block(x, [_w(o['w1']), _b(o['b1']), _w(o['w2']), _b(o['b2'])])
    assert torch.equal(_bits(_block(x, [_w(o['w1']), _b(o['b1']), _w(o['w2']), _b(o['b2'])])), _bits(got)), 'second launch differs'
    _compare(kind, got, o['ref'], 'block64 %dx%dx%d' % (n, h, w), PC.TOL_BLOCK)
    assert _lib.tune('PL_C3') == 2
    mid, _ = _conv(x, o['w1'], o['b1'], 3, 1, True)
    if kind in PC.EXACT:
        _assert_planes_exact(mid.get(), o['ref_mid'], 'block conv1 [%s]' % kind)
    two, _ = _conv(mid, o['w2'], o['b2'], 3, 1, True, res=x)
    assert torch.equal(_bits(two.get()), _bits(got)), 'k_pl_blk64 != two k_pl_c3p launches'
