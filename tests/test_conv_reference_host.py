"""The float64 reference, the restated launch geometry and the case tables of tests/golden/conv_cases.py, checked without a
GPU: conv_ref / dgrad_ref against torch's double-precision F.conv2d / conv_transpose2d / autograd, the condition under which
the integer cases of tests/test_gpu_conv_exact.py must be bit-exact, the tile walk every walk case claims to exercise, the
tiles every map case claims to contain, the coverage of every key of the four switch statements by the tables, and that the
comparisons the GPU tests make do fail for a reference that is wrong in one tap, one pixel or one halo.

What the wrong references show (test_wrong_references_fail_the_integer_comparison / .._and_the_gaussian_gate): the integer
comparison fails for all five on every case they can affect.  The Gaussian gate 1.2e-3 * max(|ref|, 1) catches all five as
well on these operands -- a dropped tap moves an output by about 0.17, a hundred gates -- so for defects of that size the two
instruments agree.  None is left uncaught by the Gaussian gate; what only the integer instrument is sure to see is a defect
that can fall BELOW the gate, which the last test pins down: one product x[c] * w[o, c] dropped from the outputs of one pixel
passes the Gaussian gate wherever x[c] happens to be small (at 2 of the 64 places probed) and is a whole unit in the integer
comparison wherever the product is not zero."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import conv_cases as CC

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'lfd-a-light-and-fast-detector_amd', 'csrc')


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _conv2d(o, stride, relu=False, res=False, tail=None, bias=True):
    y = F.conv2d(_nchw(o.x.double()), o.w.double(), o.b.double() if bias else None, stride, o.w.size(2) // 2)
    if res:
        y = y + _nchw(o.res.double())
    if relu:
        y = y.relu()
    if tail is not None:
        y = F.conv2d(y.float().half().double(), o.w2.double(), o.b2.double())
        if tail:
            y = y.relu()
    return _nhwc(y)


SMALL = [(1, 1, 1), (1, 2, 2), (2, 5, 7), (1, 8, 16), (2, 9, 17), (3, 12, 11)]
CHANNELS = [(16, 32), (32, 32), (64, 32), (32, 64), (48, 96)]


@pytest.mark.parametrize('ks,stride', [(3, 1), (3, 2), (1, 1), (1, 2)])
def test_reference_equals_double_conv2d(ks, stride):
    for i, (n, h, w) in enumerate(SMALL):
        cin, cout = CHANNELS[i % len(CHANNELS)]
        o = CC.int_operands(n, h, w, cin, cout, ks, stride, seed=i, tail=True)
        assert float(o.x.abs().max()) <= CC.X_HI and torch.equal(o.x, o.x.round()) and float(o.w.abs().max()) <= CC.W_HI_TAIL
        assert 0.1 < float((o.w2 != 0).float().mean()) < 0.4 or cout * cout < 2000
        ref = CC.conv_ref(o.x, o.w, o.b, stride)
        assert ref.dtype == torch.float64 and tuple(ref.shape) == (n,) + CC.out_hw(h, w, ks, stride) + (cout,)
        assert torch.equal(ref, _conv2d(o, stride))
        assert torch.equal(CC.conv_ref(o.x, o.w, None, stride), _conv2d(o, stride, bias=False))
        assert torch.equal(CC.conv_ref(o.x, o.w, o.b, stride, relu=True), _conv2d(o, stride, relu=True))
        assert torch.equal(CC.conv_ref(o.x, o.w, o.b, stride, residual=o.res, relu=True), _conv2d(o, stride, relu=True, res=True))
        assert torch.equal(CC.conv_ref(o.x, o.w, o.b, stride, residual=o.res), _conv2d(o, stride, res=True))
        for r1, r2 in ((True, True), (False, False)):
            assert torch.equal(CC.conv_ref(o.x, o.w, o.b, stride, relu=r1, tail=(o.w2, o.b2, r2)), _conv2d(o, stride, relu=r1, tail=r2))
        main, ident = CC.conv_ref(o.x, o.w, o.b, stride, relu=True, ds=(o.wd, o.bd))
        assert torch.equal(main, _conv2d(o, stride, relu=True))
        assert torch.equal(ident, _nhwc(F.conv2d(_nchw(o.x.double()), o.wd.double(), o.bd.double(), stride)))
        assert torch.equal(CC.conv_ref(o.x, o.w, o.b, stride, dtype=torch.float32).double(), ref)       # the cap check's dtype
        # Gaussian operands: equal up to the order of the float64 sums
        g = CC.gauss_operands(n, h, w, cin, cout, ks, stride, seed=i, tail=True)
        a, b = CC.conv_ref(g.x, g.w, g.b, stride, residual=g.res, relu=True), _conv2d(g, stride, relu=True, res=True)
        assert float((a - b).abs().max()) <= 1e-13 * max(1.0, float(b.abs().max()))


def test_reference_prologue_is_batchnorm_and_relu():
    g = torch.Generator().manual_seed(3)
    y = (torch.randn(2, 9, 17, 64, generator=g) * 1.3 + 0.2).half()
    yd = y.double().reshape(-1, 64)
    stats = torch.cat([yd.mean(0), 1 / torch.sqrt(yd.var(0, unbiased=False) + 1e-5)]).float()
    gamma, beta = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.3
    z = CC.pro_apply(y, stats, gamma, beta)
    zr = F.relu(F.batch_norm(_nchw(y.double()), None, None, gamma.double(), beta.double(), True, 0.0, 1e-5))
    assert z.dtype == torch.float16 and float((_nchw(z.double()) - zr).abs().max()) <= 2.0 ** -10 * float(zr.max())   # an fp16 ulp
    w = CC.int_tensor((64, 64, 1, 1), 2, 5).float()
    assert torch.equal(CC.conv_ref(y, w, pro=(stats, gamma, beta)), CC.conv_ref(z, w))


@pytest.mark.parametrize('ks,stride', [(3, 1), (3, 2), (1, 1), (1, 2)])
def test_data_gradient_reference_equals_conv_transpose_and_autograd(ks, stride):
    for i, (n, h, w) in enumerate(SMALL + [(2, 6, 8)]):
        cin, cout = CHANNELS[i % len(CHANNELS)]
        oh, ow = CC.out_hw(h, w, ks, stride)
        wt = CC.int_tensor((cout, cin, ks, ks), 2, i).float()
        dy = CC.int_tensor((n, oh, ow, cout), 3, i + 50).half()
        res = CC.int_tensor((n, h, w, cin), 64, i + 90).half()
        pad = ks // 2
        opad = (h + 2 * pad - ks - (oh - 1) * stride, w + 2 * pad - ks - (ow - 1) * stride)
        ct = _nhwc(F.conv_transpose2d(_nchw(dy.double()), wt.double(), None, stride, pad, output_padding=opad if stride == 2 else 0))
        ref = CC.dgrad_ref(dy, wt, h, w, stride)
        assert tuple(ref.shape) == (n, h, w, cin) and torch.equal(ref, ct)
        assert torch.equal(CC.dgrad_ref(dy, wt, h, w, stride, residual=res), ct + res.double())
        x = torch.zeros((n, cin, h, w), dtype=torch.float64, requires_grad=True)
        F.conv2d(x, wt.double(), None, stride, pad).backward(_nchw(dy.double()))
        assert torch.equal(ref, _nhwc(x.grad))
        # the data-gradient FORM the kernels run: the stride-1 conv of the zero-inserted dy with the roles swapped, taps flipped
        dz = torch.zeros((n, h, w, cout), dtype=torch.float16)
        dz[:, ::stride, ::stride] = dy
        assert torch.equal(CC.conv_ref(dz, wt.flip(2, 3).transpose(0, 1), None, 1, residual=res), ct + res.double())


# ------------------------------------------------------------------------------------------------ the exactness condition
def _all_int_cases():
    return CC.conv_cases() + CC.ds_cases() + CC.acc32_cases() + CC.stats_cases()


def _stored_values(c, o):
    """every tensor an exact run stores (float32 is exact here: see exact_cap)"""
    out = CC.case_ref(c, o, dtype=torch.float32)
    out = list(out) if isinstance(out, tuple) else [out]
    if c.variant == 'tail':
        out.append(CC.conv_ref(o.x, o.w, o.b, c.stride, relu=bool(c.relu), dtype=torch.float32))
    return out


@pytest.mark.parametrize('c', _all_int_cases(), ids=CC.case_id)
def test_integer_cases_satisfy_the_exactness_condition(c):
    o = CC.case_int_operands(c)
    assert float(o.x.abs().max()) == CC.X_HI and float(o.w.abs().max()) == (CC.W_HI_TAIL if c.tail else CC.W_HI)
    cap = CC.exact_cap(c)
    assert cap == (2 ** 24 - 1 if c.variant == 'acc32' else 2048)
    for t in _stored_values(c, o):
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= cap, (CC.case_id(c), float(t.abs().max()))
        assert float(t.abs().max()) >= 30          # and the case is not degenerate
    oh, ow = CC.out_hw(c.h, c.w, c.ks, c.stride)
    assert c.n * max(c.h * c.w * c.cin, oh * ow * c.cout) < 1.4e7          # the largest tensor of a case: 28 MB of fp16


def test_edge_dgrad_and_splitk_cases_satisfy_the_exactness_condition():
    for key, shapes in CC.edge_cases():
        cin, ks, stride, cout, tail = key
        for n, h, w in shapes:
            c = CC.Case(*key, 'tail' if tail else 'plain', 'edge', n, h, w, 0, 0)
            for t in _stored_values(c, CC.case_int_operands(c)):
                assert float(t.abs().max()) <= 2048
    for key in CC.DGRAD_KEYS:          # residual as the collected gradient, no bias
        for fwd_stride in (1, 2):
            c = CC.Case(*key, 'res', 'map', *CC.map_shape(key), 0, 0)
            o = CC.case_int_operands(c)
            # (the packed filter's values are a permutation of o.w's: the bound is the one of the stride-1 conv on dense dy,
            #  and the zero-inserted dy of a stride-2 forward conv only removes terms)
            t = CC.conv_ref(o.x, o.w, None, 1, residual=o.res, dtype=torch.float32)
            assert float(t.abs().max()) <= 2048
    for n, h, w in [CC.DGRAD_S2_WALK] + CC.DGRAD_S2_EDGES:
        oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
        dy = CC.int_tensor((n, oh, ow, 64), CC.X_HI, h * 100 + w).half()
        wt = CC.int_tensor((64, 64, 3, 3), CC.W_HI, 7).float()
        res = CC.int_tensor((n, h, w, 64), CC.RES_HI, 9).half()
        assert float(CC.dgrad_ref(dy, wt, h, w, 2, residual=res, dtype=torch.float32).abs().max()) <= 2048
    for n, h, w in CC.SPLITK_SHAPES:
        c = CC.Case(*CC.SPLITK_KEY, 'res', 'map', n, h, w, 1, 0)
        assert float(CC.case_ref(c, CC.case_int_operands(c), dtype=torch.float32).abs().max()) <= 2048
    assert [CC.takes_splitk(n, h, w) for n, h, w in CC.SPLITK_SHAPES] == [True, True, True, True, False]
    assert CC.SPLITK_SHAPES[3][0] * CC.SPLITK_SHAPES[3][1] * CC.SPLITK_SHAPES[3][2] == CC.SPLITK_MAX_PIXELS


# ------------------------------------------------------------------------------------------------ geometry, walk and maps
def test_geometry_restates_the_kernel_configuration():
    """spot values read off Cfg<> in csrc/conv_impl.h (its own comments: 8 x 16 tile of the 3x3 s1 64-channel workhorse, 4 x 32
    of the other stride-1 64-output kernels; stride-2 single buffer except the 64-channel 3x3 without tail)"""
    G = CC.conv_geometry
    assert G(64, 3, 1, 2, False) == (16, 2, 2, 2, 8, 2)
    assert G(64, 1, 1, 2, False) == (32, 1, 2, 2, 4, 2)
    assert G(128, 3, 1, 4, False) == (32, 1, 2, 1, 2, 2)
    assert G(64, 3, 2, 2, False) == (16, 2, 1, 2, 4, 2) and G(64, 3, 2, 2, True).NBUF == 1 and G(64, 3, 2, 4, False).NBUF == 1
    assert G(32, 3, 2, 1, True) == (16, 2, 1, 4, 8, 1) and G(64, 3, 1, 1, False).TH == 16
    assert {CC.key_geometry(k).NBUF for k in CC.DISPATCH_KEYS} == {1, 2}
    # the walk: every tile exactly once, whatever the counts
    for ntiles in (1, 7, 8, 9, 17, 511, 512, 513, 1040, 1044, 4097):
        blocks = max(1, min(512, 8 * -(-ntiles // 8)))
        wk = CC.walk(ntiles, blocks)
        assert sorted(t for tiles in wk for t in tiles) == list(range(ntiles)) and len(wk) == blocks
    assert [len(t) for t in CC.walk(9, 16)] == [1, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 0]       # XCD 4 one tile, 5 - 7 none
    assert CC.conv_launch(2, 135, 240, CC.conv_geometry(64, 3, 1, 2, False)) == (15, 17, 510, 512)
    assert CC.dgrad_launch(4, 159, 161) == (6, 10, 240, 240)


def _walk_cases():
    return [c for c in _all_int_cases() + CC.pro_cases() + CC.bsum_cases() if c.kind == 'walk']


def _check_walk(lc):
    wk = CC.walk(lc.ntiles, lc.blocks)
    per = [len(t) for t in wk]
    assert lc.ntiles > 1024 and lc.blocks == 512
    assert max(per) >= 3 and 2 in per, 'both buffers reused on some workgroup, exactly two tiles on another'
    per_xcd = -(-lc.ntiles // 8)
    assert lc.ntiles - 7 * per_xcd != per_xcd, 'unequal XCD ranges'
    # consecutive tiles of a workgroup: another image, another tile row AND another tile column (full <-> ragged both ways)
    per_img = lc.tiles_x * lc.tiles_y
    place = lambda t: ((t % per_img) // lc.tiles_x, t % lc.tiles_x)       # noqa: E731
    steps = {(place(a), place(b)) for tiles in wk for a, b in zip(tiles, tiles[1:])}
    assert all(a // per_img != b // per_img for tiles in wk for a, b in zip(tiles, tiles[1:]))
    last = (lc.tiles_y - 1, lc.tiles_x - 1)
    for axis in (0, 1):          # a full tile row / column followed by the ragged one, and the ragged one by a full one
        assert any(a[axis] < last[axis] and b[axis] == last[axis] for a, b in steps)
        assert any(a[axis] == last[axis] and b[axis] < last[axis] for a, b in steps)
    assert any(a[0] < last[0] and a[1] < last[1] and b == last for a, b in steps), 'a full tile followed by the corner tile'
    return max(per)


@pytest.mark.parametrize('c', _walk_cases(), ids=CC.case_id)
def test_walk_cases_walk(c):
    geo = CC.key_geometry(CC.case_key(c))
    oh, ow = CC.out_hw(c.h, c.w, c.ks, c.stride)
    assert (oh, ow) == (geo.TH + 1, 2 * geo.TW + 1)
    assert c.stride == 1 or (c.h % 2 == 1 and c.w % 2 == 1)
    _check_walk(CC.conv_launch(c.n, oh, ow, geo))


def test_dgrad_s2_walk_case_walks():
    n, h, w = CC.DGRAD_S2_WALK
    lc = CC.dgrad_launch(n, h, w)
    assert lc.tiles_x == 3 and lc.tiles_y == 2
    _check_walk(lc)
    assert sorted(CC.dgrad_launch(*s).ntiles for s in CC.DGRAD_S2_EDGES) == [1, 1, 1, 1, 2, 2, 9, 12]


@pytest.mark.parametrize('c', [c for c in _all_int_cases() + CC.pro_cases() + CC.bsum_cases() if c.kind == 'map'], ids=CC.case_id)
def test_map_cases_have_interior_ragged_and_corner_tiles(c):
    geo = CC.key_geometry(CC.case_key(c))
    oh, ow = CC.out_hw(c.h, c.w, c.ks, c.stride)
    lc = CC.conv_launch(c.n, oh, ow, geo)
    assert lc.tiles_x >= 3 and lc.tiles_y >= 3, 'an interior tile: neighbours on every side, its whole halo inside the image'
    assert ow % geo.TW != 0 and oh % geo.TH != 0, 'ragged right tiles, ragged bottom tiles and the corner tile that is both'
    assert c.n >= 2 and lc.ntiles <= lc.blocks


def test_edge_table():
    for key, shapes in CC.edge_cases():
        geo = CC.key_geometry(key)
        s = key[2]
        outs = [(n,) + CC.out_hw(h, w, key[1], s) for n, h, w in shapes]
        for want in [(1, 1, 1), (1, geo.TH, geo.TW), (1, geo.TH, geo.TW + 1), (1, geo.TH + 1, geo.TW)]:
            assert want in outs
        assert 9 in [CC.conv_launch(n, oh, ow, geo).ntiles for n, oh, ow in outs]
        if s == 2:
            assert any(h % 2 == 1 and w % 2 == 1 for _, h, w in shapes) and any(h % 2 == 0 and w % 2 == 0 for _, h, w in shapes)
            assert any(h % 2 == 0 and w % 2 == 1 for _, h, w in shapes)


# ------------------------------------------------------------------------------------------------ coverage of the switch statements
def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_tables_cover_every_key_of_the_four_switch_statements():
    """the lists of conv_cases.py side by side with the kernels' own switch statements, read from the sources"""
    # csrc/conv.hip:63 conv_dispatch
    d = re.findall(r'launch_conv<(\d+), (\d), (\d), (\d), (?:true|false), (true|false)>\(a, st\)', _src('conv.hip'))
    keys = [(int(a), int(b), int(c), 32 * int(e), int(t == 'true')) for a, b, c, e, t in d]
    assert len(keys) == len(set(keys)) == 25 and _src('conv.hip').count('launch_conv<') == 25
    assert sorted(keys) == sorted(CC.DISPATCH_KEYS)
    assert sorted({CC.case_key(c) for c in CC.conv_cases()}) == sorted(keys)
    assert sorted(k for k, _ in CC.edge_cases()) == sorted(keys)
    for k in keys:
        got = {(c.variant, c.kind) for c in CC.conv_cases() if CC.case_key(c) == k}
        want = {'tail'} if k[4] else ({'plain', 'res'} if k[2] == 1 else {'plain'})
        assert got == {(v, kind) for v in want for kind in ('walk', 'map')}
    # the fused downsample branch exists for the 3x3 s2 keys without tail; DS_KEYS are those the backbones launch
    assert set(CC.DS_KEYS) <= {k for k in keys if k[1] == 3 and k[2] == 2 and not k[4]}
    assert sorted({CC.case_key(c) for c in CC.ds_cases()}) == sorted(CC.DS_KEYS)
    assert sorted(CC.DGRAD_KEYS) == sorted(k for k in keys if k[2] == 1 and not k[4])
    assert CC.SPLITK_KEY in keys
    # csrc/conv_stats.hip:54 conv_bn_stats, :18 the prologue, :126 the backward sums
    st = _src('conv_stats.hip')
    s = re.findall(r'launch_stats<(\d+), (\d), (\d), (\d), true>\(a', st)
    skeys = [(int(a), int(b), int(c), 32 * int(e), 0) for a, b, c, e in s]
    assert len(skeys) == 8 and sorted(skeys) == sorted(CC.STATS_KEYS) == sorted({CC.case_key(c) for c in CC.stats_cases()})
    assert 'if constexpr (KS == 1 && S == 1 && CIN == 64)' in st
    assert sorted(CC.PRO_KEYS) == sorted(k for k in skeys if k[:3] == (64, 1, 1)) == sorted({CC.case_key(c) for c in CC.pro_cases()})
    assert st.count('launch_conv_<') == 3 and 'launch_conv_<64, 1, 1, 2, true, false, false, false, false, false, false, true>' in st
    assert CC.BSUM_KEYS == [(64, 1, 1, 64, 0)] == sorted({CC.case_key(c) for c in CC.bsum_cases()})
    # csrc/conv_acc32.hip:28
    a = re.findall(r'ACC32_CASE\((\d+), (\d), (\d), (\d), (?:true|false)\);', _src('conv_acc32.hip'))
    akeys = [(int(p), int(q), int(r), 32 * int(e), 0) for p, q, r, e in a]
    assert len(akeys) == len(set(akeys)) == 19 and sorted(akeys) == sorted(CC.ACC32_KEYS) == sorted({CC.case_key(c) for c in CC.acc32_cases()})
    assert set(akeys) <= set(keys)
    # csrc/dgrad_s2.hip and csrc/conv_small.hip: the constants restated
    dg = _src('dgrad_s2.hip')
    assert 'static constexpr int TH = 8, TW = 16;' in dg and 'int blocks = 512;' in dg and (CC.DGRAD_TH, CC.DGRAD_TW) == (8, 16)
    assert '(long)a.N * a.OH * a.OW <= 16384' in _src('conv.hip') and CC.SPLITK_MAX_PIXELS == 16384


# ------------------------------------------------------------------------------------------------ wrong references
def _mutants(c):
    """name -> (tap_hook, filter) for the deliberately wrong references that can affect case c"""
    geo = CC.key_geometry(CC.case_key(c))
    oh, ow = CC.out_hw(c.h, c.w, c.ks, c.stride)

    def drop_bottom(ky, kx, t):          # one tap dropped on the bottom row
        if (ky, kx) == (0, 0):
            t = t.clone()
            t[:, oh - 1] = 0
        return t

    def drop_right(ky, kx, t):           # one tap dropped on the right column
        if (ky, kx) == (0, 0):
            t = t.clone()
            t[:, :, ow - 1] = 0
        return t

    def prev_image(ky, kx, t):           # one pixel taken from the previous image
        t = t.clone()
        t[1, 0, 0] = t[0, 0, 0]
        return t

    def stale_halo(ky, kx, t):           # the left halo column of tile 1 taken from tile 0, whose left halo is the zero padding
        if kx == 0:
            t = t.clone()
            t[0, :geo.TH, geo.TW] = 0
        return t

    out = {'drop_bottom': (drop_bottom, False), 'drop_right': (drop_right, False), 'prev_image': (prev_image, False)}
    if c.ks == 3:
        out['transpose_taps'] = (None, True)
        out['stale_halo'] = (stale_halo, False)
    return out


def _two_images(o):
    return o._replace(x=o.x[:2], res=o.res[:2])


def _mutant_ref(c, o, hook, transpose, dtype):
    w = o.w.transpose(2, 3) if transpose else o.w
    return CC.conv_ref(o.x, w, o.b, c.stride, residual=o.res if c.variant == 'res' else None, relu=bool(c.relu),
                       tail=(o.w2, o.b2, bool(c.relu2)) if c.tail else None, dtype=dtype, tap_hook=hook)


@pytest.mark.parametrize('c', CC.conv_cases(), ids=CC.case_id)
def test_wrong_references_fail_the_integer_comparison(c):
    """on the first two images of the case (the wrong references differ from the right one there alone): torch.equal, the
    comparison of tests/test_gpu_conv_exact.py, tells each of them from the reference"""
    o = _two_images(CC.case_int_operands(c))
    ref = _mutant_ref(c, o, None, False, torch.float32)
    assert torch.equal(ref, CC.case_ref(c._replace(n=2), o, dtype=torch.float32))
    for name, (hook, tr) in _mutants(c).items():
        assert not torch.equal(_mutant_ref(c, o, hook, tr, torch.float32), ref), name


def _gate_ok(got, ref):
    return bool(((got - ref).abs() <= CC.GAUSS_GATE * ref.abs().clamp(min=1.0)).all())


@pytest.mark.parametrize('c', [c for c in CC.conv_cases(('map',))], ids=CC.case_id)
def test_wrong_references_and_the_gaussian_gate(c):
    """the gate of tests/test_gpu_conv.py on its Gaussian operands: catches the first four wrong references (as the integer
    comparison does) and, measured here, the stale halo as well -- three dropped taps of a column are no smaller than one"""
    o = CC.case_gauss_operands(c)
    ref = _mutant_ref(c, o, None, False, torch.float64)
    assert _gate_ok(ref.float().half().double(), ref), 'the gate passes a correctly rounded result'
    for name, (hook, tr) in _mutants(c).items():
        assert not _gate_ok(_mutant_ref(c, o, hook, tr, torch.float64), ref), name


def test_a_single_wrong_product_passes_the_gaussian_gate_and_fails_the_integer_comparison():
    """the defect below the gate: ONE product x[c] * w[o, c] of every output of one pixel dropped.  On Gaussian operands
    (|x * w| ~ 0.5 * 1 / 24 = 0.02 typically, but the gate is absolute 1.2e-3 only below |ref| = 1 and the product is that small
    whenever x[c] is) some outputs stay inside the gate -- a kernel with this defect at a pixel whose x[c] happens to be small
    passes; on integer operands every non-zero product is at least 1 and torch.equal fails whenever x[c] * w[o, c] != 0."""
    c = [k for k in CC.conv_cases(('map',)) if CC.case_key(k) == (64, 3, 1, 64, 0) and k.variant == 'plain'][0]
    passed_gate = caught_int = 0
    og, oi = CC.case_gauss_operands(c), CC.case_int_operands(c)
    refg, refi = CC.case_ref(c, og), CC.case_ref(c, oi)
    for px in range(16):
        for ch in range(4):
            # drop the centre tap's product of input channel ch at output pixel (0, 3, px)
            dg = og.x[0, 3, px, ch].double() * og.w[:, ch, 1, 1].double()
            di = oi.x[0, 3, px, ch].double() * oi.w[:, ch, 1, 1].double()
            wrong_g, wrong_i = refg.clone(), refi.clone()
            wrong_g[0, 3, px] -= dg
            wrong_i[0, 3, px] -= di
            passed_gate += int(_gate_ok(wrong_g, refg))
            if bool((di != 0).any()):
                caught_int += int(not torch.equal(wrong_i, refi))
            else:
                caught_int += 1
    assert caught_int == 64
    assert passed_gate >= 1         # (2 of 64 with these seeds)
    print('single dropped product: %d of 64 pass the Gaussian gate, 0 of 64 pass the integer comparison' % passed_gate)
