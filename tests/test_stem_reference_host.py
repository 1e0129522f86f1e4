"""The float64 reference, the restated launch geometry and the case tables of tests/golden/stem_cases.py, checked without a GPU:
the conditions under which the integer cases of tests/test_gpu_stem_exact.py must be bit-exact and can see an error at all,
stem_ref against torch's double-precision F.conv2d chains, the tile walks the walk cases claim to exercise, the coverage of the
34 kernel instances by the tables, and that torch.equal -- the comparison the GPU tests make -- rejects references that are
wrong in exactly one way.

What the wrong references show (test_wrong_references_fail_the_integer_comparison): a halo column read as zero at a tile seam,
the last tile of a workgroup's run computed from the previous tile's raw patch, the image index one too low on the first tile
after an image change and (fused kernels) the intermediate outside its image equal to relu of the bias chain instead of zero
are all told from the reference on the walk case of every instance.

What the integer cases canNOT see (test_a_skipped_rounding_is_invisible_to_the_integer_cases): a skipped fp16 rounding of an
intermediate.  Every intermediate of an integer case is an integer of magnitude <= 2048, which fp16 holds exactly, so the
reference with and without the rounding is the same tensor.  That error only shows on operands whose intermediates are not
multiples of their fp16 ulp: on a small Gaussian case the two references differ in the stored fp16 output, by about one ulp
-- inside the 4e-3 gate of the Gaussian tests, which therefore do not claim to see it either.  The rounding points are held by
the existing tolerance tests against the two-kernel stem (tests/test_gpu_conv.py) only as far as an ulp goes."""
import os

import pytest
import torch
import torch.nn.functional as F

import stem_cases as S

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'lfd-a-light-and-fast-detector_amd', 'csrc')
MEASURED = {}          # kernel -> [integer cases, largest stage magnitude, smallest positive share of the population cases] (pytest -s)


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize('inst', [S.Inst('stem', 32, 1, 1, 0), S.Inst('stem', 64, 0, 0, 0), S.Inst('gray', 32, 1, 1, 0), S.Inst('gray', 64, 2, 0, 0),
                                  S.Inst('fused', 32, 1, 1, 0), S.Inst('stem2x', 64, 2, 1, 1)], ids=S.inst_id)
def test_reference_equals_double_conv2d_chain(inst):
    for k, (n, h, w) in enumerate([(1, 1, 1), (1, 2, 2), (2, 5, 7), (1, 8, 16), (2, 9, 17), (3, 12, 11), (1, 3, 5)]):
        for values, stages in ((S.int_values(inst, n, h, w, k), S.int_stages(inst, k)), (S.gauss_values(inst, n, h, w, k), S.gauss_stages(inst, k))):
            y = _nchw(values.double())
            for j, (wt, b, stride) in enumerate(stages):
                y = F.conv2d(y, wt.double(), b.double(), stride, wt.size(2) // 2).relu()
                if j + 1 < len(stages):
                    y = y.float().half().double()
            ref = S.stem_ref(values, stages)
            assert ref.dtype == torch.float64 and tuple(ref.shape) == (n,) + S.out_map(inst, h, w) + (inst.c,)
            if values is not None and bool((values == values.round()).all()):
                assert torch.equal(ref, _nhwc(y))
                assert torch.equal(S.stem_ref(values, stages, dtype=torch.float32).double(), ref)       # the dtype of the condition test
            else:                                            # equal up to the order of the float64 sums and an fp16 tie they can flip
                assert float((ref - _nhwc(y)).abs().max()) <= 2.0 ** -10 * max(1.0, float(y.abs().max()))
                assert float(((ref - _nhwc(y)).abs() > 1e-12).float().mean()) < 1e-3


def test_frame_formats_hold_the_values():
    """to_format: the three layouts of one frame, and the uint8 bytes {0, 255} whose simple_normalize is exactly -1 / +1 --
    for no other byte"""
    v = torch.arange(256, dtype=torch.float32)
    nrm = (v / 255 - 0.5) / 0.5
    assert [int(b) for b in v[(nrm == nrm.round())]] == [0, 255] and float(nrm[0]) == -1.0 and float(nrm[255]) == 1.0
    for kernel in ('stem', 'gray'):
        for fmt in (0, 1, 2):
            i = S.Inst(kernel, 32, fmt, 1, 0)
            x = S.int_values(i, 2, 5, 7, 3)
            assert float(x.abs().max()) == (1 if fmt == 2 else S.X_HI) and torch.equal(x, x.round())
            t = S.to_format(i, x)
            assert t.dtype == (torch.float32, torch.float16, torch.uint8)[fmt] and t.is_contiguous()
            back = (t.float() / 255 - 0.5) / 0.5 if fmt == 2 else t.float()
            if kernel == 'gray':
                assert tuple(t.shape) == (2, 5, 7) and torch.equal(back, x[..., 0])
            elif fmt == 0:
                assert tuple(t.shape) == (2, 3, 5, 7) and torch.equal(_nhwc(back), x)
            else:
                assert tuple(t.shape) == (2, 5, 7, 3) and torch.equal(back, x)
            if fmt == 2:
                assert set(t.unique().tolist()) == {0, 255}
    pm = S.int_values(S.Inst('stem', 32, 1, 1, 0), 2, 5, 7, 3, pm1=True)
    assert torch.equal(pm, S.int_values(S.Inst('stem', 32, 2, 1, 0), 2, 5, 7, 3))


# ------------------------------------------------------------------------------------------------ the conditions
def _conditions(c, population):
    x, stages = S.case_int_operands(c)
    assert float(x.abs().max()) <= (1 if c.inst.fmt == S.FMT_U8 else S.X_HI) and torch.equal(x, x.round())
    for w, b, _ in stages:
        assert torch.equal(w, w.round()) and torch.equal(b, b.round()) and float(b.abs().max()) <= 64
    peak = [0.0] * len(stages)
    pos = [0.0] * len(stages)
    outs = []
    for k in range(0, c.n, 128):                  # float32 is exact here: integers far below 2^24
        col = []
        outs.append(S.stem_ref(x[k:k + 128], stages, dtype=torch.float32, collect=col))
        for j, v in enumerate(col):
            assert torch.equal(v, v.round())
            peak[j] = max(peak[j], float(v.abs().max()))
            pos[j] += float((v > 0).sum())
    out = torch.cat(outs)
    numel = [0] * len(stages)
    h, w = c.h, c.w
    for j, (wt, _, stride) in enumerate(stages):
        h, w = S.out_hw(h, w, wt.size(2), stride)
        numel[j] = c.n * h * w * wt.size(0)
    share = [p / m for p, m in zip(pos, numel)]
    # 1. every rounding point (each stage's ReLU output; the last one is the stored output) is an fp16-exact integer
    assert max(peak) <= S.F16_EXACT, (S.case_id(c), peak)
    assert float(out.max()) > 0
    if population:
        # 2. ReLU hides every error of a negative value  3. every output channel is positive somewhere  4. not a handful of values
        assert min(share) >= 0.30, (S.case_id(c), share)
        assert bool((out.reshape(-1, out.size(-1)).max(0).values > 0).all()), S.case_id(c)
        assert out.unique().numel() >= 100, (S.case_id(c), out.unique().numel())
    m = MEASURED.setdefault(c.inst.kernel, [0, 0.0, 1.0])
    m[0], m[1], m[2] = m[0] + 1, max(m[1], max(peak)), min(m[2], min(share)) if population else m[2]
    assert c.n * S.out_map(c.inst, c.h, c.w)[0] * S.out_map(c.inst, c.h, c.w)[1] * c.inst.c <= 26e6        # the largest output of a case: 52 MB of fp16
    return peak, share


@pytest.mark.parametrize('c', S.all_walk_cases(), ids=S.case_id)
def test_walk_cases_satisfy_the_conditions(c):
    peak, share = _conditions(c, True)
    print('COND %s stage magnitudes %s positive shares %s' % (S.case_id(c), [int(p) for p in peak], ['%.2f' % s for s in share]))


@pytest.mark.parametrize('inst', S.INSTANCES, ids=S.inst_id)
def test_edge_cases_satisfy_the_conditions(inst):
    """every edge case stays inside the fp16-exact range.  The population conditions (30 % positive, every channel positive, 100
    distinct values) cannot hold for a case of a few pixels -- a one-pixel case has 32 or 64 output values in all -- and are
    asserted on the largest edge case of every instance, the one of 3 x 3 tiles"""
    big = 0
    for c in S.edge_cases(inst):
        population = S.launch(inst, c.n, c.h, c.w).ntiles == 9
        big += int(population)
        _conditions(c, population)
    assert big == 1


# ------------------------------------------------------------------------------------------------ geometry and walks
def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_tables_cover_every_instance_and_the_geometry_restates_the_launchers():
    assert (len(S.STEM_INSTANCES), len(S.FUSED_INSTANCES), len(S.STEM2X_INSTANCES), len(S.GRAY_INSTANCES)) == (12, 6, 4, 12)
    assert len(set(S.INSTANCES)) == 34 and len({S.inst_id(i) for i in S.INSTANCES}) == 34
    assert len({S.case_id(c) for c in S.all_walk_cases()}) == len(S.all_walk_cases())
    st, gr, fu = _src('stem.hip'), _src('stem_gray.hip'), _src('stem_fused.hip')
    # csrc/stem.hip: launch_stem and the three dispatch levels (2 NCT x 3 formats x 2 TAIL)
    assert 'constexpr int PG = 4 / NCT, TH = PG * 2, TW = 32;' in st and 'ntiles < 2048 ? (unsigned)ntiles : 2048u' in st
    assert 'for (; t < ntiles; t += gridDim.x)' in st and st.count('return launch_stem<NCT, IN_') == 3
    assert 'dispatch_fmt<2, true>' in st and 'dispatch_fmt<2, false>' in st and 'dispatch_fmt<1, true>' in st and 'dispatch_fmt<1, false>' in st
    # csrc/stem_gray.hip
    assert 'constexpr int TH = 4 / NCT, TW = 64;' in gr and 'ntiles < 2048 ? (unsigned)ntiles : 2048u' in gr
    assert 'for (; t < ntiles; t += gridDim.x)' in gr and gr.count('LFD_GRAY_CASE(') == 7          # the macro + 2 x 3 uses, each both TAILs
    # csrc/stem_fused.hip
    assert 'static constexpr int TW = 16, RPT = 2, PG = 4 / NCT, TH = PG * RPT;' in fu
    assert 'int blocks = 8 * ((a.ntiles + 7) / 8) < 512 ? 8 * ((a.ntiles + 7) / 8) : 512;' in fu
    assert 'static constexpr int TH = 4, TW = 32;' in fu
    assert 'const int blocks = 8 * ((a.ntiles + 7) / 8) < 256 ? 8 * ((a.ntiles + 7) / 8) : 256;' in fu
    assert fu.count('const int t_step = (nblk + 7 - xcd) / 8;') == 2 and fu.count('return launch_fused<NCT, IN_') == 3
    assert 'if (gy1_0 >= 0 && gy1_0 + X2::IH <= a.H1 && gx1_0 >= 0 && gx1_0 + X2::IW <= a.W1) phase_a(std::false_type{});' in fu
    assert 'const int gy1_0 = 2 * g_cur.ty0 * X2::TH - 1, gx1_0 = 2 * g_cur.tx0 * X2::TW - 1;' in fu
    assert 'a.stagger = lfd_tune(LFD_TUNE_X2_STAGGER) && a.ntiles >= 16 * blocks;' in fu
    for a, b in (('false', 'true'), ('false', 'false'), ('true', 'true'), ('true', 'false')):
        assert 'launch_stem2x<%s, %s>(a, st)' % (a, b) in fu
    G = S.tile_geometry
    assert G(S.Inst('stem', 64, 1, 1, 0)) == (4, 32, 1, 2048, False) and G(S.Inst('stem', 32, 1, 0, 0)).TH == 8
    assert G(S.Inst('gray', 64, 1, 1, 0)) == (2, 64, 1, 2048, False) and G(S.Inst('gray', 32, 1, 0, 0)).TH == 4
    assert G(S.Inst('fused', 64, 1, 1, 0)) == (4, 16, 2, 512, True) and G(S.Inst('fused', 32, 1, 1, 0)).TH == 8
    assert G(S.Inst('stem2x', 64, 1, 1, 1)) == (4, 32, 2, 256, True)
    # 8 x 1080p through k_stem2x: a 270 x 480 map -> 68 x 15 tiles per frame
    assert S.launch(S.Inst('stem2x', 64, 1, 1, 1), 8, 1080, 1920) == (15, 68, 8160, 256)
    assert S.launch(S.Inst('stem', 64, 1, 1, 0), 2, 45, 71) == (2, 6, 24, 24)          # tests/test_gpu_conv.py: one tile per workgroup
    # how lfd_stem_faster_fused_f16 reaches the instances
    assert S.needs_knobs(S.Inst('fused', 64, 1, 1, 0)) == {'STEM2X': 0} == S.needs_knobs(S.Inst('fused', 64, 2, 1, 0))
    assert S.needs_knobs(S.Inst('fused', 64, 0, 1, 0)) == {} == S.needs_knobs(S.Inst('fused', 32, 1, 1, 0))
    assert 'if (use_x2 && channels == 64 && in_format == IN_NHWC_F16)' in fu and 'if (use_x2 && channels == 64 && in_format == IN_NHWC_U8)' in fu
    for i in S.STEM2X_INSTANCES:
        for c in S.walk_cases(i) + S.edge_cases(i):
            aligned_rows = c.w % 8 == 0 and S.needs_knobs(i, c.route).get('X2_ALN', 1) == 1
            takes_aln = aligned_rows and (i.fmt == S.FMT_U8 or c.route != 'misaligned')
            assert takes_aln == bool(i.aln), S.case_id(c)


@pytest.mark.parametrize('inst', S.INSTANCES, ids=S.inst_id)
def test_walks_cover_every_tile_once(inst):
    for c in S.walk_cases(inst) + S.edge_cases(inst):
        lc = S.launch(inst, c.n, c.h, c.w)
        wk = S.tile_walk(inst, lc)
        assert len(wk) == lc.blocks and sorted(t for tiles in wk for t in tiles) == list(range(lc.ntiles))
    for ntiles in (1, 7, 9, 2047, 2048, 2049, 6240):
        lc = S.Launch(1, 1, ntiles, min(ntiles, 2048))
        wk = S.tile_walk(S.Inst('stem', 64, 1, 1, 0), lc)
        assert sorted(t for tiles in wk for t in tiles) == list(range(ntiles))


def _place(lc, t):
    per = lc.tiles_x * lc.tiles_y
    return t // per, (t % per) // lc.tiles_x, t % lc.tiles_x


@pytest.mark.parametrize('c', S.all_walk_cases(), ids=S.case_id)
def test_walk_cases_walk(c):
    """some workgroup takes at least three tiles; consecutive tiles of a workgroup lie in different images and at different
    places; a full tile is followed by a ragged one and a ragged one by a full one"""
    i = c.inst
    g = S.tile_geometry(i)
    lc = S.launch(i, c.n, c.h, c.w)
    oh, ow = S.out_map(i, c.h, c.w)
    wk = S.tile_walk(i, lc)
    per = [len(t) for t in wk]
    assert max(per) >= 3 and lc.ntiles > 2 * lc.blocks
    pairs = [(_place(lc, a), _place(lc, b)) for tiles in wk for a, b in zip(tiles, tiles[1:])]
    assert all(a[0] != b[0] and a[1:] != b[1:] for a, b in pairs)
    assert oh % g.TH != 0 and ow % g.TW != 0
    last = (lc.tiles_y - 1, lc.tiles_x - 1)
    for axis in (0, 1):
        assert any(a[1 + axis] < last[axis] and b[1 + axis] == last[axis] for a, b in pairs)
        assert any(a[1 + axis] == last[axis] and b[1 + axis] < last[axis] for a, b in pairs)
    if i.kernel in ('stem', 'gray'):
        assert (oh, ow) == (g.TH + 1, 2 * g.TW + 1) and (lc.tiles_y, lc.tiles_x, lc.ntiles, lc.blocks) == (2, 3, 6240, 2048)
        assert per == [4] * 96 + [3] * 1952 and c.h % 2 == 1 and c.w % 2 == 1
    elif i.kernel == 'fused':
        assert (oh, ow) == (g.TH + 1, 2 * g.TW + 1) and (lc.tiles_y, lc.tiles_x, lc.ntiles, lc.blocks) == (2, 3, 1044, 512)
        assert 2 in per and 3 in per
    else:
        assert lc.blocks == 256 and (lc.ntiles == 1044 and {4, 5} <= set(per) <= {3, 4, 5} or lc.ntiles == 4200)
        h1, w1 = S.out_hw(c.h, c.w, 3, 2)
        free = {(ty, tx) for ty in range(lc.tiles_y) for tx in range(lc.tiles_x) if S.x2_unmasked(ty, tx, h1, w1)}
        if c.kind == 'b':
            # 3 x 3 tiles of which the centre one alone runs unmasked: every workgroup that meets it comes from a masked tile
            # and goes on to a masked tile (or ends there, which the walk below also finds)
            assert (lc.tiles_y, lc.tiles_x) == (3, 3) and free == {(1, 1)}
            before = [a[1:] for a, b in pairs if b[1:] == (1, 1)]
            after = [b[1:] for a, b in pairs if a[1:] == (1, 1)]
            assert len(before) >= 50 and len(after) >= 50 and (1, 1) not in before and (1, 1) not in after
            assert any(tiles and _place(lc, tiles[0])[1:] == (1, 1) for tiles in wk) and any(tiles and _place(lc, tiles[-1])[1:] == (1, 1) for tiles in wk)
        else:
            assert (lc.tiles_y, lc.tiles_x) == (2, 3) and free == set()
        assert S.x2_stagger_active(lc) == (c.kind == 'c')
        if c.kind == 'c':
            assert lc.ntiles >= 4096 and min(per) >= 16
    assert S.x2_unmasked(1, 1, 540, 960) and not S.x2_unmasked(0, 1, 540, 960) and not S.x2_unmasked(67, 1, 540, 960) and S.x2_unmasked(66, 1, 540, 960)


def test_edge_tables():
    for i in S.INSTANCES:
        g = S.tile_geometry(i)
        shapes = S.edge_shapes(i)
        maps = [(n,) + S.out_map(i, h, w) for n, h, w in shapes]
        tiles = [S.launch(i, n, h, w).ntiles for n, h, w in shapes]
        assert (1, g.TH, g.TW) in maps and tiles.count(9) == 1 and tiles.count(1) >= 4
        assert (1, g.TH + 1, g.TW) in maps
        if i.kernel == 'stem2x' and i.aln:          # the narrowest frame has 8 columns; the next width past a tile is two map columns more
            assert all(w % 8 == 0 for _, _, w in shapes) and (1, g.TH, g.TW + 2) in maps and (1, 1, 8) in shapes and (1, 2, 8) in shapes
        else:
            assert (1, g.TH, g.TW + 1) in maps and (1, 1, 1) in shapes and (1, 2, 2) in shapes and (1, 1, 1) in maps
            assert any(h % 2 == 1 and w % 2 == 1 and S.launch(i, n, h, w).ntiles == 1 and (h, w) != (1, 1) for n, h, w in shapes)
        assert any(h % 2 == 0 and w % 2 == 0 and S.out_map(i, h, w) == (g.TH, g.TW) for n, h, w in shapes)
        assert ((1, 8, 8) in shapes and (1, 19, 24) in shapes)
        if g.depth == 2:          # the whole intermediate (2 x 3) smaller than the halo region of one tile
            assert any((h, w) == (3, 5 if not i.aln else 8) for _, h, w in shapes)
            assert S.out_hw(3, 5, 3, 2) == (2, 3)


# ------------------------------------------------------------------------------------------------ wrong references
def _region(lc, g, oh, ow, t):
    _, ty, tx = _place(lc, t)
    return slice(ty * g.TH, min(ty * g.TH + g.TH, oh)), slice(tx * g.TW, min(tx * g.TW + g.TW, ow))


def _padded_with(c, x, stages, chain_value):
    """the four-conv chain with the intermediate's padding equal to v instead of zero: conv3 over (mid - v) zero-padded, plus
    conv3 of the constant v (linear in its input).  chain_value=False: v = 0, which must give the reference back."""
    mid = S.stem_ref(x, stages[:2]).float().half().double()
    (w1, b1, _), (w2, b2, _), (w3, b3, s3), (w4, b4, _) = stages
    v = (w2.double()[:, :, 0, 0] @ b1.double().relu() + b2.double()).relu().float().half().double() if chain_value else torch.zeros(c.inst.c, dtype=torch.float64)
    y = S.conv_ref(mid - v, w3, None, s3) + w3.double().sum((2, 3)) @ v + b3.double()
    y = y.relu().float().half().double()
    return S.conv_ref(y, w4, b4, 1, relu=True)


@pytest.mark.parametrize('inst', S.INSTANCES, ids=S.inst_id)
def test_wrong_references_fail_the_integer_comparison(inst):
    c = S.walk_cases(inst)[0]
    g = S.tile_geometry(inst)
    lc = S.launch(inst, c.n, c.h, c.w)
    oh, ow = S.out_map(inst, c.h, c.w)
    wk = S.tile_walk(inst, lc)
    x, stages = S.case_int_operands(c)
    conv3x3 = 2 if g.depth == 2 else 0          # the last 3x3 of the chain: its halo is the one a tile seam cuts

    def ref_of(images, **kw):
        return S.stem_ref(x[images], stages, **kw).float().half()

    # 1. the halo column at the seam between tile 0 and tile 1 of image 0 read as zero
    def seam(ky, kx, t):
        if kx == 0:
            t = t.clone()
            t[0, :g.TH, g.TW] = 0
        return t
    good = ref_of([0])
    assert not torch.equal(ref_of([0], tap_hooks={conv3x3: seam}), good), 'seam'
    assert torch.equal(ref_of([0], tap_hooks={conv3x3: lambda ky, kx, t: t}), good)

    # 2. the last tile of a workgroup's run computed from the raw patch of the tile before it: the frame zero-extended to whole
    #    tiles gives what the kernel computes for EVERY lane of a tile (for the fused kernels with the previous tile's padding too)
    run = [tiles for tiles in wk if len(tiles) >= 3][0]
    tp, tl = run[-2], run[-1]
    (np_, typ, txp), (nl, tyl, txl) = _place(lc, tp), _place(lc, tl)
    scale = 2 ** g.depth
    ext = torch.zeros((1, lc.tiles_y * g.TH * scale, lc.tiles_x * g.TW * scale, x.size(3)))
    ext[0, :c.h, :c.w] = x[np_]
    ext_out = S.stem_ref(ext, stages).float().half()
    assert tuple(ext_out.shape[1:3]) == (lc.tiles_y * g.TH, lc.tiles_x * g.TW)
    good = ref_of([nl])
    wrong = good.clone()
    ry, rx = _region(lc, g, oh, ow, tl)
    wrong[0, ry, rx] = ext_out[0, typ * g.TH:typ * g.TH + (ry.stop - ry.start), txp * g.TW:txp * g.TW + (rx.stop - rx.start)]
    assert not torch.equal(wrong, good), 'stale prefetch'

    # 3. the image index one too low on the first tile a workgroup takes in a new image
    t1 = run[1]
    n1 = _place(lc, t1)[0]
    assert n1 >= 1 and n1 != _place(lc, run[0])[0]
    both = ref_of([n1 - 1, n1])
    wrong = both[1:].clone()
    ry, rx = _region(lc, g, oh, ow, t1)
    wrong[0, ry, rx] = both[0, ry, rx]
    assert not torch.equal(wrong, both[1:]), 'image index'

    # 4. (fused kernels) the intermediate outside its H1 x W1 image = relu of the bias chain instead of zero
    if g.depth == 2:
        good = S.stem_ref(x[:2], stages)
        assert torch.equal(_padded_with(c, x[:2], stages, False), good)
        bad = _padded_with(c, x[:2], stages, True)
        assert not torch.equal(bad.float().half(), good.float().half()), 'bias-chain padding'
        assert torch.equal(bad[:, 1:-1, 1:-1], good[:, 1:-1, 1:-1])          # and the interior of the map does not depend on the padding


@pytest.mark.parametrize('inst', [i for i in S.INSTANCES if len(S.stage_shapes(i)) > 1], ids=S.inst_id)
def test_a_skipped_rounding_is_invisible_to_the_integer_cases(inst):
    """see the module docstring: on the integer operands the reference without any intermediate rounding is the reference; on a
    small Gaussian case some intermediate is not a multiple of its fp16 ulp and the stored outputs differ"""
    c = S.walk_cases(inst)[0]
    x, stages = S.case_int_operands(c)
    every = tuple(range(len(stages)))
    assert torch.equal(S.stem_ref(x[:8], stages, skip_round=every), S.stem_ref(x[:8], stages))
    small = c._replace(n=2, h=33, w=57)
    xg, sg = S.case_gauss_operands(small)
    ref = S.stem_ref(xg, sg)
    mid = S.stem_ref(xg, sg[:1])
    assert bool((mid.float().half().double() != mid).any())
    gate = S.GAUSS_GATE_PAIR if len(stages) == 2 else S.GAUSS_GATE_CHAIN
    for k in range(len(stages) - 1):
        bad = S.stem_ref(xg, sg, skip_round=(k,))
        assert not torch.equal(bad.float().half(), ref.float().half()), k
        ratio = float(((bad - ref).abs() / (gate * ref.abs().clamp(min=1.0))).max())
        print('skipped rounding of intermediate %d of %s: %.2f of the Gaussian gate' % (k + 1, S.inst_id(inst), ratio))


def test_zz_measured_conditions():
    """prints what the condition tests measured per kernel (pytest -s); run after them by its name"""
    for kernel, (cases, peak, share) in sorted(MEASURED.items()):
        print('measured %s: %d integer cases, largest stage magnitude %d, smallest positive share %.2f' % (kernel, cases, peak, share))
