"""tests/golden/stem_cases.py -- seeded operands, the float64 reference, the restated launch geometry and the case tables for
the fp16 stem kernels: k_stem (csrc/stem.hip, lfd_stem_conv_f16), k_stem_fused and k_stem2x (csrc/stem_fused.hip,
lfd_stem_faster_fused_f16) and the fp16 form of k_stem_gray (csrc/stem_gray.hip, lfd_stem_gray_f16).
tests/test_stem_reference_host.py keeps the reference and the tables honest on the CPU, tests/test_gpu_stem_exact.py compares
the kernels with them.  The generators return CPU tensors; no ctypes.  conv_ref, int_tensor, walk and out_hw are those of
conv_cases.py.

The instrument: frames hold INTEGERS in [-3, 3] (fp16 NHWC, fp32 NCHW, an [N, H, W] plane for the gray kernels); a uint8 frame
holds the bytes 0 and 255 only, for which simple_normalize (v / 255 - 0.5) / 0.5 is exactly -1 and +1 (and for no other byte).
Filters and biases are integers.  Every product and every fp32 partial sum is then an integer far below 2^24, exact in any
summation order and under any rounding inside the MFMA; the biases k_stem2x feeds as fp16 hi + lo k-steps are integers of
magnitude <= 8, so hi is the bias and lo is zero.  An fp16 holds every integer of magnitude <= 2048: while every ROUNDING POINT
of the float64 reference (the pair's intermediate, the three intermediates of the four-conv chain, the output) stays inside
that, the kernel must equal the reference bit for bit.  The host test asserts that for every integer case.

The distribution (CHAIN_DIST): conv1 filter in [-1, 1], bias in [-4, 4]; conv2 (1x1) filter in [-2, 2] with a quarter non-zero,
bias in [-8, 8]; conv3 (3x3 s2) filter in [-1, 1] with 1/16 non-zero; conv4 (1x1) filter in [-1, 1] with 1/8 non-zero; the
biases of conv3 / conv4 in [-8, 8].  The kept entries of a sparse filter are non-zero, and the shares are those of 32 input
channels: with 64 they are halved (the same number of terms per output), or the fourth stage of the 64-channel chain passes
2048 (measured on the reference: 2359 - 3412 with the unhalved shares, see the host test for what the tables give now).  A kernel instance WITHOUT the chained 1x1 stores conv1's ReLU itself; with a filter in
[-1, 1] that output has at most 86 distinct values (|3 * 27 + 4|), fewer than the 100 the conditions ask for, so those
instances draw conv1 from [-8, 8] and its bias from [-64, 64] (NOTAIL_DIST: |out| <= 3 * 27 * 8 + 64 = 712).

Layouts: reference tensors are NHWC [n, h, w, c]; filters are OIHW; pad = ks // 2."""
import collections
import functools

import torch

import conv_cases as CC
from conv_cases import conv_ref, int_tensor, out_hw, walk

X_HI = 3
F16_EXACT = CC.F16_EXACT
GAUSS_GATE_PAIR = CC.GAUSS_GATE        # tests/test_gpu_conv.py::test_stem_kernel_formats, tests/test_gpu_gray.py::_run_f16
GAUSS_GATE_CHAIN = 4e-3                # tests/test_gpu_conv.py::test_whole_stem_fused_kernel
FMT_F32, FMT_F16, FMT_U8 = 0, 1, 2     # the in_format codes of the three entry points
FMT_NAMES = {FMT_F32: 'f32', FMT_F16: 'f16', FMT_U8: 'u8'}
KNOB_DEFAULTS = {'STEM2X': 1, 'X2_ALN': 1, 'X2_STAGGER': 0}       # include/lfd_hip.h

# (filter magnitude, kept share of the filter, bias magnitude) per stage
CHAIN_DIST = [(1, 1.0, 4), (2, 0.25, 8), (1, 1.0 / 16, 8), (1, 1.0 / 8, 8)]
NOTAIL_DIST = [(8, 1.0, 64)]

# kernel: 'stem' | 'gray' | 'fused' | 'stem2x'; c channels; fmt frame format; tail: the chained 1x1 (always for the fused
# kernels); aln: k_stem2x<.., ALN>
Inst = collections.namedtuple('Inst', 'kernel c fmt tail aln')

STEM_INSTANCES = [Inst('stem', c, f, t, 0) for c in (32, 64) for f in (0, 1, 2) for t in (0, 1)]        # csrc/stem.hip:233, :258
GRAY_INSTANCES = [Inst('gray', c, f, t, 0) for c in (32, 64) for f in (0, 1, 2) for t in (0, 1)]        # csrc/stem_gray.hip:266
FUSED_INSTANCES = [Inst('fused', c, f, 1, 0) for c in (32, 64) for f in (0, 1, 2)]                      # csrc/stem_fused.hip:1112, :1153
STEM2X_INSTANCES = [Inst('stem2x', 64, f, 1, a) for f in (1, 2) for a in (1, 0)]                        # csrc/stem_fused.hip:1148-1152
INSTANCES = STEM_INSTANCES + GRAY_INSTANCES + FUSED_INSTANCES + STEM2X_INSTANCES


def inst_id(i):
    if i.kernel == 'stem2x':
        return 'stem2x_%s_%s' % (FMT_NAMES[i.fmt], 'aln' if i.aln else 'gen')
    return '%s%d_%s%s' % (i.kernel, i.c, FMT_NAMES[i.fmt], '' if i.kernel == 'fused' else ('_tail' if i.tail else '_notail'))


def needs_knobs(i, route='aligned'):
    """the tuning knobs under which lfd_stem_faster_fused_f16 reaches instance i (csrc/stem_fused.hip:1142-1153): k_stem_fused<2, fp16>
    and <2, uint8> only with STEM2X = 0; the general k_stem2x on frames with 16-byte rows only with X2_ALN = 0 (route 'knob')"""
    if i.kernel == 'fused' and i.c == 64 and i.fmt != FMT_F32:
        return {'STEM2X': 0}
    if i.kernel == 'stem2x' and route == 'knob':
        return {'X2_ALN': 0}
    return {}


def stage_shapes(i):
    """-> [(cin, cout, ks, stride)] of the convs instance i chains"""
    cin = 1 if i.kernel == 'gray' else 3
    s = [(cin, i.c, 3, 2)]
    if i.kernel in ('fused', 'stem2x'):
        return s + [(i.c, i.c, 1, 1), (i.c, i.c, 3, 2), (i.c, i.c, 1, 1)]
    return s + ([(i.c, i.c, 1, 1)] if i.tail else [])


# ------------------------------------------------------------------------------------------------ seeded operands
def conv1_scale(i):
    """conv1 of the gray kernels sums 9 taps instead of 27 (its filter range is doubled), and a uint8 frame holds magnitudes of
    1 instead of up to 3 (tripled), so that conv1's spread -- and with it the number of distinct values further down -- stays
    about that of the RGB integer case"""
    return (2 if i.kernel == 'gray' else 1) * (3 if i.fmt == FMT_U8 else 1)


def int_stages(i, seed):
    """-> [(w fp32 OIHW, b fp32 [c], stride)] with integer values, drawn as the module docstring says.  A sparse filter keeps
    the stated share of its entries and those are non-zero.  The input of every conv behind the first is a ReLU output, so a
    row of non-positive weights with a non-positive bias would be a dead channel: every row of a sparse filter keeps at least
    one entry and its first kept entry is positive."""
    shapes = stage_shapes(i)
    dist = NOTAIL_DIST if len(shapes) == 1 else CHAIN_DIST
    out = []
    for k, ((cin, cout, ks, stride), (w_hi, keep, b_hi)) in enumerate(zip(shapes, dist)):
        s = int(seed) + 1000003 * (k + 1)
        if keep == 1.0:
            w = int_tensor((cout, cin, ks, ks), w_hi * (conv1_scale(i) if k == 0 else 1), s).float()
        else:
            g = torch.Generator().manual_seed(s + 17)
            mag = torch.randint(1, w_hi + 1, (cout, cin * ks * ks), generator=g).float()
            sign = (torch.randint(0, 2, mag.shape, generator=g) * 2 - 1).float()
            kept = torch.rand(mag.shape, generator=g) < keep * 32.0 / cin
            kept[~kept.any(1), 0] = True
            first = kept.float().argmax(1)
            sign[torch.arange(cout), first] = 1.0
            w = (mag * sign * kept).reshape(cout, cin, ks, ks)
        out.append((w, int_tensor((cout,), b_hi, s + 29).float(), stride))
    return out


def gauss_stages(i, seed):
    """the distributions of tests/test_gpu_conv.py (test_stem_kernel_formats, test_whole_stem_fused_kernel) and of
    tests/test_gpu_gray.py::_weights: filters rounded to fp16, biases ~ N(0, 0.1^2)"""
    g = torch.Generator().manual_seed(int(seed))
    out = []
    for k, (cin, cout, ks, stride) in enumerate(stage_shapes(i)):
        if k == 0:
            scale = 0.5 if cin == 1 else 0.2
        else:
            scale = 1.0 / (cin * ks * ks) ** 0.5
        out.append(((torch.randn(cout, cin, ks, ks, generator=g) * scale).half().float(), torch.randn(cout, generator=g) * 0.1, stride))
    return out


def to_format(i, values):
    """values: NHWC float [n, h, w, cin] holding what the kernel is to see -> the frame tensor in the format of instance i:
    fp32 NCHW / fp16 NHWC / uint8 NHWC (values must be -1 / +1), or the [n, h, w] plane of the gray kernels"""
    if i.fmt == FMT_U8:
        assert bool((values.abs() == 1).all())
        t = ((values + 1) * 127.5).to(torch.uint8)          # -1 -> 0, +1 -> 255
    elif i.fmt == FMT_F16:
        t = values.half()
    else:
        t = values.float()
    if i.kernel == 'gray':
        return t[..., 0].contiguous()
    return t.permute(0, 3, 1, 2).contiguous() if i.fmt == FMT_F32 else t.contiguous()


def int_values(i, n, h, w, seed, pm1=None):
    """-> NHWC float32 [n, h, w, cin]: integers in [-3, 3], or -1 / +1 alone for uint8 instances (or with pm1=True)"""
    cin = stage_shapes(i)[0][0]
    pm1 = (i.fmt == FMT_U8) if pm1 is None else pm1
    if pm1:
        g = torch.Generator().manual_seed(int(seed) + 7)
        return (torch.randint(0, 2, (n, h, w, cin), generator=g) * 2 - 1).float()
    return int_tensor((n, h, w, cin), X_HI, seed).float()


def gauss_values(i, n, h, w, seed):
    """uniform in [-1, 1) rounded to fp16, as the existing stem tests draw their frames"""
    cin = stage_shapes(i)[0][0]
    g = torch.Generator().manual_seed(int(seed) + 11)
    return (torch.rand(n, h, w, cin, generator=g) * 2 - 1).half().float()


# ------------------------------------------------------------------------------------------------ float64 reference
def stem_ref(x, stages, dtype=torch.float64, tap_hooks=None, skip_round=(), collect=None):
    """x: the frame as NHWC float [n, h, w, cin] (the values the kernel sees: fp16-representable); stages: [(w OIHW, b, stride)].
    Chains conv_ref + bias + ReLU and rounds to fp16 between stages (every kernel stores its intermediates as fp16).  Runs on
    the device of its operands.  -> [n, oh, ow, cout] in `dtype`, NOT rounded: the caller compares with .half().
    For the host test alone: tap_hooks {stage: tap_hook of conv_ref}, skip_round (stages whose fp16 rounding is left out) and
    collect (a list that receives every stage's value before its ReLU)."""
    y = x
    for k, (w, b, stride) in enumerate(stages):
        y = conv_ref(y, w.to(y.device), b.to(y.device), stride, dtype=dtype, tap_hook=(tap_hooks or {}).get(k))
        if collect is not None:
            collect.append(y)
        y = y.relu()
        if k + 1 < len(stages) and k not in skip_round:
            y = y.float().half().to(dtype)
    return y


# ------------------------------------------------------------------------------------------------ launch geometry
# TH x TW: the tile in output pixels; depth: stride-2 pairs between the raw frame and the map the tiles are counted on;
# max_blocks: the cap of the grid; xcd: the XCD-contiguous walk of conv_cases.walk (else workgroup b takes b, b + grid, ...)
Tile = collections.namedtuple('Tile', 'TH TW depth max_blocks xcd')
Launch = CC.Launch


def tile_geometry(i):
    nct = i.c // 32
    if i.kernel == 'stem':            # csrc/stem.hip:221 (TH = PG * 2 = 8 / NCT, TW = 32), :226 min(ntiles, 2048), :98-100 the walk
        return Tile(8 // nct, 32, 1, 2048, False)
    if i.kernel == 'gray':            # csrc/stem_gray.hip:254 (TH = 4 / NCT, TW = 64), :259 min(ntiles, 2048), :165-167 the walk
        return Tile(4 // nct, 64, 1, 2048, False)
    if i.kernel == 'fused':           # csrc/stem_fused.hip:62 FCfg (TW = 16, TH = (4 / NCT) * 2), :1091-1104 launch_fused, :126-134
        return Tile(8 // nct, 16, 2, 512, True)
    return Tile(4, 32, 2, 256, True)  # csrc/stem_fused.hip:341 X2, :1065-1078 launch_stem2x, :515-520 the walk


def out_map(i, h, w):
    """the [oh, ow] of the map instance i writes for an h x w frame"""
    for _ in range(tile_geometry(i).depth):
        h, w = out_hw(h, w, 3, 2)
    return h, w


def launch(i, n, h, w):
    g = tile_geometry(i)
    oh, ow = out_map(i, h, w)
    tx, ty = -(-ow // g.TW), -(-oh // g.TH)
    nt = n * tx * ty
    return Launch(tx, ty, nt, min(g.max_blocks, 8 * -(-nt // 8)) if g.xcd else min(nt, g.max_blocks))


def tile_walk(i, lc):
    """-> [tiles of workgroup b], in the order it takes them"""
    if tile_geometry(i).xcd:
        return walk(lc.ntiles, lc.blocks)
    return [list(range(b, lc.ntiles, lc.blocks)) for b in range(lc.blocks)]


def x2_unmasked(ty, tx, h1, w1):
    """csrc/stem_fused.hip:944: k_stem2x runs a tile without the zero-padding mask when its 9 x 65 intermediate region lies
    inside the h1 x w1 intermediate image"""
    return 8 * ty - 1 >= 0 and 8 * ty - 1 + 9 <= h1 and 64 * tx - 1 >= 0 and 64 * tx - 1 + 65 <= w1


def x2_stagger_active(lc):
    """csrc/stem_fused.hip:1082: the start-up stagger runs only from 16 tiles per workgroup"""
    return lc.ntiles >= 16 * lc.blocks


# ------------------------------------------------------------------------------------------------ case tables
# route (k_stem2x alone): how the case reaches its instance -- 'aligned' (W % 8 == 0, 16-byte base), 'misaligned' (fp16 frame at
# a base 2 bytes past a 16-byte boundary), 'knob' (X2_ALN = 0), 'width' (W % 8 != 0)
Case = collections.namedtuple('Case', 'inst kind n h w route stagger')
WALK_FRAMES = 1040                     # k_stem / k_stem_gray: x 6 tiles = 6240 tiles on 2048 workgroups
X2_A, X2_A259, X2_B, X2_C = (174, 17, 264), (174, 17, 259), (116, 35, 264), (700, 17, 264)


def in_size(o, depth, odd=True):
    """a raw extent whose extent after `depth` stride-2 pairs is o"""
    for _ in range(depth):
        o = 2 * o - 1 if odd else 2 * o
    return o


def walk_shape(i):
    """k_stem: 1040 frames with output (TH + 1) x 65 = 2 x 3 tiles (two full columns, one of a single pixel, a ragged row of one
    pixel under each): 6240 tiles on 2048 workgroups -- four tiles on the first 96 workgroups, three on the others; 2048 = 2 mod 6,
    so consecutive tiles of a workgroup lie in different images and at different places of the image.  k_stem_gray: the same with
    output (TH + 1) x 129.  k_stem_fused: 174 frames with a second-pair map of (TH + 1) x 33 = 1044 tiles on 512 workgroups, the
    walk shape of conv_cases.walk_shape.  Odd raw sizes."""
    g = tile_geometry(i)
    n = WALK_FRAMES if g.depth == 1 else CC.WALK_IMAGES
    return n, in_size(g.TH + 1, g.depth), in_size(2 * g.TW + 1, g.depth)


def walk_cases(i):
    if i.kernel != 'stem2x':
        return [Case(i, 'walk', *walk_shape(i), 'aligned', 0)]
    # (a) 174 x 17 x 264: map 5 x 66 = 2 x 3 tiles, 1044 tiles, 4 - 5 per workgroup, 32 apart (32 = 2 mod 6)
    # (b) 116 x 35 x 264: map 9 x 66 = 3 x 3 tiles, 1044 tiles; the centre tile alone runs unmasked
    # (c) 700 x 17 x 264: 4200 tiles >= 16 * 256, where X2_STAGGER = 1 takes effect
    if i.aln:
        return [Case(i, 'a', *X2_A, 'aligned', 0), Case(i, 'b', *X2_B, 'aligned', 0),
                Case(i, 'c', *X2_C, 'aligned', 0), Case(i, 'c', *X2_C, 'aligned', 1)]
    r = 'misaligned' if i.fmt == FMT_F16 else 'knob'
    return [Case(i, 'a', *X2_A, r, 0), Case(i, 'a259', *X2_A259, 'width', 0), Case(i, 'b', *X2_B, r, 0),
            Case(i, 'c', *X2_C, r, 0), Case(i, 'c', *X2_C, r, 1)]


def all_walk_cases():
    return [c for i in INSTANCES for c in walk_cases(i)]


def edge_shapes(i):
    """-> [(n, h, w)] raw frames: one pixel; 2 x 2; exactly one tile from an odd and from an even frame; one pixel past a tile
    in each direction; 3 x 3 tiles in one frame (ragged both ways); two frames of 2 x 2 tiles; the existing (1, 8, 8) and
    (1, 19, 24); for the fused kernels 3 x 5, whose whole intermediate (2 x 3) is smaller than a tile's halo region.  The aligned
    k_stem2x instances need W % 8 == 0: their widths are rounded up to it (the next wider frame the instance accepts)."""
    g = tile_geometry(i)
    d = g.depth
    s = [(1, 1, 1), (1, 2, 2), (1, in_size(g.TH, d), in_size(g.TW, d)), (1, in_size(g.TH, d, False), in_size(g.TW, d, False)),
         (1, in_size(g.TH + 1, d), in_size(g.TW, d)), (1, in_size(g.TH, d), in_size(g.TW + 1, d)),
         (1, in_size(2 * g.TH + 1, d), in_size(2 * g.TW + 1, d)), (2, in_size(g.TH + 1, d, False), in_size(g.TW + 2, d)),
         (1, 8, 8), (1, 19, 24)]
    if d == 2:
        s.append((1, 3, 5))
    if i.kernel == 'stem2x' and i.aln:
        s = [(n, h, -(-w // 8) * 8) for n, h, w in s]
    return s


def edge_cases(i):
    route = 'aligned'
    if i.kernel == 'stem2x' and not i.aln:
        route = 'misaligned' if i.fmt == FMT_F16 else 'knob'
    out = []
    for n, h, w in edge_shapes(i):          # (X2_ALN = 0 is needed only where the rows are 16-byte ones; the misaligned base stays)
        r = 'width' if (route == 'knob' and w % 8 != 0) else route
        out.append(Case(i, 'edge', n, h, w, r, 0))
    return out


def case_id(c):
    return '%s_%s_%dx%dx%d%s%s' % (inst_id(c.inst), c.kind, c.n, c.h, c.w, '' if c.route == 'aligned' else '_' + c.route,
                                   '_stagger' if c.stagger else '')


# cases whose first seed leaves an output channel that is positive nowhere (one frame of a few hundred pixels through the sparse
# filters of the chain): the seed is moved on by this much; tests/test_stem_reference_host.py asserts the conditions for every case
SEED_BUMP = {'gray64_f32_tail_edge_1x9x257': 1, 'fused32_f32_edge_1x65x129': 1, 'fused32_f16_edge_1x65x129': 1, 'fused64_f32_edge_1x33x129': 1,
             'fused64_u8_edge_1x33x129': 1, 'stem2x_f16_gen_edge_1x33x257': 1}


def case_seed(c):
    i = c.inst
    return 7919 * SEED_BUMP.get(case_id(c._replace(route='aligned', stagger=0)), 0) + sum(int(v) * p for v, p in zip((len(i.kernel), i.c, i.fmt, i.tail, i.aln, c.n, c.h, c.w), (1, 3, 7, 11, 13, 17, 19, 23)))


@functools.lru_cache(maxsize=2)
def case_int_operands(c):
    """-> (values NHWC float32 [n, h, w, cin], stages); cached: the tests that run a case more than once share them.  The two
    stagger settings and the routes of one shape share their operands (the seed does not depend on them)."""
    s = case_seed(c)
    return int_values(c.inst, c.n, c.h, c.w, s), int_stages(c.inst, s)


def case_gauss_operands(c):
    s = case_seed(c) + 1
    return gauss_values(c.inst, c.n, c.h, c.w, s), gauss_stages(c.inst, s)


def ref_in_chunks(x, stages, chunk=128, **kw):
    """stem_ref over `chunk` frames at a time (bounds the float64 temporaries of the largest cases)"""
    return torch.cat([stem_ref(x[k:k + chunk], stages, **kw) for k in range(0, x.size(0), chunk)])
