"""Seeded operands, a float64 reference, the restated tile walks and the case tables of the hi/lo-plane kernels
('fp32_storage' mode: csrc/planes*.hip, lfd_amd/engine_p2.py), shared by tests/test_planes_reference_host.py (CPU: the reference is
pinned to torch, the walk properties and the exactness caps of every case are asserted) and tests/test_gpu_planes_walk.py (the
kernels against this reference at shapes where every workgroup walks a RUN of tiles).  CPU only; imports no compiled code.

The exact instruments.  A plane value is hi + lo / 2048 with hi, lo fp16 (engine_p2.to_planes); the kernels accumulate
main = sum w_hi x_hi and corr = sum (w_hi x_lo + w_lo x_hi) in fp32 and store main + corr / 2048 (w_lo x_lo is dropped by design).
With operands on a dyadic grid whose partial sums all fit 24 bits every one of those steps is exact IN ANY ORDER, so the kernel
must reproduce the float64 result bit for bit:
  'int'  integer activations in [-3, 3], integer filters in [-2, 2], integer bias           (lo planes all zero)
  'xlo'  activations a + b / 4096 (a in [-3, 3], b in [-8, 8]: most lo planes non-zero), integer filters: exercises w_hi x_lo
  'wlo'  integer activations, filters w + k / 8192 (k in [-8, 8]: most lo planes non-zero): exercises w_lo x_hi
'gauss' draws what tests/test_gpu_planes.py::_inputs draws and is compared at the project's relative gates.
"""
import torch
import torch.nn.functional as F

LO = 2048.0
EXACT = ('int', 'xlo', 'wlo')
INSTRUMENTS = EXACT + ('gauss',)

TOL = 4e-6            # single conv: relative to max(1, max |y|) (tests/test_gpu_planes.py)
TOL_HEAD = 2.5 * TOL  # head chain
TOL_BLOCK = 1e-5      # residual block


# ------------------------------------------------------------------------------------------------ planes (engine_p2.to_planes)
def to_planes(x):
    x = x.float()
    hi = x.half()
    return torch.stack([hi, ((x - hi.float()) * LO).half()], 0).contiguous()


def from_planes(p):
    return p[0].float() + p[1].float() / LO


def rt(t):
    """round trip through planes: the value a kernel hands on when it stores t as planes (float64 in, float64 out)"""
    return from_planes(to_planes(t.float())).double()


def survives_planes(t):
    return bool(torch.equal(rt(t), t.double()))


# ------------------------------------------------------------------------------------------------ seeded operands
def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def activations(kind, shape, seed, amp=3):
    g = _gen(seed)
    if kind == 'gauss':
        return from_planes(to_planes(torch.randn(*shape, generator=g) * 2))          # the value the planes hold
    a = torch.randint(-amp, amp + 1, shape, generator=g).float()
    if kind == 'xlo':
        a = a + torch.randint(-8, 9, shape, generator=g).float() / 4096
    return a


def filters(kind, cout, cin, ks, seed, nnz=48, amp=2, den=8192):
    """[cout, cin, ks, ks]; exact kinds: about `nnz` non-zero taps per output channel (spread over all of K) with integer values in
    [-amp, amp] -- a cap on sum |w| and so on every partial sum; gauss: N(0, 1 / K)"""
    g = _gen(seed)
    k = cin * ks * ks
    if kind == 'gauss':
        return torch.randn(cout, cin, ks, ks, generator=g) * (1.0 / k ** 0.5)
    w = torch.randint(-amp, amp + 1, (cout, cin, ks, ks), generator=g).float()
    keep = torch.rand(cout, cin, ks, ks, generator=g) < min(1.0, float(nnz) / k)
    w = w * keep
    if kind == 'wlo':
        w = w + keep * torch.randint(-8, 9, (cout, cin, ks, ks), generator=g).float() / den
    return w


def bias(kind, c, seed):
    g = _gen(seed)
    if kind == 'gauss':
        return torch.randn(c, generator=g)
    return torch.randint(-3, 4, (c,), generator=g).float()


def later(kind):
    """the instrument of the filters BEHIND the first conv of a chain: 'wlo' puts its lo plane into the first filter only (the
    intermediate then lies on the 2^-13 grid, and a second non-integer filter would leave the grid)"""
    return 'int' if kind == 'wlo' else kind


def weight_survives_split(w):
    hi = w.half()
    lo = ((w - hi.float()) * LO).half()
    return bool(torch.equal(hi.float() + lo.float() / LO, w.float()))


def lo_fraction(t):
    return float((to_planes(t)[1] != 0).float().mean())


# ------------------------------------------------------------------------------------------------ float64 reference
def ref_conv(x, w, b, ks, stride, relu, res=None):
    """x [N,H,W,C] -> [N,OH,OW,cout] in float64 (padding ks // 2)"""
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), stride=stride, padding=ks // 2).permute(0, 2, 3, 1)
    if res is not None:
        y = y + res.double()
    return (y.relu() if relu else y).contiguous()


def ref_chained(x, w, b, ks, stride, w2, b2, relu2):
    """conv + ReLU -> planes -> 1x1 (+ ReLU): returns (mid, out)"""
    mid = ref_conv(x, w, b, ks, stride, True)
    return mid, ref_conv(rt(mid), w2, b2, 1, 1, relu2)


def ref_block(x, w1, b1, w2, b2):
    mid = ref_conv(x, w1, b1, 3, 1, True)
    return mid, ref_conv(rt(mid), w2, b2, 3, 1, True, res=x)


def ref_stem(xr, ws, bs):
    """the 'faster' stem on the frame values xr [N,H,W,3]: 3x3 s2 -> 1x1 -> 3x3 s2 -> 1x1, ReLU after each, planes in between;
    returns every stage (the last is the output)"""
    out, y = [], xr
    for (w, b), (ks, s) in zip(zip(ws, bs), ((3, 2), (1, 1), (3, 2), (1, 1))):
        y = ref_conv(rt(y), w, b, ks, s, True)
        out.append(y)
    return out


def ref_group_norm(t, gamma, beta, eps=1e-5):
    """t [N,P,C] float64, groups of 8 channels, + ReLU"""
    return F.group_norm(t.permute(0, 2, 1), t.shape[2] // 8, gamma.double(), beta.double(), eps).permute(0, 2, 1).relu()


def ref_sums(t):
    """per (image, group of 8 channels): sum and sum of squares of t [N,P,C] -> [N, C/8, 2] float64"""
    v = t.double().reshape(t.shape[0], -1, t.shape[-1] // 8, 8)
    return torch.stack([v.sum((1, 3)), (v * v).sum((1, 3))], -1)


def sums_fixed(t):
    """the fixed-point GroupNorm sums (units of 2^-24) as int64, and whether they are exact integers below 2^24 * 2^24"""
    s = ref_sums(t) * 2.0 ** 24
    r = s.round()
    ok = bool(torch.equal(r, s)) and float(ref_sums(t).abs().max()) < 2.0 ** 24
    return r.long(), ok


def ref_head_first(x, w0, b0, w1, b1):
    """mode 0: x [N,P,cin] -> neck 1x1 + ReLU -> planes -> tower 1x1 (no ReLU): (mid, t1)"""
    mid = (x.double() @ w0.double().t() + b0.double()).relu()
    return mid, rt(mid) @ w1.double().t() + b1.double()


def ref_head_tower(t, gamma, beta, w, b):
    """modes 1 / 2: GroupNorm + ReLU -> planes -> 1x1"""
    return rt(ref_group_norm(t, gamma, beta)) @ w.double().t() + b.double()


# ------------------------------------------------------------------------------------------------ restated walks
# lfd_pl_conv2d's switch (csrc/planes.hip): key (cin, ks, stride, ceil(cout / 32)) -> (NCT, WREG, PTO) of launch_pl<...>; the
# 128-channel 3x3 has two instances, chosen by the number of output pixels
CONV_INSTANCES = {
    (64, 3, 1, 2): (2, True, 0), (64, 3, 2, 2): (2, True, 0), (64, 3, 2, 4): (2, True, 0), (64, 1, 1, 4): (4, True, 0),
    (128, 3, 1, 4): {'small': (2, False, 1), 'large': (4, False, 1)}, (128, 3, 2, 4): (4, False, 0), (128, 1, 1, 4): (4, True, 0),
    (128, 1, 1, 1): (1, True, 1), (128, 1, 1, 2): (2, True, 0), (32, 3, 2, 1): (1, True, 0), (32, 3, 2, 2): (2, True, 0),
}
C128_SMALL_MAX_PIXELS = 16384
# engine_p2._DISPATCH
DISPATCH = {
    (64, 3, 1, 2): {'res'}, (64, 3, 2, 2): {'tail', 'ds'}, (64, 3, 2, 4): {'ds'}, (64, 1, 1, 4): {'tail', 'gn', 'out32'},
    (128, 3, 1, 4): {'res'}, (128, 3, 2, 4): {'ds'}, (128, 1, 1, 4): {'tail', 'gn', 'out32'}, (128, 1, 1, 1): {'out32'},
    (128, 1, 1, 2): {'out32'}, (32, 3, 2, 1): {'tail', 'ds'}, (32, 3, 2, 2): {'tail', 'ds'},
}
C3_TILE = (16, 4)          # C3 / C3P: TW, TH (csrc/planes_c3.hip, planes_c3p.hip)
C3_BLOCKS = 256
HEAD_TILE_PIXELS = 64
HEAD_BLOCKS = {'head': 512, 'out': 512, 'b2': 256}       # launch_pl_head<...>, launch_pl_head_out, launch_pl_head_b2
STEM_BLOCKS, STEM_TW, STEM_RING = 256, 16, 10            # launch_stem2xs, SS::TW, SS::RR
BLK_TW, BLK_NIN, BLK_NMID = 30, 8, 4                     # PB::TW, PB::NIN, PB::NMID


def pcfg_tile(cin, ks, stride, nct, pto):
    """PCfg<...>::TW, TH (csrc/planes_impl.h)"""
    pt = pto if pto else (2 if stride == 1 else 1)
    tw = 32 if (stride == 1 and not (cin == 64 and ks == 3)) else 16
    return tw, (4 // nct) * pt * (32 // tw)


def pl_heavy(cin, ks, nct, wreg, tail, ds):
    """PlHeavy<...>::value: one workgroup per CU.  When it is false the launch still takes one per CU if the LDS image is
    larger than 80 KB -- not restated: such cases assert their properties for both grid sizes (conv_blocks)."""
    wregs = ((ks * ks * cin // 16) * 8 if wreg else 96) + (nct * 2 * 8 if tail else 0) + ((cin // 16) * 8 if ds else 0)
    return (not wreg) or wregs > 96


def out_hw(h, w, ks, stride):
    p = ks // 2
    return (h + 2 * p - ks) // stride + 1, (w + 2 * p - ks) // stride + 1


def conv_instance(key, npix_out):
    inst = CONV_INSTANCES[key]
    if isinstance(inst, dict):
        inst = inst['small' if npix_out <= C128_SMALL_MAX_PIXELS else 'large']
    return inst


def conv_blocks(key, cout, opts, ntiles, npix_out):
    """the grid sizes launch_pl_ may take for this case: [blocks] or, where per_cu is not restated, both candidates"""
    nct, wreg, _ = conv_instance(key, npix_out)
    tail, ds = 'tail' in opts, 'ds' in opts
    cgroups = 1 if tail else -(-cout // (nct * 32))
    per_cus = [1] if pl_heavy(key[0], key[1], nct, wreg, tail, ds) else [1, 2]
    return sorted({max(1, min(256 * pc // cgroups, 8 * (-(-ntiles // 8)))) for pc in per_cus})


def walk_strided(ntiles, blocks):
    """launch_pl_ / k_pl_c3 / k_pl_c3p: eight XCD ranges of ceil(nt / 8) tiles; workgroup b (XCD b & 7, index b >> 3) takes tiles
    x_begin + (b >> 3) + i * wgs_xcd.  Returns the run of every workgroup."""
    per = -(-ntiles // 8)
    runs = []
    for b in range(blocks):
        xcd, bix = b & 7, b >> 3
        x0, x1 = xcd * per, min(xcd * per + per, ntiles)
        step = (blocks + 7 - xcd) // 8
        runs.append(list(range(x0 + bix, x1, step)) if step > 0 else [])
    return runs


def walk_contiguous(ntiles, blocks):
    """k_pl_conv_ml / k_pl_head* : contiguous chunks of ceil(range / wgs_xcd) tiles inside each XCD range"""
    per = -(-ntiles // 8)
    runs = []
    for b in range(blocks):
        xcd, bix = b & 7, b >> 3
        x0, x1 = xcd * per, min(xcd * per + per, ntiles)
        wgs = (blocks + 7 - xcd) // 8
        chunk = -(-(x1 - x0) // wgs) if wgs > 0 and x1 > x0 else 0
        t0 = x0 + bix * chunk
        runs.append(list(range(t0, min(t0 + chunk, x1))) if chunk > 0 else [])
    return runs


def grid_blocks(cap, ntiles):
    return max(1, min(cap, 8 * (-(-ntiles // 8))))


def image_tiles(n, oh, ow, tw, th):
    """tile index -> (image, ty, tx, ragged right, ragged bottom, interior) for one map"""
    tx_, ty_ = -(-ow // tw), -(-oh // th)
    out = []
    for i in range(n):
        for ty in range(ty_):
            for tx in range(tx_):
                rr, rb = (tx + 1) * tw > ow, (ty + 1) * th > oh
                out.append((i, ty, tx, rr, rb, 0 < ty < ty_ - 1 and 0 < tx < tx_ - 1))
    return out


def level_tiles(n, levels_tiles_per_img):
    """tile index -> (level, image, index in the image) for a launch over several levels (tile_start per level)"""
    out = []
    for l, tpi in enumerate(levels_tiles_per_img):
        out += [(l, i, j) for i in range(n) for j in range(tpi)]
    return out


def covered_once(runs, ntiles):
    seen = sorted(t for r in runs for t in r)
    return seen == list(range(ntiles))


def stem_geometry(n, h, w):
    """lfd_pl_stem2x: frame h x w -> mid ((h+1)//2, (w+1)//2) -> out; chunks = row pairs of 16-column strips"""
    mh, mw = (h + 1) // 2, (w + 1) // 2
    oh, ow = (mh + 1) // 2, (mw + 1) // 2
    tiles_x, cy = -(-ow // STEM_TW), (oh + 1) // 2
    return dict(oh=oh, ow=ow, tiles_x=tiles_x, cy=cy, total=n * tiles_x * cy)


def stem_runs(n, h, w):
    """launch_stem2xs: workgroup b takes chunks [b total / g, (b + 1) total / g); chunk u -> (image, strip, row pair) as struct Walk"""
    g_ = stem_geometry(n, h, w)
    total, per_img, cy = g_['total'], g_['tiles_x'] * g_['cy'], g_['cy']
    blocks = min(STEM_BLOCKS, total)
    runs = []
    for b in range(blocks):
        u0, u1 = b * total // blocks, (b + 1) * total // blocks
        runs.append([(u // per_img, (u % per_img) // cy, (u % per_img) % cy) for u in range(u0, u1)])
    return runs


def stem_ring_rows(run, cy):
    """ring row (of STEM_RING) of each chunk's first row along a run -- walk_next: +5 at a strip change, +4 otherwise"""
    rc, out = 0, []
    for _, _, c in run:
        out.append(rc)
        rc += 5 if c + 1 == cy else 4
    return out


def block_geometry(n, h, w):
    """lfd_pl_block64: strips of PB::TW columns; segments of SH rows, one (strip, segment) per workgroup"""
    strips = -(-w // BLK_TW)
    cols = n * strips
    segs = max(1, 256 // cols)
    sh = min(h, max(4, -(-h // segs)))
    segs = -(-h // sh)
    return dict(strips=strips, SH=sh, segs=segs, nwork=cols * segs, last=h - (segs - 1) * sh, clamped=-(-h // max(1, 256 // cols)) < 4)


# ------------------------------------------------------------------------------------------------ case tables
# 3x3 stride-1 64 -> 64 behind PL_C3 = 2 (k_pl_c3p), 1 (k_pl_c3), 0 (k_pl_conv): plain, residual + ReLU, residual without ReLU.
# 86 images of 17 x 33: a 3 x 3 grid of 8-row tiles (PL_C3 = 0: 774 tiles, 4 on some of its 256 workgroups) or 5 x 3 of 4-row
# tiles (1290 tiles, up to 6 per workgroup); a full interior tile, the ragged right column (33 = 2 * 16 + 1) and the ragged
# bottom row (17 = 2 * 8 + 1 = 4 * 4 + 1) all come up in the middle of runs, and the stride of 32 tiles crosses images every step
C3_CASE = dict(n=86, h=17, w=33)
# the same kernels where a run DWELLS in an image: 4 images of 50 x 250 (13 x 16 tiles of 4 x 16 each, 832 tiles): an XCD range is
# half an image, so the 3-4 tiles of a k_pl_c3p / k_pl_c3 run are interior tiles of one image, two tile rows apart
C3_WIDE = dict(n=4, h=50, w=250)
C3_MODES = (('plain', False, True), ('res_relu', True, True), ('res', True, False))      # name, residual, relu
C3_EDGES = [dict(n=1, h=1, w=1), dict(n=1, h=1, w=40), dict(n=70, h=2, w=2), dict(n=2, h=5, w=3)]

# every other key of lfd_pl_conv2d's switch: (key, cout, variant) -> n, h, w of the INPUT.  Each is about the smallest map with
# a 3 x 3 grid of tiles (an interior tile, a ragged right column, a ragged bottom row) repeated over enough images that some
# workgroup gets >= 3 tiles at the largest grid the launch may take.
CONV_CASES = [
    # key, cout, n, h, w
    ((64, 3, 2, 2), 64, 114, 18, 66),      # out 9 x 33, tiles 4 x 16
    ((64, 3, 2, 4), 128, 58, 18, 66),      # two cout groups: 256 workgroups
    ((64, 1, 1, 4), 128, 114, 5, 65),      # tiles 2 x 32
    ((128, 3, 1, 4), 128, 50, 5, 65),      # 16250 pixels: the <= 16384-pixel instance (two cout groups of 64), tiles 2 x 32
    ((128, 3, 1, 4), 128, 18, 19, 65),     # 22230 pixels: the large instance, tiles 1 x 32
    ((128, 3, 2, 4), 128, 114, 10, 66),    # out 5 x 33, tiles 2 x 16
    ((128, 1, 1, 4), 128, 114, 5, 65),
    ((128, 1, 1, 1), 5, 114, 9, 65),       # tiles 4 x 32; cls | reg 1 + 4
    ((128, 1, 1, 2), 50, 114, 9, 65),      # 46 + 4
    ((32, 3, 2, 1), 32, 114, 34, 66),      # out 17 x 33, tiles 8 x 16
    ((32, 3, 2, 2), 64, 114, 18, 66),
]
CONV_EDGES = [((128, 1, 1, 4), 128, 1, 1, 1), ((128, 1, 1, 4), 128, 70, 1, 3), ((64, 3, 2, 2), 64, 1, 1, 1), ((128, 3, 1, 4), 128, 1, 1, 37)]
OUT32_SPLIT = {5: (1, 4), 50: (46, 4), 128: (124, 4)}    # cout -> (f_c0, f_c1) of the fp32 outputs


def conv_variants(key):
    return ['plain'] + sorted(DISPATCH[key])


def has_sums(key, variant):
    """GroupNorm sums ride on the plain 1x1 ('gn') and on the chained neck -> tower pair ('tail' of a 1x1)"""
    return variant == 'gn' or (variant == 'tail' and key[1] == 1)


def conv_case_id(key, cout, n, h, w):
    return 'c%dk%ds%d_%d_%dx%dx%d' % (key[0], key[1], key[2], cout, n, h, w)


# GroupNorm + ReLU applied by the CONSUMER to the tile it fetched (gn_in of lfd_pl_conv2d, Gaussian operands only): the second
# tower conv (sums out) and the cls / reg output convs at the walk shapes of their keys: cout -> n, h, w
GNIN_CASES = [(128, 114, 5, 65), (5, 114, 9, 65), (50, 114, 9, 65)]
TOL_GNIN_OUT = 8e-6       # fp32 outputs behind a consumer-side GroupNorm (tests/test_gpu_planes.py)

# every value of the tuning knobs that select a kernel, and the modes of lfd_pl_head_levels
KNOBS = {'PL_C3': (2, 1, 0), 'PL_HEAD_ROLES': (1, 0), 'PL_HEAD_OUT_REGS': (1, 0), 'PL_STEM': (1, 0)}
HEAD_FIRST_MODES = [(0, 64), (0, 128), (3, 128)]          # (mode, cin) of the passes that read planes; modes 1 and 2 read fp32

# lfd_pl_conv2d_levels (k_pl_conv_ml, 128 -> 128 1x1 with GroupNorm sums): tiles 2 x 32, contiguous runs
ML_CASE = dict(n=18, sizes=[(37, 65), (19, 33), (9, 17), (5, 9), (3, 5)])

# lfd_pl_head_levels: one launch over five levels of 95 images; 64-pixel tiles (11, 3, 1, 1, 1 per image -- every level ends on a
# ragged tile), 1615 tiles: contiguous runs of 4 on 512 workgroups (7 on the 256 of k_pl_head_b2), the last workgroups of
# every XCD with an empty run; runs in levels 2-4 change image at every tile; 95 keeps the level starts off the run starts
HEAD_CASE = dict(n=95, pixels=[21 * 31, 11 * 16, 6 * 8, 3 * 4, 2 * 2])
HEAD_OUT_CHANNELS = [(1, 4), (28, 4), (29, 4), (46, 4), (60, 4), (5, 0), (0, 4)]       # f_c0 + f_c1 in {5, 32, 33, 50, 64}; cls-only; reg-only

# lfd_pl_stem2x: 3 frames of 106 x 1552 -> out 27 x 388: 25 strips (388 = 24 * 16 + 4) of 14 row pairs (27 odd: the last pair is
# half empty), 1050 chunks on 256 workgroups: runs of 4-5 chunks -- the ring of 10 rows wraps in every run, runs cross strip
# ends and the two image ends
STEM_CASE = dict(n=3, h=106, w=1552)
STEM_KERNELS = [(1, 1), (0, 1), (2, 1), (1, 0)]          # (frame format, PL_STEM): the row stream on all formats, the tile kernel on fp16


def stem_instruments(fmt):
    return ('gauss',) if fmt == 2 else INSTRUMENTS


STEM_EDGES = [dict(n=1, h=8, w=16), dict(n=4, h=3, w=32)]

# lfd_pl_block64: (n, h, w)
BLOCK_CASES = [
    (43, 35, 59),     # 86 columns of work -> 2 segments of 18 and 17 rows: taller than twice the input ring (8); width 30 + 29
    (2, 9, 61),       # 6 columns -> 42 segments wanted: ceil(9 / 42) = 1 row clamped to SH = 4; last segment 1 row; width 60 + 1
    (3, 3, 60),       # h < 4: one segment of 3 rows; width 30 * 2
    (1, 1, 1),
]


# ------------------------------------------------------------------------------------------------ operands of a case
def conv_operands(kind, key, cout, n, h, w, variant, seed=0):
    """everything a conv case feeds the kernel and the float64 results it must give.  dict with x, w, b and, per variant,
    res / w2, b2, relu2 / wd, bd; 'ref' (and 'ref_mid', 'ref_ds')"""
    cin, ks, stride, _ = key
    s = seed * 7919 + cin * 31 + ks * 7 + stride * 3 + cout + 1000 * INSTRUMENTS.index(kind) + 17 * len(variant)
    chained = variant == 'tail'
    # a chained pair multiplies two filters' gains: fewer, smaller taps in both
    nnz, amp = (12, 1) if chained else (48, 2)
    o = dict(kind=kind, x=activations(kind, (n, h, w, cin), s), w=filters(kind, cout, cin, ks, s + 1, nnz, amp), b=bias(kind, cout, s + 2))
    relu = variant not in ('gn', 'out32')
    o['relu'] = relu
    if variant == 'res':
        oh, ow = out_hw(h, w, ks, stride)
        o['res'] = activations(kind if kind != 'wlo' else 'int', (n, oh, ow, cout), s + 3) if kind != 'gauss' else \
            from_planes(to_planes(torch.randn(n, oh, ow, cout, generator=_gen(s + 3))))
        o['ref'] = ref_conv(o['x'], o['w'], o['b'], ks, stride, True, o['res'])
    elif chained:
        o['w2'], o['b2'] = filters(later(kind), cout, cout, 1, s + 4, 6, 1), bias(kind, cout, s + 5)
        o['relu2'] = ks == 3          # the stem pair ends on a ReLU; a GroupNorm follows the neck -> tower pair
        o['ref_mid'], o['ref'] = ref_chained(o['x'], o['w'], o['b'], ks, stride, o['w2'], o['b2'], o['relu2'])
    elif variant == 'ds':
        o['wd'], o['bd'] = filters(kind, cout, cin, 1, s + 6, 24, 2), bias(kind, cout, s + 7)
        o['ref'] = ref_conv(o['x'], o['w'], o['b'], ks, stride, True)
        o['ref_ds'] = ref_conv(o['x'], o['wd'], o['bd'], 1, stride, False)
    else:
        o['ref'] = ref_conv(o['x'], o['w'], o['b'], ks, stride, relu)
    return o


def c3_operands(kind, n, h, w, seed=0):
    s = seed * 7919 + 64 + 1000 * INSTRUMENTS.index(kind)
    o = dict(kind=kind, x=activations(kind, (n, h, w, 64), s), w=filters(kind, 64, 64, 3, s + 1), b=bias(kind, 64, s + 2))
    o['res'] = activations(kind if kind != 'wlo' else 'int', (n, h, w, 64), s + 3) if kind != 'gauss' else \
        from_planes(to_planes(torch.randn(n, h, w, 64, generator=_gen(s + 3))))
    pre = ref_conv(o['x'], o['w'], o['b'], 3, 1, False)
    o['ref'] = {'plain': pre.relu(), 'res_relu': (pre + o['res'].double()).relu(), 'res': pre + o['res'].double()}
    return o


def block_operands(kind, n, h, w, seed=0):
    s = seed * 7919 + 640 + 1000 * INSTRUMENTS.index(kind) + h * 13 + w
    g = _gen(s)
    if kind == 'gauss':           # tests/test_gpu_planes_block.py::_block_inputs
        x = from_planes(to_planes(torch.randn(n, h, w, 64, generator=g)))
        w1 = torch.randn(64, 64, 3, 3, generator=g) * (1.0 / 576 ** 0.5)
        w2 = torch.randn(64, 64, 3, 3, generator=g) * (1.0 / 576 ** 0.5)
        b1, b2 = torch.randn(64, generator=g) * 0.1, torch.randn(64, generator=g) * 0.1
    else:
        x = activations(kind, (n, h, w, 64), s)
        w1, b1 = filters(kind, 64, 64, 3, s + 1, 12, 1), bias(kind, 64, s + 2)
        w2, b2 = filters(later(kind), 64, 64, 3, s + 3, 6, 1), bias(kind, 64, s + 4)
    o = dict(kind=kind, x=x, w1=w1, b1=b1, w2=w2, b2=b2)
    o['ref_mid'], o['ref'] = ref_block(x, w1, b1, w2, b2)
    return o


def stem_frames(kind, fmt, n, h, w, seed=0):
    """fmt 0: fp32 NCHW, 1: fp16 NHWC, 2: uint8 NHWC (gauss only).  Returns (frame tensor as the kernel takes it, values [N,H,W,3])"""
    g = _gen(seed * 7919 + 77 + fmt * 5 + 1000 * INSTRUMENTS.index(kind))
    if fmt == 2:
        assert kind == 'gauss', 'simple_normalize is not dyadic'
        x = torch.randint(0, 256, (n, h, w, 3), generator=g, dtype=torch.uint8)
        return x, (x.float() / 255 - 0.5) / 0.5
    if kind == 'gauss':
        v = torch.rand(n, h, w, 3, generator=g) * 2 - 1
        if fmt == 1:
            v = v.half().float()
    else:
        v = torch.randint(-3, 4, (n, h, w, 3), generator=g).float()
        if kind == 'xlo':
            # fp16 frames carry no lo plane: multiples of 1/256 there (exact in fp16); fp32 frames get a real lo plane
            v = v + torch.randint(-8, 9, (n, h, w, 3), generator=g).float() / (4096 if fmt == 0 else 256)
    return (v.permute(0, 3, 1, 2).contiguous() if fmt == 0 else v.half()), v


def stem_operands(kind, fmt, n, h, w, seed=0):
    s = seed * 7919 + 900 + 1000 * INSTRUMENTS.index(kind)
    frame, v = stem_frames(kind, fmt, n, h, w, seed)
    if kind == 'gauss':           # tests/test_gpu_planes.py::_stem2x_case
        g = _gen(s)
        c = 64
        ws = [torch.randn(c, 3, 3, 3, generator=g) * 0.3, torch.randn(c, c, 1, 1, generator=g) * (1.0 / c ** 0.5),
              torch.randn(c, c, 3, 3, generator=g) * (1.0 / (9 * c) ** 0.5), torch.randn(c, c, 1, 1, generator=g) * (1.0 / c ** 0.5)]
        bs = [torch.randn(c, generator=g) for _ in range(4)]
    else:
        k2 = later(kind)
        ws = [filters(kind, 64, 3, 3, s + 1, 6, 1), filters(k2, 64, 64, 1, s + 2, 4, 1), filters(k2, 64, 64, 3, s + 3, 6, 1),
              filters(k2, 64, 64, 1, s + 4, 4, 1)]
        bs = [bias(kind, 64, s + 5 + i) for i in range(4)]
    o = dict(kind=kind, fmt=fmt, frame=frame, values=v, ws=ws, bs=bs)
    o['stages'] = ref_stem(v, ws, bs)
    o['ref'] = o['stages'][-1]
    return o


def gnin_operands(cout, n, h, w, seed=0):
    """a stored 128-channel tensor t (planes), its GroupNorm parameters, and a 1x1 conv of GroupNorm(t) + ReLU as the kernel's
    LDS tile holds it (rounded through planes)"""
    g = _gen(seed * 7919 + 4200 + cout)
    t = from_planes(to_planes(torch.randn(n, h, w, 128, generator=g) * 2))
    gamma, beta = torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g) * 0.1
    wt, b = torch.randn(cout, 128, 1, 1, generator=g) * 0.09, torch.randn(cout, generator=g)
    y = rt(ref_group_norm(t.double().reshape(n, h * w, 128), gamma, beta)).reshape(n, h, w, 128)
    return dict(t=t, gamma=gamma, beta=beta, w=wt, b=b, ref=ref_conv(y, wt, b, 1, 1, False))


def head_first_operands(kind, cin, n, pixels, seed=0):
    """modes 0 (cin 64 / 128: neck + first tower conv) and 3 (cin 128, tower conv on stored planes; w0 only): per level its own
    input and filters"""
    out = []
    for l, p in enumerate(pixels):
        s = seed * 7919 + 300 + 1000 * INSTRUMENTS.index(kind) + cin + 50 * l
        x = activations(kind, (n, p, cin), s)
        if kind == 'gauss':
            g = _gen(s + 1)
            w0, b0 = torch.randn(128, cin, generator=g) / cin ** 0.5, torch.randn(128, generator=g)
            w1, b1 = torch.randn(128, 128, generator=g) / 128 ** 0.5, torch.randn(128, generator=g)
        else:
            # (wlo on the 2^-12 grid here: the squares in the GroupNorm sums must stay multiples of 2^-24)
            w0, b0 = filters(kind, 128, cin, 1, s + 1, 8, 1, 4096).reshape(128, cin), bias(kind, 128, s + 2)
            w1, b1 = filters(later(kind), 128, 128, 1, s + 3, 4, 1).reshape(128, 128), bias(kind, 128, s + 4)
        mid, t1 = ref_head_first(x, w0, b0, w1, b1)
        t3 = x.double() @ w0.double().t() + b0.double()          # mode 3: one conv, no ReLU
        out.append(dict(x=x, w0=w0, b0=b0, w1=w1, b1=b1, mid=mid, t1=t1, t3=t3))
    return out


def head_chain_operands(n, pixels, channels, seed=0):
    """the Gaussian chain behind mode 0: GroupNorm parameters, the second tower conv (mode 1) and the output convs (mode 2) for
    `channels` = (f_c0, f_c1); drawn as tests/test_gpu_planes.py::test_pl_head_levels_chain_vs_float64 draws them"""
    out = []
    for l, p in enumerate(pixels):
        g = _gen(seed * 7919 + 500 + 50 * l + channels[0] * 3 + channels[1])
        ct = channels[0] + channels[1]
        w2, b2 = torch.randn(128, 128, generator=g) / 128 ** 0.5, torch.randn(128, generator=g)
        w3, b3 = torch.randn(ct, 128, generator=g) / 128 ** 0.5, torch.randn(ct, generator=g)
        ga1, be1, ga2, be2 = [torch.randn(128, generator=g) * s_ + o_ for s_, o_ in ((0.3, 1.0), (0.3, 0.0), (0.3, 1.0), (0.3, 0.0))]
        out.append(dict(w2=w2, b2=b2, w3=w3, b3=b3, ga1=ga1, be1=be1, ga2=ga2, be2=be2, scale=torch.tensor([1.7 + l])))
    return out


# ------------------------------------------------------------------------------------------------ wrong references
# a reference wrong in exactly one way a walk bug would produce; the comparison must tell each from the right one
def wrong_seam_pixel(ref, tw, th):
    """one pixel at a tile seam (first pixel of the second tile column / row) takes its left neighbour's value"""
    bad = ref.clone()
    y, x = min(th, ref.shape[1] - 1), min(tw, ref.shape[2] - 1)
    bad[-1, y, x] = ref[-1, y, x - 1] if x > 0 else ref[-1, y - 1, x]
    return bad


def wrong_last_tile_of_run(ref, run, tiles, tw, th):
    """the last tile of a run holds the previous tile's values (a stale buffer)"""
    bad = ref.clone()
    (i1, ty1, tx1), (i0, ty0, tx0) = tiles[run[-1]][:3], tiles[run[-2]][:3]
    dst = bad[i1, ty1 * th:(ty1 + 1) * th, tx1 * tw:(tx1 + 1) * tw]
    src = ref[i0, ty0 * th:(ty0 + 1) * th, tx0 * tw:(tx0 + 1) * tw]
    hh, ww = min(dst.shape[0], src.shape[0]), min(dst.shape[1], src.shape[1])
    dst[:hh, :ww] = src[:hh, :ww]
    return bad


def wrong_image_after_change(ref, run, tiles, tw, th):
    """the first tile after an image change inside a run is computed for the previous image"""
    bad = ref.clone()
    for a, b in zip(run, run[1:]):
        if tiles[a][0] != tiles[b][0]:
            i, ty, tx = tiles[b][:3]
            bad[i, ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw] = ref[tiles[a][0], ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw]
            return bad
    raise AssertionError('no image change in this run')


def gate_fails(bad, ref, tol):
    return float((bad.double() - ref.double()).abs().max()) > tol * max(1.0, float(ref.abs().max()))
