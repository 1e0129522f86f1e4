"""tests/golden/conv_cases.py -- seeded inputs, the float64 reference, the restated launch geometry and the case tables for
the forward conv kernels of csrc/conv_impl.h (entry files csrc/conv.hip, conv_stats.hip, conv_acc32.hip) and for
csrc/conv_small.hip and csrc/dgrad_s2.hip beside it (tests/test_conv_reference_host.py keeps the reference and the tables
honest on the CPU, tests/test_gpu_conv_exact.py compares the kernels with them).  The generators return CPU tensors; no
ctypes.  conv_ref / dgrad_ref run on whatever device their operands are on.

The instrument: x holds INTEGERS in [-3, 3] (fp16), the filter integers in [-2, 2], the bias integers in [-8, 8] (fp32), the
residual integers in [-64, 64] (fp16).  Every product is an integer of magnitude <= 6 and every fp32 partial sum an integer
of magnitude <= 6 * K + 8 (K = ks * ks * cin <= 1152) < 2^24, so fp32 accumulation is exact in any order and under any
rounding inside the MFMA.  An fp16 output holds every integer of magnitude <= 2048, an fp32 (ACC32) output every integer
below 2^24: while the float64 reference stays inside that (exact_cap() states it; the host test checks it for every integer
case) the kernel must equal the reference bit for bit.  A chained 1x1 ("tail") rounds its fp16 intermediate, so that one
has to stay <= 2048 as well; tail cases draw the main filter from [-1, 1] and a sparse tail filter (a quarter non-zero).

Layouts: x [n, h, w, cin] and outputs [n, oh, ow, cout] are NHWC; filters are OIHW [cout, cin, ks, ks]; pad = ks // 2."""
import collections
import functools

import torch

X_HI, W_HI, BIAS_HI, RES_HI = 3, 2, 8, 64
W_HI_TAIL = 1                          # main filter of a tail case (see above)
F16_EXACT, F32_EXACT = 2048, 2 ** 24   # integers of at most this magnitude are all representable
GAUSS_GATE = 1.2e-3                    # tests/test_gpu_conv.py::_run: |got - ref| <= 1.2e-3 * max(|ref|, 1)


def out_hw(h, w, ks, stride):
    pad = ks // 2
    return (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1


# ------------------------------------------------------------------------------------------------ seeded inputs
def int_tensor(shape, hi, seed):
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(-hi, hi + 1, tuple(shape), generator=g, dtype=torch.int16)


Operands = collections.namedtuple('Operands', 'x w b res w2 b2 wd bd')


def int_operands(n, h, w, cin, cout, ks, stride, seed, tail=False, w_hi=None):
    """-> Operands of CPU tensors with integer values: x fp16, w fp32 OIHW, b fp32, res fp16 [n, oh, ow, cout]; w2 / b2 the
    chained 1x1 (cout -> cout, about a quarter non-zero) when `tail`, else None; wd / bd a 1x1 filter cin -> cout (the
    downsample branch)."""
    oh, ow = out_hw(h, w, ks, stride)
    w_hi = (W_HI_TAIL if tail else W_HI) if w_hi is None else w_hi
    s = int(seed)
    x = int_tensor((n, h, w, cin), X_HI, s).half()
    wt = int_tensor((cout, cin, ks, ks), w_hi, s + 100003).float()
    b = int_tensor((cout,), BIAS_HI, s + 200003).float()
    res = int_tensor((n, oh, ow, cout), RES_HI, s + 300007).half()
    w2 = b2 = None
    if tail:
        keep = torch.rand((cout, cout, 1, 1), generator=torch.Generator().manual_seed(s + 400009)) < 0.25
        w2 = int_tensor((cout, cout, 1, 1), W_HI, s + 500009).float() * keep
        b2 = int_tensor((cout,), BIAS_HI, s + 600011).float()
    wd = int_tensor((cout, cin, 1, 1), W_HI, s + 700001).float()
    bd = int_tensor((cout,), BIAS_HI, s + 800011).float()
    return Operands(x, wt, b, res, w2, b2, wd, bd)


def gauss_operands(n, h, w, cin, cout, ks, stride, seed, tail=False):
    """the distribution of tests/test_gpu_conv.py::_run: x ~ N(0, 0.5^2), filters ~ N(0, 1 / K) rounded to fp16, biases
    ~ N(0, 0.1^2), residual ~ N(0, 0.5^2)"""
    oh, ow = out_hw(h, w, ks, stride)
    g = torch.Generator().manual_seed(int(seed))
    x = (torch.randn(n, h, w, cin, generator=g) * 0.5).half()
    wt = (torch.randn(cout, cin, ks, ks, generator=g) * (1.0 / (cin * ks * ks) ** 0.5)).half().float()
    b = torch.randn(cout, generator=g) * 0.1
    res = (torch.randn(n, oh, ow, cout, generator=g) * 0.5).half()
    w2 = b2 = None
    if tail:
        w2 = (torch.randn(cout, cout, 1, 1, generator=g) * (1.0 / cout ** 0.5)).half().float()
        b2 = torch.randn(cout, generator=g) * 0.1
    wd = (torch.randn(cout, cin, 1, 1, generator=g) * (1.0 / cin ** 0.5)).half().float()
    bd = torch.randn(cout, generator=g) * 0.1
    return Operands(x, wt, b, res, w2, b2, wd, bd)


# ------------------------------------------------------------------------------------------------ float64 reference
def pro_apply(y, stats, gamma, beta):
    """the BN + ReLU prologue as k_bn_apply forms it: a = gamma * rstd, b = beta - mean * a in fp32, z = relu(fma(y, a, b))
    rounded to fp16.  y [.., c] fp16, stats fp32 [2 * c] (mean | rstd)."""
    c = y.size(-1)
    a = gamma.float() * stats[c:].float()
    b = beta.float() - stats[:c].float() * a
    return torch.addcmul(b, y.float(), a).relu().half()


def conv_ref(x, w, bias=None, stride=1, residual=None, relu=False, tail=None, ds=None, pro=None, dtype=torch.float64, tap_hook=None):
    """out[n, oy, ox, :] = sum over taps (ky, kx) of xpad[n, oy * stride + ky, ox * stride + kx, :] @ w[:, :, ky, kx]^T:
    ks * ks shifted matmuls over the zero-padded input, no conv call.  Then + bias, + residual, ReLU; tail = (w2, b2, relu2)
    rounds the result to fp16 and applies a 1x1 conv (+ b2, ReLU); ds = (wd, bd) also returns the 1x1 stride-`stride` conv
    of x (the centre tap's pixels) + bd without ReLU: -> (out, ident); pro = (stats, gamma, beta) convolves pro_apply(x).
    -> [n, oh, ow, cout] in `dtype`.  tap_hook(ky, kx, term [n, oh, ow, cout]) -> term is for the host test alone, which builds
    deliberately wrong references with it."""
    if pro is not None:
        x = pro_apply(x, *pro)
    n, h, wd_, cin = x.shape
    cout, cin_w, ks, _ = w.shape
    assert cin_w == cin and ks in (1, 3)
    pad = ks // 2
    oh, ow = out_hw(h, wd_, ks, stride)
    xp = torch.zeros((n, h + 2 * pad, wd_ + 2 * pad, cin), dtype=dtype, device=x.device)
    xp[:, pad:pad + h, pad:pad + wd_] = x.to(dtype)
    wt = w.to(dtype)
    out = torch.zeros((n * oh * ow, cout), dtype=dtype, device=x.device)
    for ky in range(ks):
        for kx in range(ks):
            xs = xp[:, ky:ky + (oh - 1) * stride + 1:stride, kx:kx + (ow - 1) * stride + 1:stride]
            term = xs.reshape(-1, cin) @ wt[:, :, ky, kx].t()
            if tap_hook is not None:
                term = tap_hook(ky, kx, term.reshape(n, oh, ow, cout)).reshape(-1, cout)
            out += term
    out = out.reshape(n, oh, ow, cout)
    if bias is not None:
        out = out + bias.to(dtype)
    if residual is not None:
        out = out + residual.to(dtype)
    if relu:
        out = out.relu()
    if tail is not None:
        w2, b2, relu2 = tail
        mid = out.float().half().to(dtype)          # the intermediate is stored as fp16
        out = mid @ w2.to(dtype)[:, :, 0, 0].t() + b2.to(dtype)
        if relu2:
            out = out.relu()
    if ds is not None:
        wds, bds = ds
        xc = xp[:, pad:pad + (oh - 1) * stride + 1:stride, pad:pad + (ow - 1) * stride + 1:stride]
        return out, xc @ wds.to(dtype)[:, :, 0, 0].t() + bds.to(dtype)
    return out


def dgrad_ref(dy, w, h, w_in, stride, residual=None, dtype=torch.float64):
    """the transposed convolution: dx[n, iy, ix, :] = sum over (oy, ox, ky, kx) with oy * stride + ky - pad == iy (same for x)
    of dy[n, oy, ox, :] @ w[:, :, ky, kx], as ks * ks strided scatter-adds into the padded dx; + residual.
    dy [n, oh, ow, cout], w OIHW [cout, cin, ks, ks] of the FORWARD conv -> [n, h, w_in, cin]"""
    n, oh, ow, cout = dy.shape
    cin, ks = w.size(1), w.size(2)
    pad = ks // 2
    assert (oh, ow) == out_hw(h, w_in, ks, stride)
    dxp = torch.zeros((n, h + 2 * pad + stride, w_in + 2 * pad + stride, cin), dtype=dtype, device=dy.device)
    d = dy.to(dtype).reshape(-1, cout)
    wt = w.to(dtype)
    for ky in range(ks):
        for kx in range(ks):
            dxp[:, ky:ky + (oh - 1) * stride + 1:stride, kx:kx + (ow - 1) * stride + 1:stride] += (d @ wt[:, :, ky, kx]).reshape(n, oh, ow, cin)
    dx = dxp[:, pad:pad + h, pad:pad + w_in]
    if residual is not None:
        dx = dx + residual.to(dtype)
    return dx.contiguous()


def exact_cap(case):
    """the largest magnitude every stored value of an exact run may have: 2048 where it is stored as fp16 (the output, the
    tail's intermediate, both outputs of the downsample launch), 2^24 - 1 for the fp32 output of an ACC32 kernel.  The
    accumulators themselves never exceed X_HI * W_HI * K + BIAS_HI + RES_HI <= 6984 < 2^24."""
    assert X_HI * W_HI * case.ks * case.ks * case.cin + BIAS_HI + RES_HI < F32_EXACT
    return F32_EXACT - 1 if case.variant == 'acc32' else F16_EXACT


# ------------------------------------------------------------------------------------------------ launch geometry
Geometry = collections.namedtuple('Geometry', 'TW RPT PT PG TH NBUF')


def conv_geometry(cin, ks, stride, nct, tail):
    """Cfg<CIN, KS, S, NCT, WREG, TAIL> of csrc/conv_impl.h restated (nct = cout / 32: every dispatch key has one cout group)"""
    TW = 16 if stride == 2 or (cin == 64 and ks == 3) else 32
    RPT = 32 // TW
    PT = 2 if stride == 1 else 1
    PG = 4 // nct
    TH = PG * PT * RPT
    NBUF = 2 if stride == 1 or (cin == 64 and ks == 3 and nct == 2 and not tail) else 1
    return Geometry(TW, RPT, PT, PG, TH, NBUF)


Launch = collections.namedtuple('Launch', 'tiles_x tiles_y ntiles blocks')


def conv_launch(n, oh, ow, geo, cgroups=1):
    """launch_conv_ restated: tiles of TH x TW output pixels, min(512 / cgroups, 8 * ceil(ntiles / 8)) workgroups"""
    tx, ty = -(-ow // geo.TW), -(-oh // geo.TH)
    nt = n * tx * ty
    return Launch(tx, ty, nt, max(1, min(512 // cgroups, 8 * -(-nt // 8))))


def walk(ntiles, blocks):
    """the persistent tile walk -> [tiles of workgroup b]: XCD b & 7 owns [xcd * ceil(ntiles / 8), next range) cut at ntiles,
    workgroup b starts at its b >> 3-th tile and steps by the number of workgroups of that XCD"""
    per_xcd = -(-ntiles // 8)
    out = []
    for b in range(blocks):
        xcd, bix = b & 7, b >> 3
        begin = xcd * per_xcd
        end = min(begin + per_xcd, ntiles)
        out.append(list(range(begin + bix, end, (blocks + 7 - xcd) // 8)))
    return out


DGRAD_TH, DGRAD_TW = 8, 16             # csrc/dgrad_s2.hip: tiles of dy, the same walk on min(512, 8 * ceil(ntiles / 8)) workgroups
DGRAD_GEOMETRY = Geometry(DGRAD_TW, 2, 2, 2, DGRAD_TH, 2)


def dgrad_launch(n, h, w):
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return conv_launch(n, oh, ow, DGRAD_GEOMETRY)


SPLITK_MAX_PIXELS = 16384              # csrc/conv.hip: 128 -> 128 3x3 s1 with n * oh * ow <= this takes csrc/conv_small.hip


def takes_splitk(n, oh, ow):
    return n * oh * ow <= SPLITK_MAX_PIXELS


# ------------------------------------------------------------------------------------------------ case tables
# (cin, ks, stride, cout, tail), in the order of the switch statements
# csrc/conv.hip:63 conv_dispatch
DISPATCH_KEYS = [
    (64, 3, 1, 64, 0), (64, 3, 2, 64, 0), (64, 3, 2, 64, 1), (64, 3, 2, 128, 0), (64, 3, 1, 128, 0), (64, 3, 1, 32, 0),
    (64, 1, 1, 32, 0), (64, 1, 1, 64, 0), (64, 1, 1, 128, 0), (64, 1, 2, 64, 0), (64, 1, 2, 128, 0),
    (128, 3, 1, 128, 0), (128, 3, 2, 128, 0), (128, 3, 1, 64, 0), (128, 3, 2, 64, 0), (128, 1, 1, 64, 0), (128, 1, 1, 128, 0),
    (128, 1, 2, 128, 0),
    (32, 3, 2, 32, 1), (32, 3, 2, 32, 0), (32, 3, 2, 64, 0), (32, 3, 1, 32, 0), (32, 1, 1, 32, 0), (32, 1, 2, 64, 0), (32, 1, 1, 128, 0),
]
# csrc/conv_stats.hip:54 conv_bn_stats (STATS); the 1x1 s1 64-input keys also carry the BN + ReLU prologue (PRO, :18)
STATS_KEYS = [(64, 3, 1, 64, 0), (64, 3, 2, 64, 0), (64, 3, 2, 128, 0), (64, 1, 1, 64, 0), (64, 1, 1, 128, 0), (64, 1, 2, 64, 0),
              (64, 1, 2, 128, 0), (128, 1, 1, 128, 0)]
PRO_KEYS = [(64, 1, 1, 64, 0), (64, 1, 1, 128, 0)]
# csrc/conv_stats.hip:126 lfd_conv1x1_dgrad_bn_bwd_sums_nhwc_f16 (BSUM)
BSUM_KEYS = [(64, 1, 1, 64, 0)]
# csrc/conv_acc32.hip:28 lfd_conv2d_nhwc_f16_acc32
ACC32_KEYS = [
    (32, 3, 2, 32, 0), (32, 3, 2, 64, 0), (32, 1, 1, 32, 0), (32, 1, 2, 64, 0),
    (64, 3, 1, 64, 0), (64, 3, 2, 64, 0), (64, 3, 2, 128, 0),
    (64, 1, 1, 64, 0), (64, 1, 1, 128, 0), (64, 1, 2, 64, 0), (64, 1, 2, 128, 0),
    (128, 3, 1, 128, 0), (128, 3, 2, 128, 0),
    (128, 1, 1, 64, 0), (128, 1, 1, 128, 0), (128, 1, 2, 128, 0),
    (128, 3, 1, 64, 0), (64, 3, 1, 32, 0), (64, 1, 1, 32, 0),
]
# the downsample launch (csrc/conv.hip:34): the 3x3 s2 keys without tail that the backbones use (tests/test_gpu_conv.py)
DS_KEYS = [(64, 3, 2, 64, 0), (64, 3, 2, 128, 0), (128, 3, 2, 128, 0), (32, 3, 2, 64, 0)]
# data-gradient packs: every stride-1 key without tail is the data gradient of a conv cout_key -> cin_key (roles swapped)
DGRAD_KEYS = [k for k in DISPATCH_KEYS if k[2] == 1 and not k[4]]

Case = collections.namedtuple('Case', 'cin ks stride cout tail variant kind n h w relu relu2')
WALK_IMAGES = 174                      # x 6 tiles = 1044 tiles on 512 workgroups: see walk_shape


def key_geometry(key):
    cin, ks, stride, cout, tail = key
    return conv_geometry(cin, ks, stride, cout // 32, bool(tail))


def in_size(o, stride, odd=True):
    """an input extent whose output extent is o"""
    return o if stride == 1 else (2 * o - 1 if odd else 2 * o)


def walk_shape(key):
    """174 images of (TH + 1) x (2 TW + 1) output pixels: 2 x 3 tiles each (two full, one right-ragged column of one pixel, a
    bottom-ragged row of one pixel under each), 1044 tiles: XCD ranges of 131 tiles (the last 127) on 64 workgroups each ->
    three tiles on some, two on most, one on the last workgroup of XCD 7.  A workgroup's consecutive tiles are 64 apart: in
    different images, and (64 = 4 mod 6) at different places of the image, so a full tile is followed by a ragged one and a
    ragged one by a full one.  Odd inputs under stride 2."""
    geo = key_geometry(key)
    return WALK_IMAGES, in_size(geo.TH + 1, key[2]), in_size(2 * geo.TW + 1, key[2])


def map_shape(key):
    """2 images of (2 TH + 1) x (2 TW + 5) output pixels: 3 x 3 tiles with an interior tile, a ragged right column of 5 pixels,
    a ragged bottom row of 1 pixel and the corner.  Under stride 2 an even height and an odd width."""
    geo = key_geometry(key)
    return 2, in_size(2 * geo.TH + 1, key[2], odd=False), in_size(2 * geo.TW + 5, key[2])


def edge_shapes(key):
    """-> [(n, h, w)]: one pixel; exactly one tile; TH x (TW + 1); (TH + 1) x TW; under stride 2 one tile from an even and from
    an odd input and a 2 x 2 input; 3 x 3 tiles in one image = 9 tiles on 16 workgroups (XCD ranges of 2: XCD 4 gets one tile,
    XCDs 5 - 7 none)"""
    geo = key_geometry(key)
    s = key[2]
    TH, TW = geo.TH, geo.TW
    out = [(1, 1, 1), (1, in_size(TH, s), in_size(TW, s)), (1, in_size(TH, s), in_size(TW + 1, s)),
           (1, in_size(TH + 1, s), in_size(TW, s)), (1, in_size(2 * TH + 1, s), in_size(2 * TW + 1, s))]
    if s == 2:
        out += [(1, 2 * TH, 2 * TW), (1, 2, 2), (2, 2 * TH + 2, 2 * TW + 1)]
    return out


def variants(key):
    """plain; residual for stride 1 without tail; the two tail keys are their own variant.  (The downsample branch of the
    3x3 s2 keys has its own entry point and table, DS_KEYS.)"""
    cin, ks, stride, cout, tail = key
    if tail:
        return ['tail']
    return ['plain', 'res'] if stride == 1 else ['plain']


def _case(key, variant, kind, shape):
    # ReLU would hide every error of a negative output: plain cases and map-shaped tail cases run without it; residual cases
    # (the closing conv of a block) and walk-shaped tail / downsample cases run as the networks run them
    relu = variant == 'res' or (variant in ('tail', 'ds') and kind == 'walk')
    return Case(*key, variant, kind, *shape, int(relu), int(relu and variant == 'tail'))


def conv_cases(kinds=('walk', 'map')):
    """every key of conv_dispatch x its variants x the two shapes"""
    return [_case(k, v, kind, walk_shape(k) if kind == 'walk' else map_shape(k))
            for k in DISPATCH_KEYS for v in variants(k) for kind in kinds]


def table_cases(keys, variant, kinds=('walk', 'map')):
    return [_case(k, variant, kind, walk_shape(k) if kind == 'walk' else map_shape(k)) for k in keys for kind in kinds]


def ds_cases():
    return table_cases(DS_KEYS, 'ds')


def acc32_cases():
    return table_cases(ACC32_KEYS, 'acc32')


def stats_cases():
    return table_cases(STATS_KEYS, 'stats')


# the prologue / backward-sums kernels: the walk and map shapes of their keys, and 260 x 5 x 33 (2 x 2 tiles each, 1040 tiles:
# eight equal XCD ranges of 130, a workgroup's tiles all at the same place of their images)
PRO_BSUM_EXTRA = (260, 5, 33)


def pro_cases():
    return table_cases(PRO_KEYS, 'pro') + [_case(k, 'pro', 'walk260', PRO_BSUM_EXTRA) for k in PRO_KEYS]


def bsum_cases():
    return table_cases(BSUM_KEYS, 'bsum') + [_case(k, 'bsum', 'walk260', PRO_BSUM_EXTRA) for k in BSUM_KEYS]


def edge_cases():
    """-> [(key, [(n, h, w)])] for every dispatch key (plain, or tail for the two tail keys)"""
    return [(k, edge_shapes(k)) for k in DISPATCH_KEYS]


# csrc/dgrad_s2.hip: (n, h, w) of dx.  174 images of 18 x 66: dy 9 x 33 = 2 x 3 tiles each, 1044 tiles; then the edges: one pixel, 2 x 2,
# exactly one dy tile from an odd and from an even dx, one past it either way, 9 tiles, a ragged multi-tile map
DGRAD_S2_WALK = (WALK_IMAGES, 18, 66)
DGRAD_S2_EDGES = [(1, 1, 1), (1, 2, 2), (1, 15, 31), (1, 16, 32), (1, 16, 33), (1, 17, 32), (1, 34, 66), (2, 37, 53)]
# csrc/conv_small.hip (n, h, w): the two last-stage maps, then 16384 pixels (split-K) and 16512 (the streamed-weight kernel)
SPLITK_SHAPES = [(1, 17, 30), (8, 17, 30), (2, 23, 40), (1, 128, 128), (1, 128, 129)]
SPLITK_KEY = (128, 3, 1, 128, 0)


def case_id(c):
    return '%dto%d_k%ds%d%s_%s_%s_%dx%dx%d' % (c.cin, c.cout, c.ks, c.stride, 't' if c.tail else '', c.variant, c.kind, c.n, c.h, c.w)


def key_id(k):
    return '%dto%d_k%ds%d%s' % (k[0], k[3], k[1], k[2], 't' if k[4] else '')


def case_seed(c):
    return sum(int(v) * p for v, p in zip((c.cin, c.ks, c.stride, c.cout, c.tail, c.n, c.h, c.w), (1, 3, 7, 11, 13, 17, 19, 23)))


def case_key(c):
    return (c.cin, c.ks, c.stride, c.cout, c.tail)


@functools.lru_cache(maxsize=4)
def case_int_operands(c):
    """cached: the tests that run a case more than once share its operands"""
    return int_operands(c.n, c.h, c.w, c.cin, c.cout, c.ks, c.stride, case_seed(c), tail=bool(c.tail))


def case_gauss_operands(c):
    return gauss_operands(c.n, c.h, c.w, c.cin, c.cout, c.ks, c.stride, case_seed(c) + 1, tail=bool(c.tail))


def case_ref(c, ops_, dtype=torch.float64):
    """the reference of a case on the operands `ops_` (any device): the plain / res / tail / acc32 / stats output, or
    (out, ident) for 'ds'"""
    if c.variant == 'ds':
        return conv_ref(ops_.x, ops_.w, ops_.b, c.stride, relu=bool(c.relu), ds=(ops_.wd, ops_.bd), dtype=dtype)
    if c.variant in ('acc32', 'plain'):
        return conv_ref(ops_.x, ops_.w, ops_.b, c.stride, relu=bool(c.relu), dtype=dtype)
    if c.variant == 'res':
        return conv_ref(ops_.x, ops_.w, ops_.b, c.stride, residual=ops_.res, relu=bool(c.relu), dtype=dtype)
    if c.variant == 'tail':
        return conv_ref(ops_.x, ops_.w, ops_.b, c.stride, relu=bool(c.relu), tail=(ops_.w2, ops_.b2, bool(c.relu2)), dtype=dtype)
    if c.variant in ('stats', 'pro', 'bsum'):          # the bare conv in front of a BatchNorm: no bias, no ReLU
        return conv_ref(ops_.x, ops_.w, None, c.stride, dtype=dtype)
    raise ValueError(c.variant)
