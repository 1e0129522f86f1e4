"""tests/golden/norm_cases.py -- seeded cases, float64 references, the fp32 restatement of the forward apply passes and the
derived error bounds for the train-mode BatchNorm / GroupNorm kernels of csrc/train.hip (tests/test_norm_reference_host.py keeps
the references honest on the CPU, tests/test_gpu_train_norms.py compares the kernels with them).  CPU tensors only: no GPU, no
ctypes.

Layouts: BatchNorm tensors are NHWC, flattened here to [m, c] (m = n * h * w pixels); a level-concatenated tensor is [n, P, c]
with level l in rows [start_l, start_l + hw_l) of every image.  GroupNorm tensors are [n, P, c], c = 8 * groups (group j =
channels 8j .. 8j+7), P = sum(seg_hw); statistics are [n, nseg, 2, groups] (mean, rstd), as the kernels store them.

Error model (nothing tuned): u16 = 2^-11 and u32 = 2^-24 are the unit roundoffs of fp16 and fp32.
* store_bound: a value that leaves the kernel as fp16 after a short fp32 expression.
* sum_bound: an fp32 sum whose longest chain of additions has L terms before the fp64 final pass.
The references that take `stats` evaluate xhat in float64 FROM THOSE STATS (the kernel's own), so that the statistics are judged
once, by their own tolerances, and not a second time inside every output."""
import functools
import math

import torch

EPS, MOMENTUM = 1e-5, 0.1
U16, U32 = 2.0 ** -11, 2.0 ** -24
LOSS_SCALE = 16.0
MAX_LEVELS = 8                    # LFD_MAX_LEVELS (include/lfd_hip.h)
THREADS, BN_MAX_BLOCKS = 256, 1024


# ------------------------------------------------------------------------------------------------ seeded inputs
def rand16(shape, seed, scale=1.0, shift=0.0):
    g = torch.Generator().manual_seed(int(seed))
    return (torch.randn(shape, generator=g) * scale + shift).half()


def norm_params(c, seed):
    """gamma ~ U(0.5, 1.5), beta ~ N(0, 0.3^2), fp32 (the distribution of tests/test_gpu_train_convs.py)"""
    g = torch.Generator().manual_seed(1000 + int(seed))
    return torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3


def running_stats(c, seed):
    g = torch.Generator().manual_seed(2000 + int(seed))
    return torch.randn(c, generator=g) * 0.1, torch.rand(c, generator=g) * 1.5 + 0.5


def activations(shape, seed):
    """pre-norm activations: N(0.7, 2^2) rounded to fp16"""
    return rand16(shape, seed, 2.0, 0.7)


def gradients(shape, seed):
    """output gradients carrying LOSS_SCALE: N(0, 0.05^2) * 16, fp16"""
    return (rand16(shape, 5000 + int(seed), 0.05).float() * LOSS_SCALE).half()


# ------------------------------------------------------------------------------------------------ case tables
# A / B: GroupNorm over segments, (name, n, groups, seg_hw, seed)
GN_SEG_CASES = [
    ('pyramid', 3, 16, [1920, 480, 120, 30, 9, 1], 11),     # largest segment at the 64-block cap: threads loop
    ('block_edges', 2, 4, [257, 64, 1], 12),                # 1028 vectors = 4 blocks + 4 vectors; exactly one block; 4 vectors
    ('cap_binds', 70, 32, [240, 7], 13),                    # 4096 / 140 = 29 blocks where 7680 vectors would want 30; c = 256
    ('max_levels', 1, 16, [1, 2, 3, 5, 8, 13, 21, 34], 14),
    ('one_group', 2, 1, [5], 15),
]
# C / D: BatchNorm into / from a level-concatenated tensor
BN_LEVELS = [(7, 9), (4, 5), (2, 3), (1, 1)]
BN_GAP_AFTER_FIRST, BN_TAIL_ROWS = 5, 3
BN_LEVEL_N = 3
BN_PARTIALS_CIN, BN_PARTIALS_COUT = [64, 128, 128, 128], 128          # 1x1 stride-1 tap convs of the neck
BN_INTO_CASES = [(c, relu) for c in (64, 128) for relu in (True, False)]
# E: the plain kernels at the channel / group counts channels_ok / gn_ok admit and nothing ran.
# (name, (n, h, w, c), mode): mode 'z' = ReLU mask from the stored z, 'y' = recomputed from y, 'res' = residual + want_g, 'none'
BN_PLAIN_CASES = [
    ('c8_one_pixel', (1, 1, 1, 8), 'none'),
    ('c8_two_pixels', (2, 1, 1, 8), 'z'),
    ('c8_255', (1, 5, 51, 8), 'z'),
    ('c8_256', (2, 8, 16, 8), 'y'),
    ('c8_257', (1, 1, 257, 8), 'none'),
    ('c16', (2, 5, 3, 16), 'z'),
    ('c256', (3, 7, 9, 256), 'z'),
    ('c256_residual', (2, 6, 5, 256), 'res'),
    ('above_grid_cap', (1, 129, 128, 128), 'z'),            # 264 192 vectors > 1024 * 256
]
GN_PLAIN_CASES = [('g1', (2, 5, 3, 8)), ('g2', (3, 17, 13, 16)), ('g32', (2, 9, 7, 256)), ('g1_one_pixel', (2, 1, 1, 8))]
# F: accuracy of the statistics against mean / std
ACCURACY_RATIOS_ASSERTED, ACCURACY_RATIOS_PRINTED = (0.25, 2.0), (4.0, 16.0, 64.0)
ACCURACY_BN_SHAPES = [(3, 33, 47, 64), (2, 5, 3, 64)]
ACCURACY_GN_CASE = 'block_edges'


def gn_seg_case(name):
    return next(c for c in GN_SEG_CASES if c[0] == name)


def bn_level_starts(levels=BN_LEVELS):
    """-> (first row of every level, rows per image): a 5-row gap behind the first level, 3 unused rows at the end"""
    starts, p = [], 0
    for i, (h, w) in enumerate(levels):
        starts.append(p)
        p += h * w + (BN_GAP_AFTER_FIRST if i == 0 else 0)
    return starts, p + BN_TAIL_ROWS


def accuracy_input(shape, ratio, seed=77):
    """N(ratio, 1) rounded to fp16: mean / std = ratio"""
    return rand16(shape, seed, 1.0, ratio)


# ------------------------------------------------------------------------------------------------ launch geometry
def bn_chain(m, c):
    """longest fp32 addition chain of the BatchNorm reductions over [m, c]: vectors per thread + the block reduce"""
    vecs = m * (c // 8)
    blocks = min(max(-(-vecs // THREADS), 1), BN_MAX_BLOCKS)
    return -(-vecs // (blocks * THREADS)) + THREADS // (c // 8)


def gn_blocks(max_vecs, nvirt):
    cap = min(max(4096 // max(nvirt, 1), 1), 64)
    return min(max(-(-max_vecs // THREADS), 1), cap)


def gn_chain(n, seg_hw, groups):
    """the same for the GroupNorm reductions: a thread adds the 8 channels of every vector it owns into one accumulator"""
    max_vecs = max(seg_hw) * groups
    blocks = gn_blocks(max_vecs, n * len(seg_hw))
    return 8 * -(-max_vecs // (blocks * THREADS)) + THREADS // groups


# ------------------------------------------------------------------------------------------------ error bounds
def store_bound(ref, operands):
    """|got - ref| for a value stored as fp16: u16 |ref| + 2^-24 for the store (half an ulp of the smallest subnormal), plus
    2^-21 * sum|operands| for the fp32 expression in front of it (at most six roundings of u32 each, relative to the operand
    magnitudes, rounded up to a power of two)"""
    return U16 * ref.abs() + 2.0 ** -24 + 2.0 ** -21 * operands


def sum_bound(chain, abs_terms, term_roundings=0):
    """|delta| of an fp32 sum: chain * u32 * sum|terms|; term_roundings = fp32 roundings inside every term before it is added"""
    return (chain + term_roundings) * U32 * abs_terms


def f32_out_bound(ref, prev=None):
    """a float64 value rounded to fp32, (+= onto `prev` in fp32)"""
    b = U32 * ref.abs()
    return b if prev is None else b + U32 * (ref.abs() + abs(prev))


def undecided(pre, terms):
    """elements whose recomputed ReLU mask [gamma * xhat + beta > 0] the mathematics does not decide: |pre| <= 2^-20 * terms,
    terms = |gamma * xhat| + |beta| (four fp32 roundings in the kernel's expression, with a margin of four)"""
    return pre.abs() <= 2.0 ** -20 * terms


# ------------------------------------------------------------------------------------------------ BatchNorm, float64
def bn_forward_ref(y, eps=EPS, momentum=MOMENTUM, running_mean=None, running_var=None):
    """y [m, c] -> dict(mean, var (biased), rstd, running_mean, running_var), float64.  One value per channel (m == 1) follows
    bn_stats_final_body: variance 0, rstd = 1 / sqrt(eps), running_var blended with the BIASED variance (torch refuses m == 1)."""
    yd = y.double()
    m = yd.size(0)
    mean = yd.sum(0) / m
    var = ((yd - mean) ** 2).sum(0) / m
    out = dict(mean=mean, var=var, rstd=1.0 / torch.sqrt(var + eps))
    if running_mean is not None:
        unb = var * m / (m - 1) if m > 1 else var
        out['running_mean'] = (1 - momentum) * running_mean.double() + momentum * mean
        out['running_var'] = (1 - momentum) * running_var.double() + momentum * unb
    return out


def split_stats(stats):
    """float32[2 * c] as the kernels return it -> (mean, rstd) float64"""
    c = stats.numel() // 2
    return stats[:c].double(), stats[c:].double()


def bn_apply_ref(y, stats, gamma, beta, res=None, relu=True):
    """-> (z, operands, pre, terms): z = relu?(gamma * xhat + beta (+ res)) from `stats`; operands = sum of the magnitudes the
    kernel's expression y * a + (beta - mean * a) (+ res) adds; pre / terms for undecided()"""
    mean, rstd = split_stats(stats)
    a = gamma.double() * rstd
    yd = y.double()
    pre = a * (yd - mean) + beta.double()
    operands = (yd * a).abs() + (mean * a).abs() + beta.double().abs()
    z = pre
    if res is not None:
        z = z + res.double()
        operands = operands + res.double().abs()
    if relu:
        z = z.clamp_min(0.0)
    return z, operands, pre, (a * (yd - mean)).abs() + beta.double().abs()


def bn_backward_ref(dz, y, mask, stats, gamma, inv_scale):
    """g = dz * mask; dbeta = sum g * inv_scale; dgamma = sum g xhat * inv_scale; dy = gamma rstd (g - mean(g) - xhat mean(g xhat)).
    dz, y [m, c]; mask: bool [m, c] or None.  -> dict with the results and the sums of magnitudes the bounds need."""
    mean, rstd = split_stats(stats)
    yd, m = y.double(), y.size(0)
    g = dz.double() if mask is None else dz.double() * mask
    xh = (yd - mean) * rstd
    s0, s1 = g.sum(0), (g * xh).sum(0)
    a = gamma.double() * rstd
    return dict(g=g, xh=xh, a=a, m=m, s0=s0, s1=s1, abs0=g.abs().sum(0), abs1=(g * xh).abs().sum(0),
                dbeta=s0 * inv_scale, dgamma=s1 * inv_scale, dy=a * (g - s0 / m - xh * (s1 / m)))


def bn_backward_bounds(r, chain, inv_scale, prev_dgamma=None, prev_dbeta=None):
    """-> (dy, dgamma, dbeta) bounds for bn_backward_ref's result `r`.  The sums: chain (+ 3 roundings inside a g * xhat term:
    y - mean, * rstd, * g) in fp32, then fp64; each leaves the final pass rounded to fp32 (u32) and is multiplied by 1 / m in
    fp32 (2 u32: the reciprocal and the product)."""
    d0, d1 = sum_bound(chain, r['abs0']), sum_bound(chain, r['abs1'], 3)
    m = r['m']
    dm0, dm1 = (d0 + 3 * U32 * r['s0'].abs()) / m, (d1 + 3 * U32 * r['s1'].abs()) / m
    a, xh = r['a'].abs(), r['xh'].abs()
    operands = a * (r['g'].abs() + (r['s0'] / m).abs() + xh * (r['s1'] / m).abs())
    dy = store_bound(r['dy'], operands) + a * (dm0 + xh * dm1)
    return (dy, d1 * inv_scale + f32_out_bound(r['dgamma'], prev_dgamma), d0 * inv_scale + f32_out_bound(r['dbeta'], prev_dbeta))


# ------------------------------------------------------------------------------------------------ GroupNorm, float64
def _seg_bounds(seg_hw):
    o = 0
    for hw in seg_hw:
        yield o, o + hw
        o += hw


def seg_group_sum(t, seg_hw, groups):
    """t [n, P, c] float64 -> sums over (pixels of the segment, 8 channels of the group): [n, nseg, groups]"""
    n = t.size(0)
    return torch.stack([t[:, a:b].reshape(n, b - a, groups, 8).sum((1, 3)) for a, b in _seg_bounds(seg_hw)], 1)


def seg_group_expand(v, seg_hw):
    """v [n, nseg, groups] -> [n, P, 8 * groups]"""
    return torch.cat([v[:, s, None, :].expand(-1, hw, -1) for s, hw in enumerate(seg_hw)], 1).repeat_interleave(8, 2)


def seg_counts(seg_hw):
    return torch.tensor([8.0 * hw for hw in seg_hw], dtype=torch.float64)[None, :, None]


def gn_forward_ref(y, seg_hw, groups, eps=EPS):
    """y [n, P, c] -> stats [n, nseg, 2, groups] float64 (mean, rstd with the biased variance) per (image, segment, group)"""
    yd = y.double()
    cnt = seg_counts(seg_hw)
    mean = seg_group_sum(yd, seg_hw, groups) / cnt
    var = seg_group_sum((yd - seg_group_expand(mean, seg_hw)) ** 2, seg_hw, groups) / cnt
    return torch.stack([mean, 1.0 / torch.sqrt(var + eps)], 2)


def gn_stats_view(stats, n, nseg, groups):
    """float32[n * nseg * 2 * groups] as the kernels return it -> float64 [n, nseg, 2, groups]"""
    return stats.double().reshape(n, nseg, 2, groups)


def gn_apply_ref(y, seg_hw, groups, stats, gamma, beta, relu=True):
    """stats [n, nseg, 2, groups] float64 -> (z, operands) as bn_apply_ref"""
    mean, rstd = seg_group_expand(stats[:, :, 0], seg_hw), seg_group_expand(stats[:, :, 1], seg_hw)
    a = gamma.double() * rstd
    yd = y.double()
    z = a * (yd - mean) + beta.double()
    operands = (yd * a).abs() + (mean * a).abs() + beta.double().abs()
    return (z.clamp_min(0.0) if relu else z), operands


def gn_backward_ref(dz, y, mask, seg_hw, groups, stats, gamma, inv_scale):
    """per (image, segment, group): m1 = mean(g gamma), m2 = mean(g gamma xhat), dy = rstd (g gamma - m1 - xhat m2);
    dgamma = sum g xhat, dbeta = sum g over ALL images and segments, times inv_scale.  mask: bool [n, P, c] or None."""
    mean, rstd = seg_group_expand(stats[:, :, 0], seg_hw), seg_group_expand(stats[:, :, 1], seg_hw)
    g = dz.double() if mask is None else dz.double() * mask
    xh = (y.double() - mean) * rstd
    gg = g * gamma.double()
    cnt = seg_counts(seg_hw)
    s1, s2 = seg_group_sum(gg, seg_hw, groups), seg_group_sum(gg * xh, seg_hw, groups)
    m1, m2 = seg_group_expand(s1 / cnt, seg_hw), seg_group_expand(s2 / cnt, seg_hw)
    return dict(gg=gg, xh=xh, rstd=rstd, cnt=cnt, s1=s1, s2=s2, m1=m1, m2=m2,
                abs1=seg_group_sum(gg.abs(), seg_hw, groups), abs2=seg_group_sum((gg * xh).abs(), seg_hw, groups),
                dy=rstd * (gg - m1 - xh * m2), dgamma=(g * xh).sum((0, 1)) * inv_scale, dbeta=g.sum((0, 1)) * inv_scale,
                absg=(g * xh).abs().sum((0, 1)), absb=g.abs().sum((0, 1)))


def gn_backward_bounds(r, seg_hw, chain, inv_scale, prev_dgamma=None, prev_dbeta=None):
    """-> (dy, dgamma, dbeta) bounds.  Terms: g gamma (1 rounding), g gamma xhat (4: y - mean, * rstd, g * gamma, * xhat),
    g xhat (3); the group sums leave the final pass as fp32 and are multiplied by 1 / m in fp32 (3 u32, as for BatchNorm)."""
    d1, d2 = sum_bound(chain, r['abs1'], 1), sum_bound(chain, r['abs2'], 4)
    dm1 = seg_group_expand((d1 + 3 * U32 * r['s1'].abs()) / r['cnt'], seg_hw)
    dm2 = seg_group_expand((d2 + 3 * U32 * r['s2'].abs()) / r['cnt'], seg_hw)
    rstd, xh = r['rstd'].abs(), r['xh'].abs()
    operands = rstd * (r['gg'].abs() + r['m1'].abs() + xh * r['m2'].abs())
    dy = store_bound(r['dy'], operands) + rstd * (dm1 + xh * dm2)
    return (dy, sum_bound(chain, r['absg'], 3) * inv_scale + f32_out_bound(r['dgamma'], prev_dgamma),
            sum_bound(chain, r['absb']) * inv_scale + f32_out_bound(r['dbeta'], prev_dbeta))


# ------------------------------------------------------------------------------------------------ fp32 restatement
def _apply_f32(y, a_mean, a_rstd, gamma, beta, res, relu):
    """the kernels' forward apply pass as written (-ffp-contract=off: no fma): a = gamma * rstd; b = beta - mean * a;
    f = y * a + b (+ res); max(f, 0); cast to fp16.  torch evaluates every operator on its own, in fp32."""
    a = gamma.float() * a_rstd
    b = beta.float() - a_mean * a
    f = y.float() * a + b
    if res is not None:
        f = f + res.float()
    if relu:
        f = torch.clamp_min(f, 0.0)
    return f.half()


def bn_apply_f32(y, stats, gamma, beta, res=None, relu=True):
    """y [m, c] fp16, stats float32[2 * c] -> z fp16"""
    c = stats.numel() // 2
    return _apply_f32(y, stats[:c].float(), stats[c:].float(), gamma, beta, res, relu)


def gn_apply_f32(y, seg_hw, groups, stats, gamma, beta, relu=True):
    """y [n, P, c] fp16, stats float32 [n, nseg, 2, groups] -> z fp16"""
    st = stats.float().reshape(y.size(0), len(seg_hw), 2, groups)
    return _apply_f32(y, seg_group_expand(st[:, :, 0], seg_hw), seg_group_expand(st[:, :, 1], seg_hw), gamma, beta, None, relu)


# ------------------------------------------------------------------------------------------------ seeded case inputs
@functools.lru_cache(maxsize=None)
def gn_seg_inputs(name):
    """-> dict(n, groups, seg_hw, c, y [n, P, c], dz, gamma, beta)"""
    _, n, groups, seg_hw, seed = gn_seg_case(name)
    c, p = 8 * groups, sum(seg_hw)
    gamma, beta = norm_params(c, seed)
    return dict(n=n, groups=groups, seg_hw=list(seg_hw), c=c, y=activations((n, p, c), seed), dz=gradients((n, p, c), seed),
                gamma=gamma, beta=beta)


@functools.lru_cache(maxsize=None)
def bn_level_inputs(c, n=BN_LEVEL_N, seed=31):
    """per level of BN_LEVELS: dict(y [n, h, w, c], gamma, beta, running_mean, running_var); + the seeded concatenated gradient"""
    starts, p = bn_level_starts()
    lv = []
    for l, (h, w) in enumerate(BN_LEVELS):
        gamma, beta = norm_params(c, seed + 10 * l + n)
        rm, rv = running_stats(c, seed + 10 * l + n)
        lv.append(dict(y=activations((n, h, w, c), seed + 10 * l + n + c), gamma=gamma, beta=beta, running_mean=rm, running_var=rv))
    return dict(levels=lv, starts=starts, p=p, dz=gradients((n, p, c), seed + n))


@functools.lru_cache(maxsize=None)
def bn_partials_inputs(n, seed=41):
    """the tap convs of case C: per level dict(x [n, h, w, cin], weight [128, cin, 1, 1] fp32, cin) + norm parameters"""
    lv = []
    for l, ((h, w), cin) in enumerate(zip(BN_LEVELS, BN_PARTIALS_CIN)):
        g = torch.Generator().manual_seed(seed + l)
        wt = torch.randn((BN_PARTIALS_COUT, cin, 1, 1), generator=g) * math.sqrt(2.0 / cin)
        gamma, beta = norm_params(BN_PARTIALS_COUT, seed + l)
        rm, rv = running_stats(BN_PARTIALS_COUT, seed + l)
        lv.append(dict(x=rand16((n, h, w, cin), seed + 100 + l, 1.0, 0.2), weight=wt, cin=cin, gamma=gamma, beta=beta,
                       running_mean=rm, running_var=rv))
    return lv


@functools.lru_cache(maxsize=None)
def bn_plain_inputs(name):
    _, shape, mode = next(c for c in BN_PLAIN_CASES if c[0] == name)
    seed = 50 + [c[0] for c in BN_PLAIN_CASES].index(name)
    c = shape[3]
    gamma, beta = norm_params(c, seed)
    rm, rv = running_stats(c, seed)
    return dict(shape=shape, mode=mode, c=c, y=activations(shape, seed), dz=gradients(shape, seed), gamma=gamma, beta=beta,
                running_mean=rm, running_var=rv, res=rand16(shape, 7000 + seed) if mode == 'res' else None)


@functools.lru_cache(maxsize=None)
def gn_plain_inputs(name):
    _, shape = next(c for c in GN_PLAIN_CASES if c[0] == name)
    seed = 70 + [c[0] for c in GN_PLAIN_CASES].index(name)
    n, h, w, c = shape
    gamma, beta = norm_params(c, seed)
    return dict(n=n, groups=c // 8, seg_hw=[h * w], c=c, shape=shape, y=activations((n, h * w, c), seed),
                dz=gradients((n, h * w, c), seed), gamma=gamma, beta=beta)


def recomputed_mask_cases():
    """every (y [m, c], gamma, beta) whose ReLU mask the kernels recompute from y (relu with no z): the level units of case D
    and the 'y' cases of E"""
    out = []
    for l, lv in enumerate(bn_level_inputs(128)['levels']):
        out.append(('levels[%d]' % l, lv['y'].reshape(-1, 128), lv['gamma'], lv['beta']))
    for name, _, mode in BN_PLAIN_CASES:
        if mode == 'y':
            d = bn_plain_inputs(name)
            out.append((name, d['y'].reshape(-1, d['c']), d['gamma'], d['beta']))
    return out
