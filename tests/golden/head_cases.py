"""Instrument of tests/test_gpu_head_exact.py (checked on the CPU by tests/test_head_reference_host.py): the fp16 neck + shared
detection head of csrc/head.hip -- k_head, k_head2, k_gn_finalize -- one kernel family at a time, through the C ABI.

  * `operands`   seeded tensors of a case on one of two instruments: 'int' (integer operands for which every fp16 rounding point and
                 every fp32 accumulation of the chain is exact) and 'gauss' (scaled so that every stage has about unit variance);
  * `chain`      the chain  neck -> conv1 -> GroupNorm+ReLU -> conv2 -> GroupNorm+ReLU -> final conv  in float64 (the reference), or in
                 float32 with a shuffled K order (the emulations the gates come from), in either kernel's arithmetic (`form`), and
                 wrong in exactly one way (`wrong`) for the checks that the comparison resolves the bugs it is meant to catch;
  * `walk_head2` / `walk_head`  the launch geometry restated from the source: which block and wave works on which (level, image, pixel
                 groups / tile) in which iteration; tests/test_head_reference_host.py compares the restated constants with head.hip;
  * `Device`     the driver: guarded device buffers of a case and the five launches over lfd_head_forward_f16 /
                 lfd_groupnorm_finalize[_fold] / lfd_head_forward_decode_f16;
  * the case tables and the gates."""
import ctypes as C

import torch

HC, TPX, GPX = 128, 64, 32       # head channels; pixels per statistics tile; pixels per k_head2 group
H2_CH = 12                       # longest k_head2 chunk, in groups
H2_SLOTS = 2048                  # h2_plan_chunks: about one chunk per resident wave
H2_ITEM_CHUNKS = 4               # k_head2 work item = 4 consecutive chunks of a level, one per wave
H2_BLOCKS = 256                  # launch_head2: blocks = min(items, 256), strided walk
HEAD_BLOCKS = 512                # launch_head: grid = min(tiles, 512), contiguous ranges of ceil(tiles / grid)
RING = {64: 4, 128: 2}           # k_head input ring depth per tap channel count
EPS = 1e-5
GAP = 3                          # guard rows between the levels of cls / reg (and behind the last one)

# Gates, per kernel form and quantity: 4 x the largest deviation |d| / max(|ref|, 1) from the float64 reference of the float32
# emulations of that form (two K orders) over every Gaussian case, rounded up by at most a tenth -- derived on the CPU, not read off
# the kernels: tests/test_head_reference_host.py re-derives the figures and fails when an emulation exceeds a quarter of its gate (or
# falls below an eighth).  The margin covers MFMA's internal summation order and fp16 roundings that flip at a stage boundary.
# k_head2 rounds every filter row once more, as fp16(w a): its second-pass statistics and outputs sit further from float64 than
# k_head's, by design.  Emulation figures and the errors measured on the MI355X: DESIGN.md 4f.
GATES = {
    'head': dict(partial1=7.5e-3, partial2=7.5e-3, ab1=2.8e-5, ab2=1.2e-4, cls=6e-3, reg=1e-2),
    'head2': dict(partial1=8e-3, partial2=0.23, ab1=2.6e-5, ab2=2.7e-3, cls=1.25e-2, reg=1.8e-2),
}


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def rt16(t):
    """the values an fp16 store keeps"""
    return t.float().half().to(t.dtype)


def hilo(v):
    """a bias on k_head2's extra MFMA k-step: fp16 hi + fp16 lo of the fp32 value"""
    v = v.float()
    hi = v.half()
    lo = (v - hi.float()).half()
    return hi.double() + lo.double(), hi.double()


# ------------------------------------------------------------------------------------------------ cases
def case(name, n, levels, groups=16, rows=(4, 1), scale=True, chunk=0, contiguous=False, seed=0, gauss=True):
    return dict(name=name, n=n, levels=list(levels), groups=groups, reg_rows=rows[0], cls_rows=rows[1], scale=scale, chunk=chunk,
                contiguous=contiguous, seed=seed, gauss=gauss)


def _tiles(k):
    """a level of k statistics tiles whose last tile holds one pixel"""
    return 64 * (k - 1) + 1


# k_head2 (and, under tune('HEAD2', 0), k_head): every level size, batch 1 and 3, taps of 64 and 128 channels, every layout of the
# final rows.  `chunk`: forced H2_CHUNK (0 = planned).
SMALL_CASES = [
    case('sizes3', 3, [(1, 64), (31, 64), (32, 128), (33, 64), (63, 128), (64, 64), (65, 128), (96, 64)], seed=1),
    case('sizes1', 1, [(127, 64), (510, 64), (96, 128), (510, 128)], rows=(4, 28), seed=2),
    case('sizes1_c4', 1, [(127, 64), (510, 64), (96, 128), (510, 128)], rows=(4, 28), chunk=4, seed=2),
    case('sizes1_c12', 1, [(127, 64), (510, 64), (96, 128), (510, 128)], rows=(4, 28), chunk=12, seed=2),
    case('g8_ft2', 3, [(510, 64), (127, 128)], groups=8, rows=(4, 29), seed=3),
    case('g4_cls', 1, [(65, 64), (1, 128)], groups=4, rows=(0, 5), scale=False, seed=4),
    case('ft2_full', 3, [(96, 64), (33, 128)], rows=(4, 60), scale=False, seed=5),
    case('cls33', 1, [(63, 64), (31, 128)], rows=(0, 33), scale=False, seed=6),
    case('reg_only', 3, [(31, 128), (64, 64)], rows=(4, 0), seed=7),
    case('dec', 3, [(17 * 30, 64), (9 * 15, 64), (5 * 8, 128), (3 * 4, 128)], contiguous=True, seed=8),
]
# k_head2's strided walk: some block runs three items (items > 2 x 256) with 2-group chunks; the planned chunk length is 6 here
WALK_CASES = [
    case('walk_c2', 3, [(1368 * 32 + 5, 64)], chunk=2, seed=9),
    case('walk_plan', 3, [(1368 * 32 + 5, 64)], chunk=0, seed=9, gauss=False),
    # more items than blocks over levels (64, 64, 128, 128): a workgroup switches level, and neck K length, inside its walk
    case('switch', 1, [(33253, 64), (33253, 64), (17893, 128), (17893, 128)], chunk=2, seed=19),
]
# k_head only (groups of fewer than 8 channels: the atomic statistics path), no knob involved
ATOMIC_CASES = [
    case('g32', 3, [(96, 64), (65, 128)], groups=32, seed=10),
    case('g64', 1, [(130, 64), (33, 128)], groups=64, rows=(4, 28), seed=11),
    case('g128', 3, [(65, 64), (33, 128)], groups=128, rows=(0, 5), scale=False, seed=12),
]
# k_head's contiguous ranges against its ring: `per` tiles per block, 1..6 on the 4-deep ring (64 channels), 1..3 on the 2-deep one
RING_CASES = [
    case('ring_per1', 2, [(_tiles(2), 64), (_tiles(3) + 32, 64), (_tiles(2), 128), (_tiles(3) + 32, 128)], seed=13),
    case('ring_per2', 3, [(_tiles(85), 64), (_tiles(86) + 32, 64), (_tiles(85), 128), (_tiles(86) + 32, 128)], seed=14),
    case('ring_per3', 2, [(_tiles(257), 64), (_tiles(257) + 32, 64), (_tiles(257), 128), (_tiles(257) + 32, 128)], seed=15, gauss=False),
    case('ring_per4', 3, [(_tiles(257), 64), (_tiles(256) + 32, 64)], seed=16, gauss=False),
    case('ring_per5', 3, [(_tiles(341), 64), (_tiles(342) + 32, 64)], seed=17, gauss=False),
    case('ring_per6', 3, [(_tiles(427), 64), (_tiles(428) + 32, 64)], seed=18, gauss=False),
]
RING_PER = {'ring_per1': (1, 1), 'ring_per2': (2, 2), 'ring_per3': (3, 3), 'ring_per4': (4, None), 'ring_per5': (5, None),
            'ring_per6': (6, None)}
H2_CASES = SMALL_CASES + WALK_CASES                  # cases k_head2 runs
HEAD_CASES = SMALL_CASES + ATOMIC_CASES + RING_CASES  # cases k_head runs (HEAD2 = 0 for groups <= 16)
ALL_CASES = SMALL_CASES + WALK_CASES + ATOMIC_CASES + RING_CASES
BY_NAME = dict((c['name'], c) for c in ALL_CASES)
# k_head2 variants: (K-permuted filter copies, folded filters, tower-1 activations handed to the output pass, knobs)
VARIANTS = {
    'plain': dict(perm=False, fold=False, a1=False, knobs={}),
    'perm': dict(perm=True, fold=False, a1=False, knobs={}),
    'fold': dict(perm=True, fold=True, a1=False, knobs={}),
    'fold_agpr0': dict(perm=True, fold=True, a1=False, knobs={'H2_AGPR': 0}),
    'fold_a1': dict(perm=True, fold=True, a1=True, knobs={}),
    'fold_a1_off': dict(perm=True, fold=True, a1=True, knobs={'H2_A1': 0}),
}
KNOB_DEFAULTS = {'HEAD2': 1, 'H2_CHUNK': 0, 'H2_AGPR': 1, 'H2_A1': 1}


def uses_head2(c, head2=1):
    """the dispatch of head_forward_impl: k_head2 needs the knob and groups of at least 8 channels"""
    return bool(head2) and HC // c['groups'] >= 8


def final_tiles(c):
    return (c['reg_rows'] + c['cls_rows'] + 31) // 32


def geometry(c):
    """tiles, point offsets (with GAP guard rows unless the case asks for contiguous offsets) and buffer sizes"""
    n, tpi, tstart, poff, t, p = c['n'], [], [], [], 0, 0
    gap = 0 if c['contiguous'] else GAP
    for hw, _ in c['levels']:
        tpi.append((hw + TPX - 1) // TPX)
        tstart.append(t)
        t += tpi[-1] * n
        poff.append(p)
        p += hw + gap
    return dict(tpi=tpi, tile_start=tstart, ntiles=t, p_off=poff, P=p, cc=max(c['cls_rows'], 1))


# ------------------------------------------------------------------------------------------------ operands
def _sparse(g, rows, cols, nnz):
    w = torch.zeros(rows, cols)
    for r in range(rows):
        idx = torch.randperm(cols, generator=g)[:nnz]
        w[r, idx] = torch.randint(0, 2, (nnz,), generator=g).float() * 2 - 1
    return w


def operands(c, kind):
    """per level: x [n, hw, cin], wn, bn, w1, w2, wf [rows, 128], bf, scale, gamma / beta of both norms; kind 'int' also carries the
    supplied (a, b) of both norms, [L, n, 128, 2] fp32: a in {1/2, 1, 2}, b integer, different for every (level, image).
    Every filter and activation is an fp16 value; biases, gamma, beta, Scale are fp32 values."""
    g = _gen(1000 * c['seed'] + (1 if kind == 'int' else 2))
    n, rows, L = c['n'], c['reg_rows'] + c['cls_rows'], []
    for hw, cin in c['levels']:
        o = {}
        if kind == 'int':
            o['x'] = torch.randint(0, 3, (n, hw, cin), generator=g).float()
            o['wn'], o['bn'] = _sparse(g, HC, cin, 4), torch.randint(-2, 3, (HC,), generator=g).float()
            o['w1'], o['w2'], o['wf'] = _sparse(g, HC, HC, 6), _sparse(g, HC, HC, 6), _sparse(g, rows, HC, 6)
            # |bf| up to 3000: the odd values above 2048 need the lo half of the bias k-step
            o['bf'] = torch.randint(-3000, 3001, (rows,), generator=g).float()
            o['bf'][0], o['bf'][-1] = 2049.0, -2051.0
            o['scale'] = 0.5 if c['scale'] else None
        else:
            o['x'] = torch.randn(n, hw, cin, generator=g).half().float()
            o['wn'] = (torch.randn(HC, cin, generator=g) * (2.0 / cin) ** 0.5).half().float()
            o['bn'] = torch.randn(HC, generator=g) * 0.1
            o['w1'] = (torch.randn(HC, HC, generator=g) * (2.0 / HC) ** 0.5).half().float()
            o['w2'] = (torch.randn(HC, HC, generator=g) * (2.0 / HC) ** 0.5).half().float()
            o['wf'] = (torch.randn(rows, HC, generator=g) * (2.0 / HC) ** 0.5).half().float()
            o['bf'] = torch.randn(rows, generator=g) * 0.5
            o['scale'] = 1.37 if c['scale'] else None
        for k in ('1', '2'):
            o['gamma' + k] = 1 + 0.1 * torch.randn(HC, generator=g)
            o['beta' + k] = 0.1 * torch.randn(HC, generator=g)
        L.append(o)
    out = dict(levels=L, kind=kind)
    if kind == 'int':
        ab = torch.empty(2, len(L), n, HC, 2)
        ab[..., 0] = 2.0 ** torch.randint(-1, 2, (2, len(L), n, HC), generator=g).float()
        ab[..., 1] = torch.randint(-3, 4, (2, len(L), n, HC), generator=g).float()
        out['ab'] = ab
    return out


def unpermuted_k(w):
    """[M, 128] filter as the MFMAs see it when K-permuted fragments are consumed in the standard order (or the other way round):
    within every k-step of 16, element 8a + 4b + c <-> 8b + 4a + c (csrc/head.hip `perm`, engine._perm_head_weight)"""
    return w.view(w.shape[0], HC // 16, 2, 2, 4).transpose(2, 3).reshape(w.shape[0], HC).contiguous()


# ------------------------------------------------------------------------------------------------ the chain
WRONG = ('drop_last_group', 'stats_full_tiles', 'next_image_ab', 'unpermuted_k', 'bias_lo_dropped', 'reg_unscaled', 'cls_shifted')


def chain(c, O, form='head', dtype=torch.float64, kseed=None, ab=None, wrong=None, wrong_ranges=(), caps=False, round16=True):
    """The chain of one case.  form 'head': (a, b) applied to the accumulator, fp32 biases (k_head); 'head2': filter rows rounded once
    as fp16(fp32(w) * a), shift and biases as fp16 hi + lo (k_head2).  dtype float64: the reference ((a, b) stay float64 in form
    'head'); float32: an emulation -- K shuffled by `kseed`, float32 accumulation over k-steps of 16, float32 tile sums, (a, b)
    rounded to fp32.  ab: supplied [2, L, n, 128, 2] instead of the chain's own statistics.  wrong: one of WRONG; wrong_ranges: (level, image, first
    pixel, end pixel) that take the next image's (a, b) under 'next_image_ab'.
    Returns partial1 / partial2 [tiles, groups, 2], ab1 / ab2 [L, n, 128, 2], cls [n, P, cc], reg [n, P, 4] (NaN outside the levels),
    all float64; with caps=True also 'round_err' (largest change at an fp16 rounding point) and 'cap' (largest bound on a partial
    sum, in units of the value grid of its stage: the exactness conditions of the integer instrument)."""
    G, n, geo = c['groups'], c['n'], geometry(c)
    gs, rr, cr = HC // G, c['reg_rows'], c['cls_rows']
    emu = dtype == torch.float32
    res = dict(partial1=torch.zeros(geo['ntiles'], G, 2, dtype=torch.float64), partial2=torch.zeros(geo['ntiles'], G, 2, dtype=torch.float64),
               ab1=torch.zeros(len(c['levels']), n, HC, 2, dtype=torch.float64), ab2=torch.zeros(len(c['levels']), n, HC, 2, dtype=torch.float64),
               cls=torch.full((n, geo['P'], geo['cc']), float('nan'), dtype=torch.float64),
               reg=torch.full((n, geo['P'], 4), float('nan'), dtype=torch.float64), round_err=0.0, cap=0.0)
    kg = _gen(kseed) if kseed is not None else None
    lo_i = 1 if wrong == 'bias_lo_dropped' else 0

    def mm(t, w, grid=1.0):
        if caps:
            res['cap'] = max(res['cap'], float((t.double().abs() @ w.double().abs().t()).max()) / grid)
        if kg is not None:
            p = torch.randperm(w.shape[1], generator=kg)
            t, w = t[..., p], w[:, p]
        if not emu:
            return t.double() @ w.double().t()
        # float32 the way an MFMA chain accumulates, and the same on every host: k-steps of 16 products, each step's sum added to the
        # float32 accumulator with one rounding (a library float32 matmul would sum in an order that depends on the machine)
        acc = torch.zeros(t.shape[:-1] + (w.shape[0],), dtype=torch.float32)
        for q in range(0, w.shape[1], 16):
            acc = (acc.double() + t[..., q:q + 16].double() @ w[:, q:q + 16].double().t()).float()
        return acc

    def bias(v):
        return (hilo(v)[lo_i] if form == 'head2' else v.double()).to(dtype)

    def store16(t):
        r = rt16(t.relu()) if round16 else t.relu()
        if caps:
            res['round_err'] = max(res['round_err'], float((r - t.relu()).abs().max()))
        return r.to(dtype)

    def norm(cv, w_next, abv):
        """ReLU(GroupNorm(c)) as conv `w_next` produced it, for one image: cv = the raw conv output (form 'head') or its input t
        (form 'head2', where the conv is redone with the folded filter)"""
        a, b = abv[:, 0], abv[:, 1]
        if form == 'head2':
            wf_ = (w_next.float() * a.float()[:, None]).half().double()
            return store16(mm(cv, wf_, 0.25) + bias(b))
        return store16(cv * a.to(dtype) + b.to(dtype))

    def stats(cv, l, hw, pad_value, grid):
        """per tile and group (sum, sum of squares) of cv [n, hw, 128] in the layout of the partial buffer"""
        tpi = geo['tpi'][l]
        v = torch.zeros(n, tpi * TPX, HC, dtype=dtype)
        v[:, :hw] = cv
        if wrong == 'drop_last_group' and hw % GPX:
            v[:, hw - hw % GPX:] = 0
        if wrong == 'stats_full_tiles':
            v[:, hw:] = pad_value
        v = v.view(n, tpi, TPX, G, gs)
        s = torch.stack([v.sum((2, 4)), (v * v).sum((2, 4))], -1).double()              # [n, tpi, G, 2]
        if caps:
            res['cap'] = max(res['cap'], float(v.abs().sum((2, 4)).max()) / grid, float(s[..., 1].max()) / grid ** 2)
        return s

    def affine(s, l, hw, gamma, beta):
        cnt = float((geo['tpi'][l] * TPX if wrong == 'stats_full_tiles' else hw) * gs)
        tot = s.sum(1)                                                                 # [n, G, 2]
        mean = tot[..., 0] / cnt
        var = (tot[..., 1] / cnt - mean * mean).clamp(min=0)
        rstd = 1.0 / (var + EPS).sqrt()
        a = gamma.double()[None] * rstd.repeat_interleave(gs, 1)
        b = beta.double()[None] - mean.repeat_interleave(gs, 1) * a
        out = torch.stack([a, b], -1)
        return out.float().double() if (emu or form == 'head2') else out

    for l, ((hw, cin), o) in enumerate(zip(c['levels'], O['levels'])):
        w2 = unpermuted_k(o['w2']) if wrong == 'unpermuted_k' else o['w2']
        t0 = store16(mm(o['x'], o['wn']) + bias(o['bn']))
        c1 = mm(t0, o['w1'])
        pad1 = mm(store16(bias(o['bn'])[None]), o['w1'])[0] if wrong == 'stats_full_tiles' else 0
        s1 = stats(c1, l, hw, pad1, 1.0)
        ts = geo['tile_start'][l]
        res['partial1'][ts:ts + n * geo['tpi'][l]] = s1.reshape(-1, G, 2)
        res['ab1'][l] = affine(s1, l, hw, o['gamma1'], o['beta1'])
        ab1 = ab[0, l].double() if ab is not None else res['ab1'][l]
        src1 = t0 if form == 'head2' else c1

        def tower1(i, j, p0=0, p1=hw):      # image i with the (a, b) of image j
            return norm(src1[i, p0:p1], o['w1'], ab1[j])
        t1 = torch.stack([tower1(i, i) for i in range(n)])
        if wrong == 'next_image_ab':
            for (wl, wi, p0, p1) in wrong_ranges:
                if wl == l:
                    t1[wi, p0:p1] = tower1(wi, wi + 1, p0, p1)
        c2 = mm(t1, w2, 0.5)
        if wrong == 'stats_full_tiles':
            pt0 = store16(bias(o['bn'])[None])
            pad2 = mm(norm(pt0 if form == 'head2' else mm(pt0, o['w1']), o['w1'], ab1[0]), w2)[0]
        else:
            pad2 = 0
        s2 = stats(c2, l, hw, pad2, 0.5)
        res['partial2'][ts:ts + n * geo['tpi'][l]] = s2.reshape(-1, G, 2)
        res['ab2'][l] = affine(s2, l, hw, o['gamma2'], o['beta2'])
        ab2 = ab[1, l].double() if ab is not None else res['ab2'][l]
        src2 = t1 if form == 'head2' else c2

        def tower2(i, j, p0=0, p1=hw):
            return norm(src2[i, p0:p1], w2, ab2[j])
        t2 = torch.stack([tower2(i, i) for i in range(n)])
        if wrong == 'next_image_ab':
            for (wl, wi, p0, p1) in wrong_ranges:
                if wl == l:
                    t2[wi, p0:p1] = tower2(wi, wi + 1, p0, p1)
        out = (mm(t2, o['wf'], 0.25) + bias(o['bf'])).double()
        po = geo['p_off'][l]
        if rr:
            sc = 1.0 if (o['scale'] is None or wrong == 'reg_unscaled') else float(torch.tensor(o['scale']).float())
            res['reg'][:, po:po + hw] = (out[..., :rr].to(dtype) * sc).double()
        if cr:
            cl = out[..., rr:rr + cr].clone()
            if wrong == 'cls_shifted' and rr + cr > 32:      # rows of the second tile land on channel `row`, not `row - reg_rows`
                cl[..., 32 - rr:] = float('nan')
                for r in range(32, min(rr + cr, cr)):
                    cl[..., r] = out[..., r]
            res['cls'][:, po:po + hw] = cl
    return res


def reference(c, O, ab=None):
    return chain(c, O, 'head', ab=ab)


def deviation(got, ref):
    """largest |d| / max(|ref|, 1) over the elements the reference defines"""
    m = ~torch.isnan(ref)
    if not bool(m.any()):
        return 0.0
    d = (got.double()[m] - ref[m]).abs() / ref[m].abs().clamp(min=1.0)
    return float(d.max()) if bool(torch.isfinite(d).all()) else float('inf')


def within(got, ref, gate):
    return deviation(got, ref) <= gate


def equal(got, ref):
    """bit for bit on the elements the reference defines (fp32 device values against float64)"""
    m = ~torch.isnan(ref)
    return torch.equal(got.double()[m], ref[m])


def folded_filter(w, abv):
    """k_gn_finalize's folded copy of a tower filter for one image, [4][9][64][8] fp16: k-steps 0..7 the K-permuted fragments of
    fp16(fp32(w) * a), k-step 8 the shift as fp16 hi / lo in elements 0 / 1 of the lanes of the first half (abv: [128, 2] fp32)"""
    from lfd_amd import engine, ops
    a, b = abv[:, 0].float(), abv[:, 1].float()
    ws = (w.float() * a[:, None]).half().float()
    body = engine._perm_head_weight(ops.pack_conv_weight(ws.view(HC, HC, 1, 1)))      # [4][8][64][8]
    out = torch.zeros(4, 9, 64, 8, dtype=torch.float16)
    out[:, :8] = body
    hi = b.half()
    lo = (b - hi.float()).half()
    out[:, 8, :32, 0] = hi.view(4, 32)
    out[:, 8, :32, 1] = lo.view(4, 32)
    return out


# ------------------------------------------------------------------------------------------------ geometry
def plan_chunks(n, gpis, forced=0):
    """h2_plan_chunks (one wave per SIMD): groups per chunk of every level"""
    total = sum(g * n for g in gpis)
    cc = 2 * ((total + H2_SLOTS - 1) // H2_SLOTS)
    cc = 2 if cc < 2 else min(cc, H2_CH)
    if forced >= 2:
        cc = forced & ~1
    out = []
    for g in gpis:
        cap = H2_CH if g >= 128 else (8 if g >= 32 else 4)
        out.append(cc if (forced >= 2 or cc < cap) else cap)
    return out


def walk_head2(c, forced=None):
    """k_head2: one record per (item, wave): block, iteration of the block's strided loop, level, image and pixel groups [g0, g1);
    image None = an idle wave (no chunk left in the level)"""
    forced = c['chunk'] if forced is None else forced
    n = c['n']
    gpis = [(hw + GPX - 1) // GPX for hw, _ in c['levels']]
    chg = plan_chunks(n, gpis, forced)
    items = []
    for l, (gpi, ch) in enumerate(zip(gpis, chg)):
        cpi = (gpi + ch - 1) // ch
        for local in range((cpi * n + H2_ITEM_CHUNKS - 1) // H2_ITEM_CHUNKS):
            items.append((l, local, cpi, ch, gpi))
    blocks = min(len(items), H2_BLOCKS)
    out = []
    for it, (l, local, cpi, ch, gpi) in enumerate(items):
        for w in range(H2_ITEM_CHUNKS):
            ck = local * H2_ITEM_CHUNKS + w
            rec = dict(item=it, block=it % blocks, iteration=it // blocks, wave=w, level=l, image=None, g0=0, g1=0)
            if ck < cpi * n:
                img, ci = ck // cpi, ck % cpi
                rec.update(image=img, g0=ci * ch, g1=min(ci * ch + ch, gpi))
            out.append(rec)
    return dict(records=out, nitems=len(items), blocks=blocks, chunk=chg)


def walk_head(c):
    """k_head: one launch per tap channel count; one record per tile: block, position in the block's contiguous range, ring slot, level,
    image, first pixel, global tile (the row of the partial buffer)"""
    n, geo, out = c['n'], geometry(c), {}
    for cin in (64, 128):
        tiles = []
        for l, (hw, ci) in enumerate(c['levels']):
            if ci == cin:
                for img in range(n):
                    for t in range(geo['tpi'][l]):
                        tiles.append((l, img, t * TPX, geo['tile_start'][l] + img * geo['tpi'][l] + t))
        if not tiles:
            continue
        grid = min(len(tiles), HEAD_BLOCKS)
        per = (len(tiles) + grid - 1) // grid
        recs = []
        for u, (l, img, p0, tg) in enumerate(tiles):
            recs.append(dict(block=u // per, pos=u % per, slot=(u % per) % RING[cin], level=l, image=img, p0=p0, tile=tg,
                             tail=p0 + TPX > c['levels'][l][0]))
        out[cin] = dict(records=recs, grid=grid, per=per, ntiles=len(tiles))
    return out


def straddling_ranges(c):
    """pixel ranges (level, image, p0, p1) of the waves of a k_head2 item whose later waves are on the next image"""
    out = []
    w = walk_head2(c)
    by_item = {}
    for r in w['records']:
        by_item.setdefault(r['item'], []).append(r)
    for recs in by_item.values():
        imgs = [r['image'] for r in recs if r['image'] is not None]
        if len(set(imgs)) > 1:
            for r in recs:
                if r['image'] == min(imgs):
                    hw = c['levels'][r['level']][0]
                    out.append((r['level'], r['image'], r['g0'] * GPX, min(r['g1'] * GPX, hw)))
    return out


# ------------------------------------------------------------------------------------------------ the driver
GUARD = 64


class Guarded(object):
    """a device tensor inside a NaN-filled buffer, GUARD elements in front and behind"""

    def __init__(self, shape, dtype, values=None):
        self.shape, self.numel = tuple(shape), 1
        for s in shape:
            self.numel *= s
        self.buf = torch.full((2 * GUARD + self.numel,), float('nan'), dtype=dtype, device='cuda')
        self.t = self.buf[GUARD:GUARD + self.numel].view(self.shape)
        if values is not None:
            self.t.copy_(values.to(dtype))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def reset(self):
        self.buf.fill_(float('nan'))

    def get(self, written=True):
        b = self.buf.cpu()
        assert bool(torch.isnan(b[:GUARD]).all()) and bool(torch.isnan(b[GUARD + self.numel:]).all()), 'guard overwritten'
        out = b[GUARD:GUARD + self.numel].view(self.shape)
        if written:
            assert bool(torch.isfinite(out.float()).all()), 'unwritten or non-finite element'
        return out


class Device(object):
    """the buffers of one case on the device and the launches over them"""

    def __init__(self, c, O, variant='plain'):
        from lfd_amd import _lib, engine, ops
        self.c, self.O, self.v, self.geo = c, O, VARIANTS[variant], geometry(c)
        n, nl, geo = c['n'], len(c['levels']), self.geo
        d = _lib.HeadDesc()
        d.n, d.num_levels = n, nl
        d.head_channels, d.num_groups, d.total_points = HC, c['groups'], geo['P']
        d.cls_channels, d.final_reg_rows, d.final_cls_rows = geo['cc'], c['reg_rows'], c['cls_rows']
        self.d, self.lv = d, (_lib.HeadLevelPtrs * nl)()
        self.keep, self.x, self.folded, self.tower1 = [], [], [], []
        rows = final_tiles(c) * 32

        def dev(t):
            t = t.cuda().contiguous()
            self.keep.append(t)
            return t.data_ptr()
        for k, ((hw, cin), o) in enumerate(zip(c['levels'], O['levels'])):
            d.level_hw[k], d.level_cin[k], d.level_point_offset[k] = hw, cin, geo['p_off'][k]
            x = Guarded((n, hw, cin), torch.float16, o['x'])           # NaN behind the last pixel
            self.x.append(x)
            lv = self.lv[k]
            lv.x = x.ptr
            lv.wn_packed, lv.bn = dev(ops.pack_conv_weight(o['wn'].view(HC, cin, 1, 1))), dev(o['bn'].float())
            w1, w2 = ops.pack_conv_weight(o['w1'].view(HC, HC, 1, 1)), ops.pack_conv_weight(o['w2'].view(HC, HC, 1, 1))
            lv.w1_packed, lv.w2_packed = dev(w1), dev(w2)
            if self.v['perm']:
                lv.w1_perm, lv.w2_perm = dev(engine._perm_head_weight(w1)), dev(engine._perm_head_weight(w2))
            fw, fb = engine._pad_rows(o['wf'].view(-1, HC, 1, 1), o['bf'].float(), rows)
            lv.wf_packed, lv.bf = dev(ops.pack_conv_weight(fw)), dev(fb)
            if o['scale'] is not None:
                lv.scale = dev(torch.tensor([o['scale']], dtype=torch.float32))
            if self.v['fold']:
                f = Guarded((2, n, _lib.HEAD_FOLDED_HALFS), torch.float16)
                self.folded.append(f)
                lv.w1_folded, lv.w2_folded = f.t[0].data_ptr(), f.t[1].data_ptr()
            if self.v['a1']:
                t1 = Guarded((n, (hw + GPX - 1) // GPX, _lib.HEAD_TOWER1_GROUP_HALFS), torch.float16)
                self.tower1.append(t1)
                lv.tower1_out = t1.ptr
        self.partial_floats = int(_lib.lib().lfd_head_partial_floats(C.byref(d)))
        self.partial = Guarded((geo['ntiles'], c['groups'], 2), torch.float32)
        self.ab = [Guarded((nl, n, HC, 2), torch.float32), Guarded((nl, n, HC, 2), torch.float32)]
        self.cls = Guarded((n, geo['P'], geo['cc']), torch.float32)
        self.reg = Guarded((n, geo['P'], 4), torch.float32)
        self.gb = []
        for k in ('1', '2'):
            self.gb.append(((C.c_void_p * nl)(*[dev(o['gamma' + k].float()) for o in O['levels']]),
                            (C.c_void_p * nl)(*[dev(o['beta' + k].float()) for o in O['levels']])))
        self.zeros = ops.zero_line(torch.device('cuda', torch.cuda.current_device()))

    def set_ab(self, ab):
        """supplied (a, b) of both norms [2, L, n, 128, 2]; with folded filters, the folded copies a finalize launch would have made"""
        for k in (0, 1):
            self.ab[k].t.copy_(ab[k])
        for l, f in enumerate(self.folded):
            o = self.O['levels'][l]
            for k, w in enumerate((o['w1'], o['w2'])):
                for i in range(self.c['n']):
                    f.t[k, i].copy_(folded_filter(w, ab[k, l, i]).reshape(-1))

    def forward(self, p, d=None, lv=None, ab2=True):
        """pass p of lfd_head_forward_f16 -> status (d, lv, ab2=False: a changed descriptor / level table / no ab2, for the argument checks)"""
        from lfd_amd._lib import lib, stream_ptr
        P = C.c_void_p
        return lib().lfd_head_forward_f16(C.byref(d or self.d), p, lv or self.lv, P(self.ab[0].ptr), P(self.ab[1].ptr if ab2 else 0),
                                          P(self.partial.ptr), P(self.cls.ptr), P(self.reg.ptr), P(self.zeros.data_ptr()), stream_ptr())

    def decode(self, desc, meta, out):
        """the output pass that thresholds, decodes and appends its candidates to out.ws (lfd_head_forward_decode_f16) -> status"""
        from lfd_amd._lib import lib, stream_ptr
        P = C.c_void_p
        return lib().lfd_head_forward_decode_f16(C.byref(self.d), self.lv, P(self.ab[0].ptr), P(self.ab[1].ptr), None, None,
                                                 P(self.zeros.data_ptr()), C.byref(desc), P(meta.data_ptr()), P(out.ws.data_ptr()),
                                                 out.ws.numel(), stream_ptr())

    def finalize(self, which, fold=True):
        """statistics of pass `which` -> (a, b) (and the folded filters when the case has them and fold is set) -> status"""
        from lfd_amd._lib import lib, stream_ptr
        P = C.c_void_p
        gam, bet = self.gb[which - 1]
        if fold:
            return lib().lfd_groupnorm_finalize_fold(C.byref(self.d), P(self.partial.ptr), gam, bet, EPS, P(self.ab[which - 1].ptr), self.lv,
                                                     which, stream_ptr())
        return lib().lfd_groupnorm_finalize(C.byref(self.d), P(self.partial.ptr), gam, bet, EPS, P(self.ab[which - 1].ptr), stream_ptr())

    def chain(self):
        """the five launches; returns what every launch left: partial1, ab1, partial2, ab2, cls, reg (host tensors, guards checked)"""
        out = {}
        for p in (1, 2):
            self.partial.reset()
            assert self.forward(p) == 0 and self.finalize(p) == 0
            out['partial%d' % p], out['ab%d' % p] = self.partial.get().clone(), self.ab[p - 1].get().clone()
        assert self.forward(3) == 0
        out['cls'], out['reg'] = self.outputs()
        for f in self.folded:
            out.setdefault('folded', []).append(f.get().clone())
        for t in self.tower1:
            out.setdefault('tower1', []).append(t.get().clone())
        for x in self.x:
            x.get()
        return out

    def outputs(self):
        """cls, reg on the host: guards and the rows between the levels untouched, every row of a level written and finite (where the
        case has such rows); NaN where nothing is to be written, like the reference"""
        c, geo = self.c, self.geo
        cls, reg = self.cls.get(False).clone(), self.reg.get(False).clone()
        inside = torch.zeros(geo['P'], dtype=torch.bool)
        for (hw, _), po in zip(c['levels'], geo['p_off']):
            inside[po:po + hw] = True
        for t, rows in ((cls, c['cls_rows']), (reg, c['reg_rows'])):
            assert bool(torch.isnan(t[:, ~inside]).all()), 'row between the levels overwritten'
            if rows:
                assert bool(torch.isfinite(t[:, inside]).all()), 'unwritten or non-finite output'
            else:
                assert bool(torch.isnan(t).all()), 'output of a tower without such rows written'
        return cls, reg
