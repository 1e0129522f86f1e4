"""tests/golden/wgrad_cases.py -- seeded inputs, the float64 reference, the restated launch geometry and the case tables for
the conv weight-gradient kernels of csrc/train.hip and csrc/stem_gray_train.hip (tests/test_wgrad_reference_host.py keeps the
reference and the tables honest on the CPU, tests/test_gpu_wgrad.py compares the kernels with them).  The generators return CPU
tensors; no ctypes.  wgrad_ref / abs_ref run on whatever device their operands are on.

The instrument: x and dy hold INTEGERS in [-3, 3] (fp16; the first conv's image the same integers in fp32).  Every product is
an integer of magnitude <= 9 and every partial sum an integer below 2^24 as long as 9 * (output pixels) < 2^24, so fp32
accumulation is exact in any order and under any rounding inside the MFMA, the fp64 final pass is exact, a power-of-two
inv_scale is exact and += into an integer-valued dw is exact: the kernel must equal the float64 reference bit for bit
(exact_cap() states the condition; the host test checks it for every integer case).

Layouts: x [n, h, w, cin] and dy [n, ho, wo, cout] are NHWC; dW is OIHW [cout, cin, ks, ks]; pad = ks // 2."""
import functools

import torch

INT_LO, INT_HI = -3, 3
EXACT_LIMIT = 2 ** 24


# ------------------------------------------------------------------------------------------------ seeded inputs
def out_hw(h, w, ks, stride):
    pad = ks // 2
    return (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1


def int_tensor(shape, seed):
    """integers in [-3, 3], int8 (callers cast: fp16 operands, fp32 images, fp32 preloaded gradients)"""
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(INT_LO, INT_HI + 1, tuple(shape), generator=g, dtype=torch.int8)


def int_operands(n, h, w, cin, cout, ks, stride, seed):
    """-> (x [n, h, w, cin], dy [n, ho, wo, cout]) fp16 with integer values"""
    ho, wo = out_hw(h, w, ks, stride)
    return int_tensor((n, h, w, cin), seed).half(), int_tensor((n, ho, wo, cout), 100003 + int(seed)).half()


def gauss_operands(n, h, w, cin, cout, ks, stride, seed):
    """x ~ N(0, 1), dy ~ N(0, 0.05^2), fp16 (the distribution of tests/test_gpu_train_convs.py)"""
    ho, wo = out_hw(h, w, ks, stride)
    g = torch.Generator().manual_seed(int(seed))
    x = torch.randn((n, h, w, cin), generator=g).half()
    dy = (torch.randn((n, ho, wo, cout), generator=g) * 0.05).half()
    return x, dy


def int_preload(shape, seed):
    """an integer-valued fp32 gradient buffer to accumulate into"""
    return int_tensor(shape, 200003 + int(seed)).float()


# ------------------------------------------------------------------------------------------------ float64 reference
REF_CHUNK_ELEMS = 1 << 25        # elements of the padded x rows of one chunk: 256 MB of float64 (dy's rows are fewer)


def wgrad_ref(x, dy, ks, stride):
    """dW[:, :, ky, kx] = dy_flat^T @ x_shifted_flat in float64 (the definition in the header comment of k_wgrad): nine strided
    slices of the zero-padded x, no conv call.  x [n, h, w, cin], dy [n, ho, wo, cout], any float dtype -> [cout, cin, ks, ks].
    Works image by image in chunks of output rows."""
    n, h, w, cin = x.shape
    ho, wo = out_hw(h, w, ks, stride)
    cout = dy.size(3)
    assert tuple(dy.shape) == (n, ho, wo, cout), (tuple(dy.shape), (n, ho, wo, cout))
    pad = ks // 2
    out = torch.zeros((cout, cin, ks, ks), dtype=torch.float64, device=x.device)
    rows = max(1, REF_CHUNK_ELEMS // ((w + 2 * pad) * max(cin, cout) * stride))
    for img in range(n):
        for r0 in range(0, ho, rows):
            r1 = min(ho, r0 + rows)
            # padded rows r0 * stride .. (r1 - 1) * stride + ks - 1 = input rows shifted by -pad
            lo, hi = r0 * stride - pad, (r1 - 1) * stride + ks - 1 - pad
            xp = torch.zeros((hi - lo + 1, w + 2 * pad, cin), dtype=torch.float64, device=x.device)
            a, b = max(lo, 0), min(hi, h - 1)
            if b >= a:
                xp[a - lo:b - lo + 1, pad:pad + w] = x[img, a:b + 1].double()
            d = dy[img, r0:r1].double().reshape(-1, cout)
            for ky in range(ks):
                for kx in range(ks):
                    xs = xp[ky:ky + (r1 - r0 - 1) * stride + 1:stride, kx:kx + (wo - 1) * stride + 1:stride]
                    out[:, :, ky, kx] += d.t() @ xs.reshape(-1, cin)
    return out


def abs_ref(x, dy, ks, stride):
    """the same contraction over |x| and |dy|: the sum of the magnitudes of the terms of every dW entry"""
    return wgrad_ref(x.abs(), dy.abs(), ks, stride)


def gauss_bound(ref, a, tiles, rows):
    """|got - ref| <= L * 2^-23 * A + 2^-24 * |ref|: L = 128 * ceil(tiles / rows) pixels a workgroup accumulates in fp32 before
    the fp64 pass (2^-23 instead of fp32's unit roundoff 2^-24: MFMA accumulation may not round to nearest), then one rounding
    of the float64 sum to fp32"""
    length = 128 * -(-tiles // rows)
    return length * 2.0 ** -23 * a + 2.0 ** -24 * ref.abs()


def exact_cap(pixels, inv_scale=1.0, preload=0):
    """the largest magnitude, in units of the result's granularity, an exact run goes through: `pixels` output pixels (all
    partial sets of a chained dW together) of products <= 9, scaled by a power-of-two inv_scale and added to an integer of
    magnitude <= preload.  Exact while this stays below 2^24."""
    assert inv_scale > 0 and (1.0 / inv_scale) == int(1.0 / inv_scale) and int(1.0 / inv_scale) & (int(1.0 / inv_scale) - 1) == 0
    return INT_HI * INT_HI * pixels + preload / inv_scale


# ------------------------------------------------------------------------------------------------ launch geometry
WG_MAX, WG_CAP = 256, 1024        # kWgradMaxWg, kWgradWgCap
TAP_SPLIT_BYTES, TIER_512_BYTES, TIER_1024_BYTES = 16 << 20, 32 << 20, 128 << 20


def geometry(n, h, w, cin, cout, ks, stride):
    """wgrad_geometry() of csrc/train.hip restated -> dict(path, rows, blocks, tiles, ho, wo).  Paths:
    'tap_split'        3x3, operands <= 16 MB: the 1x1 kernel, one tap per blockIdx.z
    'all_taps'         3x3 above that: k_wgrad<3, S>, 256 rows
    'all_taps_tiles6'  stride 2 with 256 < tiles / 6 < 512 rows;  'all_taps_512' at the cap of 512
    '1x1_256' / '1x1_512' / '1x1_1024'   k_wgrad<1, S> with rows x blocks = the tier of the operand size
    rows never exceed tiles; the partials of one launch never exceed 256 x 4 blocks x 9 taps."""
    assert ks in (1, 3) and stride in (1, 2) and cin % 8 == 0 and cout % 8 == 0 and 8 <= cin <= 128 and 8 <= cout <= 128
    ho, wo = out_hw(h, w, ks, stride)
    blocks = -(-cout // 64) * -(-cin // 64)
    tiles = n * -(-ho // 8) * -(-wo // 16)
    operand_bytes = (n * h * w * cin + n * ho * wo * cout) * 2
    if ks == 3 and operand_bytes <= TAP_SPLIT_BYTES:
        path, rows = 'tap_split', {1: 40, 2: 16}.get(blocks, 8)
    elif ks == 3:
        path, rows = 'all_taps', WG_MAX
        if stride == 2:
            rows = min(max(tiles // 6, 256), 512)
            rows = min(rows, WG_MAX * 4 // blocks)
            path = 'all_taps' if rows == 256 else ('all_taps_512' if rows == 512 else 'all_taps_tiles6')
    else:
        tier = 1024 if operand_bytes >= TIER_1024_BYTES else (512 if operand_bytes >= TIER_512_BYTES else 256)
        path, rows = '1x1_%d' % tier, tier // blocks
    rows = min(rows, WG_CAP, tiles)
    return dict(path=path, rows=rows, blocks=blocks, tiles=tiles, ho=ho, wo=wo)


# paths a (ks, stride) can reach
REACHABLE = {(3, 1): ('tap_split', 'all_taps'), (3, 2): ('tap_split', 'all_taps', 'all_taps_tiles6', 'all_taps_512'),
             (1, 1): ('1x1_256', '1x1_512', '1x1_1024'), (1, 2): ('1x1_256', '1x1_512', '1x1_1024')}


# ------------------------------------------------------------------------------------------------ case tables
KS_STRIDE = [(3, 1), (3, 2), (1, 1), (1, 2)]
# (a) edges of every path: maps (n, h, w); (2, 8, 16) is exactly one tile, (1, 9, 17) one past a tile in both directions
EDGE_MAPS = [(1, 1, 1), (1, 1, 17), (1, 9, 1), (2, 8, 16), (1, 9, 17), (3, 31, 30), (2, 37, 53), (4, 80, 80)]
# stride 2 also: exactly one OUTPUT tile from an even and from an odd map, one past it with even h / odd w, the parities
# (even, odd) of a multi-tile map -- with EDGE_MAPS every parity of (h, w)
EDGE_MAPS_S2 = [(2, 16, 32), (2, 15, 31), (1, 18, 33), (3, 30, 31)]
EDGE_CHANNELS = [(32, 64), (128, 64), (64, 128), (128, 128), (32, 32)]          # besides (64, 64), on EDGE_CHANNEL_MAPS
EDGE_CHANNEL_MAPS = [(1, 1, 17), (1, 9, 1), (1, 9, 17), (3, 31, 30)]


def edge_cases():
    """-> [(n, h, w, cin, cout, ks, stride)]"""
    out = []
    for ks, stride in KS_STRIDE:
        for m in EDGE_MAPS + (EDGE_MAPS_S2 if stride == 2 else []):
            out.append(m + (64, 64, ks, stride))
        for cin, cout in EDGE_CHANNELS:
            for m in EDGE_CHANNEL_MAPS:
                out.append(m + (cin, cout, ks, stride))
    return out


# (b) the paths above the thresholds: ((n, h, w, cin, cout, ks, stride), path).  Every map has ragged right and bottom tiles.
PATH_CASES = [
    ((1, 129, 257, 128, 128, 3, 1), 'all_taps'),             # 16.2 MB, 4 blocks, 289 tiles on 256 rows
    ((2, 129, 257, 64, 64, 3, 1), 'all_taps'),               # 578 tiles: a workgroup's tile sequence crosses the image boundary
    ((2, 297, 297, 64, 128, 3, 2), 'all_taps'),              # stride 2, 380 tiles on 256 rows, 2 blocks
    ((1, 1024, 1000, 64, 64, 3, 2), 'all_taps_tiles6'),      # 2048 tiles -> 341 rows
    ((2, 1000, 1000, 32, 32, 3, 2), 'all_taps_512'),         # 4032 tiles -> the 512 cap
    ((1, 900, 900, 128, 128, 3, 2), 'all_taps'),             # 1653 tiles / 6 = 275 rows x 4 blocks would not fit the workspace: 256
    ((3, 130, 131, 64, 64, 1, 1), '1x1_256'),                # 459 tiles on 256 rows
    ((1, 257, 259, 128, 128, 1, 1), '1x1_512'),              # 4 blocks x 128 rows
    ((1, 515, 510, 128, 128, 1, 1), '1x1_1024'),             # 4 blocks x 256 rows
    ((1, 363, 362, 64, 64, 1, 1), '1x1_512'),                # one block x 512 rows
    ((1, 725, 724, 64, 64, 1, 1), '1x1_1024'),               # one block x 1024 rows
    ((2, 259, 261, 64, 64, 1, 2), '1x1_256'),
    ((2, 365, 363, 64, 64, 1, 2), '1x1_512'),
    ((1, 649, 650, 128, 128, 1, 2), '1x1_1024'),
]
# (c) rows of the final sum: 1x1 64 -> 64 on (1, 8, 16 k) has k tiles and k rows
FINAL_ROWS = [1, 2, 7, 8, 9, 56, 57, 63, 64, 65, 120, 121]
FINAL_INV_SCALES = [1.0, 0.25]
# (d) channel counts the entry point accepts
ODD_CHANNELS = [(8, 8), (24, 40), (72, 104), (128, 8)]
ODD_CHANNEL_MAP = (2, 9, 17)
ODD_CHANNEL_KS_STRIDE = [(3, 1), (1, 2)]
# (e) the deferred path: one WgradFinals.launch().  name -> (n, h, w, cin, cout, ks, stride), inv_scale
DEFERRED_JOBS = [
    ('conv3x3', (2, 37, 53, 64, 128, 3, 1), 0.25),           # 2 blocks x 9 taps
    ('level0', (2, 19, 23, 64, 64, 3, 1), 1.0),              # shared conv, first pyramid level: head of the chain
    ('conv1x1', (3, 31, 30, 128, 128, 1, 2), 1.0),           # 4 blocks x 1 tap
    ('sliced', (1, 9, 17, 64, 64, 1, 1), 0.5),               # rows 0..39 and 40..63 go to two parameters
    ('level1', (2, 10, 12, 64, 64, 3, 1), 1.0),              # the same conv on the next level: chained into level0's dW
]
DEFERRED_SLICES = [(0, 40), (40, 64)]
DEFERRED_ROWSUMS = [dict(count=1, nrows=1, row_stride=7, accumulate=False), dict(count=300, nrows=5, row_stride=333, accumulate=True)]
# (f) the re-formed operand
XPRO_CIN = [32, 128]
XPRO_MAP, XPRO_COUT = (2, 37, 53), 64
# (g) the first conv (stride 2, pad 1, cin 3 or 1); the last map has > 4096 k-steps in both kernels (16 / 32 output pixels
# per k-step): the partial rows reach their cap of 1024
STEM_MAPS = [(1, 1, 1), (1, 2, 2), (1, 5, 3), (2, 31, 33), (3, 61, 77), (2, 260, 1030)]
STEM_CHANNELS = [32, 64]
STEM_CIN = [3, 1]
STEM_ROW_CAP = 1024


def stem_rows(n, h, w, cin):
    ho, wo = out_hw(h, w, 3, 2)
    ksteps = n * ho * -(-wo // (16 if cin == 3 else 32))
    return min(max(ksteps // 4, 1), STEM_ROW_CAP), ksteps


# (h) rounding behaviour on Gaussian inputs: every case of (b) and (2, 37, 53) per (ks, stride)
GAUSS_CASES = [c for c, _ in PATH_CASES] + [(2, 37, 53, 64, 64, ks, stride) for ks, stride in KS_STRIDE]


def case_id(c):
    return '%dx%dx%d_%dto%d_k%ds%d' % tuple(c)


def case_seed(c):
    return sum(v * p for v, p in zip(c, (1, 3, 7, 11, 13, 17, 19)))


@functools.lru_cache(maxsize=8)
def small_int_operands(c):
    """cached: the edge maps are shared by the tests that run them more than once"""
    return int_operands(*c, seed=case_seed(c))
