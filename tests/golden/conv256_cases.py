"""tests/golden/conv256_cases.py -- case table and seeded operands for csrc/conv256.hip (lfd_conv256_nhwc_f16: 3x3 / 1x1
stride-1 conv from 256 channels, all output channels of a 128-pixel tile per workgroup), in the manner of
tests/golden/conv_wide_cases.py.  The float64 reference is conv_cases.conv_ref (ks * ks shifted matmuls, no conv call).

The instrument: x holds INTEGERS in [-2, 2] (fp16), the filter integers in {-1, 0, 1}, the bias integers in [-8, 8] (fp32).
Every fp32 partial sum is an integer of magnitude <= 2 * K + 8 (K = 9 * 256 = 2304) < 2^24: the accumulation is exact in any
order.  A sum of K terms of variance 2 * (2 / 3) has sigma = sqrt(4 K / 3) = 55.4, so an output beyond 2048 -- the range in
which fp16 holds every integer -- is a > 35-sigma event; the tests assert max |ref| <= 2048 before comparing, and
tests/test_conv256_host.py checks it on the CPU for every case but the (larger) walk maps.

Launch geometry restated (csrc/conv256.hip): tiles of 8 x 16 output pixels, every output channel in one workgroup, grid =
min(ntiles, 512); workgroup b walks tiles b, b + grid, ... of the order (image, tile row, tile column).  cout > 128 runs four
channel groups of 64, cout > 64 two, else one."""
import collections
import functools

import conv_cases as CC

X_HI, W_HI, BIAS_HI = 2, 1, 8
CIN = 256
TH, TW, MAX_WORKGROUPS = 8, 16, 512

# cout 256 (four channel groups), 96 (two groups, the second half filled: the slab guard), 32 (one group, half filled: the
# heads' centerness / regression rows)
COUTS = (256, 96, 32)

Case = collections.namedtuple('Case', 'cout ks kind n h w')


def launch(n, h, w):
    """-> (tiles_x, tiles_y, ntiles, grid) of lfd_conv256_nhwc_f16"""
    tx, ty = -(-w // TW), -(-h // TH)
    nt = n * tx * ty
    return tx, ty, nt, min(nt, MAX_WORKGROUPS)


def channel_groups(cout):
    return 4 if cout > 128 else (2 if cout > 64 else 1)


def walk_shape():
    """images of 9 x 33 pixels -- 2 x 3 tiles: two full, a ragged right column of one pixel, a ragged bottom row of one pixel
    under each -- just enough of them for 1.5 tiles per workgroup of the capped grid: workgroups 0 .. 255 run two tiles, the
    others one, and a workgroup's two tiles lie in different images at different places (the grid width is 2 mod 6)."""
    n = -(-(3 * MAX_WORKGROUPS) // (2 * 6))
    return n, TH + 1, 2 * TW + 1


MAPS = [('pixel', (1, 1, 1)), ('small', (2, 5, 11)), ('edge', (2, TH + 1, TW + 1)), ('walk', walk_shape())]


def cases():
    """3x3: every cout on every map; 1x1 (the fp32-output instance only): every cout on the small maps"""
    out = [Case(cout, 3, kind, *m) for cout in COUTS for kind, m in MAPS]
    out += [Case(cout, 1, kind, *m) for cout in COUTS for kind, m in MAPS if kind in ('pixel', 'edge')]
    return out


def case_id(c):
    return '256to%d_k%d_%s_%dx%dx%d' % (c.cout, c.ks, c.kind, c.n, c.h, c.w)


def case_seed(c):
    return sum(int(v) * p for v, p in zip((c.cout, c.ks, c.n, c.h, c.w), (11, 3, 17, 19, 23))) + 256


@functools.lru_cache(maxsize=2)
def int_operands(c):
    """-> CC.Operands (CPU): x fp16, w fp32 OIHW, b fp32, integers in the ranges above"""
    s = case_seed(c)
    x = CC.int_tensor((c.n, c.h, c.w, CIN), X_HI, s).half()
    w = CC.int_tensor((c.cout, CIN, c.ks, c.ks), W_HI, s + 100003).float()
    b = CC.int_tensor((c.cout,), BIAS_HI, s + 200003).float()
    return CC.Operands(x, w, b, None, None, None, None, None)


def gauss_operands(c):
    return CC.gauss_operands(c.n, c.h, c.w, CIN, c.cout, c.ks, 1, case_seed(c) + 1)


def case_ref(c, o, relu):
    """float64, on the device the operands are on"""
    return CC.conv_ref(o.x, o.w, o.b, 1, relu=bool(relu))


def abs_ref(o):
    """sum |x| |w| per output (float64): the scale of the per-launch tolerance"""
    return CC.conv_ref(o.x.abs(), o.w.abs(), None, 1)
