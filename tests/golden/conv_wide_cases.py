"""tests/golden/conv_wide_cases.py -- case tables and seeded operands for csrc/conv_wide.hip (the layers with cin or cout above
128 that LFDResNet's 'fast' / 'faster' body presets bring, and the four <= 128 layers of FastBlock / FastestBlock bodies
that conv_dispatch routes there because csrc/conv.hip has no instance for them).  The
float64 reference is conv_cases.conv_ref (ks * ks shifted matmuls, no conv call); tests/test_gpu_conv_wide.py compares.

The instrument: x holds INTEGERS in [-2, 2] (fp16), the filter integers in {-1, 0, 1}, the bias integers in [-8, 8] (fp32),
the residual integers in [-64, 64] (fp16).  Every fp32 partial sum is an integer of magnitude <= 2 * K + 72 (K = ks * ks * cin
<= 4608) < 2^24: the accumulation is exact in any order, split over the four waves or not.  A sum of K terms of variance
(2) * (2 / 3) has sigma = sqrt(4 K / 3): 78 at K = 4608, so an output beyond 2048 -- the range in which fp16 holds every
integer -- is a 26-sigma event; the tests assert max |ref| <= 2048 on the reference before comparing, and
tests/test_presets_host.py checks it on the CPU for every case but the (larger) walk maps.

Launch geometry restated (csrc/conv_wide.hip): tiles of 4 x 16 output pixels, one 32-channel slab per workgroup, grid =
(min(ntiles, 1024 // slabs), slabs); workgroup b walks tiles b, b + grid.x, ..."""
import collections
import functools

import conv_cases as CC

X_HI, W_HI, BIAS_HI, RES_HI = 2, 1, 8, 64
TH, TW, MAX_WORKGROUPS = 4, 16, 1024

# (cin, cout, ks, stride, residual) -- the list of the issue, in its order
WIDE_SHAPES = [
    (128, 256, 3, 2, 0), (256, 512, 3, 2, 0), (256, 256, 3, 2, 0),
    (256, 256, 3, 1, 1), (256, 256, 3, 1, 0), (512, 512, 3, 1, 1), (512, 512, 3, 1, 0),
    (128, 256, 3, 1, 0), (256, 512, 3, 1, 0), (256, 128, 3, 1, 0), (512, 256, 3, 1, 0),
    (256, 256, 1, 1, 0), (512, 512, 1, 1, 0), (128, 256, 1, 2, 0), (256, 512, 1, 2, 0), (256, 128, 1, 1, 0), (512, 128, 1, 1, 0),
]
# the <= 128 keys the FastBlock / FastestBlock bodies need and csrc/conv.hip lacked: conv_dispatch routes them to the wide
# kernel as well (a 32-channel input is one half-filled chunk there)
ROUTED_SHAPES = [(64, 32, 3, 2, 0), (64, 32, 1, 2, 0), (32, 64, 3, 1, 0), (32, 64, 3, 1, 1), (32, 32, 1, 2, 0)]

Case = collections.namedtuple('Case', 'cin cout ks stride res kind n h w')


def launch(n, oh, ow, cout):
    """-> (tiles_x, tiles_y, ntiles, grid.x) of lfd_conv_wide_launch"""
    tx, ty = -(-ow // TW), -(-oh // TH)
    nt = n * tx * ty
    return tx, ty, nt, min(nt, MAX_WORKGROUPS // (cout // 32))


def walk_shape(cout, stride):
    """images of 5 x 33 output pixels -- 2 x 3 tiles: two full, a ragged right column of one pixel, a ragged bottom row of
    one pixel under each -- about 1.5 tiles per workgroup of the capped grid: some workgroups run one tile, some two, and a
    workgroup's two tiles lie in different images at different places (the grid width is 4 mod 6 or 2 mod 6).  Odd inputs
    under stride 2."""
    cap = MAX_WORKGROUPS // (cout // 32)
    n = -(-(3 * cap) // (2 * 6))
    return n, CC.in_size(TH + 1, stride), CC.in_size(2 * TW + 1, stride)


def shapes_of(s):
    cin, cout, ks, stride, res = s
    maps = [('9x11', (2, 9, 11)), ('8x10', (2, 8, 10)), ('pixel', (1, 1, 1)), ('walk', walk_shape(cout, stride))]
    return [Case(cin, cout, ks, stride, res, kind, *m) for kind, m in maps]


def wide_cases():
    return [c for s in WIDE_SHAPES + ROUTED_SHAPES for c in shapes_of(s)]


def case_id(c):
    return '%dto%d_k%ds%d_%s_%s_%dx%dx%d' % (c.cin, c.cout, c.ks, c.stride, 'res' if c.res else 'plain', c.kind, c.n, c.h, c.w)


def case_seed(c):
    return sum(int(v) * p for v, p in zip((c.cin, c.ks, c.stride, c.cout, c.res, c.n, c.h, c.w), (1, 3, 7, 11, 13, 17, 19, 23)))


@functools.lru_cache(maxsize=2)
def int_operands(c):
    """-> CC.Operands (CPU): x fp16, w fp32 OIHW, b fp32, res fp16 [n, oh, ow, cout], integers in the ranges above"""
    oh, ow = CC.out_hw(c.h, c.w, c.ks, c.stride)
    s = case_seed(c)
    x = CC.int_tensor((c.n, c.h, c.w, c.cin), X_HI, s).half()
    w = CC.int_tensor((c.cout, c.cin, c.ks, c.ks), W_HI, s + 100003).float()
    b = CC.int_tensor((c.cout,), BIAS_HI, s + 200003).float()
    res = CC.int_tensor((c.n, oh, ow, c.cout), RES_HI, s + 300007).half()
    return CC.Operands(x, w, b, res, None, None, None, None)


def gauss_operands(c):
    return CC.gauss_operands(c.n, c.h, c.w, c.cin, c.cout, c.ks, c.stride, case_seed(c) + 1)


def case_ref(c, o, relu):
    """float64, on the device the operands are on"""
    return CC.conv_ref(o.x, o.w, o.b, c.stride, residual=o.res if c.res else None, relu=bool(relu))
