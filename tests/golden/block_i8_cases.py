"""tests/golden/block_i8_cases.py -- shapes, seeded operands and the integer reference for csrc/block_i8.hip: lfd_block_i8_fused
(a whole 64-channel residual block) and for csrc/conv_i8.hip's pair instances: lfd_conv2d_downsample_nhwc_i8 (the two stride-2 convs of
a stage-entry block), built on
tests/golden/conv_i8_cases.py.

Operands are FULL-RANGE int8, independent per element.  The reference composes conv_i8_cases.acc_ref (exact integer sums over a
zero-padded input) and epilogue_ref (float64):
    mid = q(ReLU(acc1 mult1 + biasq1));  v = ReLU(acc2(mid) mult2 + biasq2 + x res_mult);  out = q(v), tap = half(v out_scale)
acc_ref pads what it is given with zeros, so pixels outside the image are zero AT BOTH STAGES: the input halo, and the mid map
(conv2's padding is 0, not conv1 evaluated outside the image).

Two instruments, as for the single conv: exact_constants (powers of two: every value of both epilogues is exact in fp32, the
kernel must equal the reference bit for bit) and random_constants (arbitrary fp32: the kernel must equal the layer-by-layer
launches bit for bit -- both sides evaluate the same fp32 expressions on the same exact sums, so there is no near-tie allowance).

Launch geometry restated (csrc/block_i8.hip, csrc/conv_i8.hip): the block kernel walks tiles of 8 x 16 output pixels with at most 256 workgroups
(one per CU), the pair kernel tiles of 4 x 16 OUTPUT pixels with at most 1024; workgroup b runs tiles b, b + grid, ... of the
order (image, tile row, tile column)."""
import collections
import functools

import torch

import conv_i8_cases as QC

TH, TW, MAX_WORKGROUPS = 8, 16, 256
PAIR_TH, PAIR_TW, PAIR_MAX_WORKGROUPS = 4, 16, 1024
PAIR_KEYS = [(64, 64), (64, 128), (128, 128)]
BIG_BIAS = 64.0          # a conv1 bias under which "conv1 evaluated outside the image" is 64 in every channel, not 0

BlockCase = collections.namedtuple('BlockCase', 'kind n h w')
PairCase = collections.namedtuple('PairCase', 'cin cout kind n h w')          # h, w: the INPUT map


def block_launch(c):
    """-> (tiles_x, tiles_y, ntiles, grid) of lfd_block_i8_fused"""
    tx, ty = -(-c.w // TW), -(-c.h // TH)
    nt = c.n * tx * ty
    return tx, ty, nt, min(nt, MAX_WORKGROUPS)


def pair_out_hw(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def pair_launch(c):
    oh, ow = pair_out_hw(c.h, c.w)
    tx, ty = -(-ow // PAIR_TW), -(-oh // PAIR_TH)
    nt = c.n * tx * ty
    return tx, ty, nt, min(nt, PAIR_MAX_WORKGROUPS)


def _walk_images(cap):
    """images of 2 x 3 tiles (two full, a ragged column and a ragged row of one pixel): 1.5 tiles per workgroup of the capped
    grid, and cap = 4 mod 6 for both caps, so a workgroup's second tile lies in another image at another place"""
    assert cap % 6 == 4
    return -(-(3 * cap) // (2 * 6))


def block_cases():
    return [BlockCase('pixel', 1, 1, 1),                                  # every halo pixel of both stages is outside the image
            BlockCase('edge', 2, TH + 1, TW + 1),                         # one tile plus one row and one column
            BlockCase('general', 2, 37, 53),
            BlockCase('walk', _walk_images(MAX_WORKGROUPS), TH + 1, 2 * TW + 1)]


def pair_cases():
    out = []
    for cin, cout in PAIR_KEYS:
        out += [PairCase(cin, cout, 'pixel', 1, 1, 1),
                PairCase(cin, cout, 'edge_odd', 2, 2 * PAIR_TH + 1, 2 * PAIR_TW + 1),      # output 5 x 17
                PairCase(cin, cout, 'edge_even', 2, 2 * PAIR_TH + 2, 2 * PAIR_TW + 2),     # output 5 x 17, the last row / column unread
                PairCase(cin, cout, 'general', 2, 37, 53),
                PairCase(cin, cout, 'walk', _walk_images(PAIR_MAX_WORKGROUPS), 2 * PAIR_TH + 1, 4 * PAIR_TW + 1)]   # output 5 x 33
    return out


def block_id(c):
    return '%s_%dx%dx%d' % (c.kind, c.n, c.h, c.w)


def pair_id(c):
    return '%dto%d_%s_%dx%dx%d' % (c.cin, c.cout, c.kind, c.n, c.h, c.w)


def _conv_case(c, which):
    """the conv_i8_cases.Case whose seed and magnitudes stand for conv `which` (1 | 2) of a block case"""
    return QC.Case(64, 64, 3, 1, c.kind, c.n, c.h, c.w + 1000 * (which - 1))


@functools.lru_cache(maxsize=2)
def block_operands(c):
    """-> (x [n,h,w,64], w1, w2 [64,64,3,3]) int8 CPU tensors, full range"""
    s = QC.case_seed(_conv_case(c, 1)) + 5000011
    return QC._randint8((c.n, c.h, c.w, 64), s), QC._randint8((64, 64, 3, 3), s + 1), QC._randint8((64, 64, 3, 3), s + 2)


def block_exact_constants(c, big_bias=False):
    """(k1, k2) conv_i8_cases.Consts of powers of two (conv_i8_cases.exact_constants, one draw per conv).  big_bias: conv1's
    biasq is BIG_BIAS in every channel"""
    k1, k2 = QC.exact_constants(_conv_case(c, 1)), QC.exact_constants(_conv_case(c, 2))
    if big_bias:
        k1 = k1._replace(biasq=torch.full((64,), BIG_BIAS))
    return k1, k2


def block_random_constants(c):
    return QC.random_constants(_conv_case(c, 1)), QC.random_constants(_conv_case(c, 2))


def block_ref(x, w1, w2, k1, k2):
    """-> (mid int8, v float64, q int8, tap float64 = v * out_scale) on x's device; zero outside the image at both stages"""
    _, mid, _ = QC.epilogue_ref(QC.acc_ref(x, w1, 1), k1, None, True)
    v, q, f = QC.epilogue_ref(QC.acc_ref(mid, w2, 1), k2, x, True)
    return mid, v, q, f


def _pair_conv_case(c, ks):
    return QC.Case(c.cin, c.cout, ks, 2, c.kind, c.n, c.h, c.w)


@functools.lru_cache(maxsize=2)
def pair_operands(c):
    """-> (x [n,h,w,cin], w3 [cout,cin,3,3], wd [cout,cin,1,1]) int8 CPU tensors, full range"""
    s = QC.case_seed(_pair_conv_case(c, 3)) + 7000003
    return QC._randint8((c.n, c.h, c.w, c.cin), s), QC._randint8((c.cout, c.cin, 3, 3), s + 1), QC._randint8((c.cout, c.cin, 1, 1), s + 2)


def pair_exact_constants(c):
    """(k3, kd): each conv's own constants"""
    return QC.exact_constants(_pair_conv_case(c, 3)), QC.exact_constants(_pair_conv_case(c, 1))


def pair_random_constants(c):
    return QC.random_constants(_pair_conv_case(c, 3)), QC.random_constants(_pair_conv_case(c, 1))


def pair_ref(x, w3, wd, k3, kd):
    """-> (v3, q3 int8 (ReLU), vd, qd int8 (no ReLU))"""
    v3, q3, _ = QC.epilogue_ref(QC.acc_ref(x, w3, 2), k3, None, True)
    vd, qd, _ = QC.epilogue_ref(QC.acc_ref(x, wd, 2), kd, None, False)
    return v3, q3, vd, qd
