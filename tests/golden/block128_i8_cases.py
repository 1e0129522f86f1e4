"""tests/golden/block128_i8_cases.py -- shapes, seeded operands and the integer reference for csrc/block128_i8.hip:
lfd_block128_i8_fused, a whole 128-channel residual block in one launch.  Built on tests/golden/conv_i8_cases.py and modelled on
tests/golden/block_i8_cases.py.

Operands are FULL-RANGE int8, independent per element.  The reference composes conv_i8_cases.acc_ref (exact integer sums over a
zero-padded input) and epilogue_ref (float64):
    mid = q(ReLU(acc1 mult1 + biasq1));  v = ReLU(acc2(mid) mult2 + biasq2 + x res_mult);  out = q(v), tap = half(v out_scale)
acc_ref pads what it is given with zeros, so pixels outside the image are zero AT BOTH STAGES: the input halo, and the mid map
(conv2's padding is 0, not conv1 evaluated outside the image).

Two instruments, as for the 64-channel block: exact_constants (powers of two from the (128, 128, 3, 1) key: every value of both
epilogues is exact in fp32, the kernel must equal the reference bit for bit) and random_constants (arbitrary fp32: the kernel must
equal the two lfd_conv2d_nhwc_i8 launches bit for bit -- both sides evaluate the same fp32 expressions on the same exact sums, so
there is no near-tie allowance).

Launch geometry restated (csrc/block128_i8.hip): tiles of 8 x 16 output pixels, at most 256 workgroups (one per CU, one wave per
SIMD); workgroup b runs tiles b, b + grid, ... of the order (image, tile row, tile column).  Per tile a workgroup alternates
between two input-halo buffers in LDS and reuses one mid buffer and one 4-register halo ring (filled twice per tile), so the
walk case gives a workgroup of the capped grid at least 3.5 tiles: every buffer is reused at least once."""
import collections
import functools

import torch

import conv_i8_cases as QC

C = 128
TH, TW, MAX_WORKGROUPS = 8, 16, 256
WALK_TILES_PER_WORKGROUP = 3.5
BIG_BIAS = 64.0          # a conv1 bias under which "conv1 evaluated outside the image" is 64 in every channel, not 0

Case = collections.namedtuple('Case', 'kind n h w')


def launch(c):
    """-> (tiles_x, tiles_y, ntiles, grid) of lfd_block128_i8_fused"""
    tx, ty = -(-c.w // TW), -(-c.h // TH)
    nt = c.n * tx * ty
    return tx, ty, nt, min(nt, MAX_WORKGROUPS)


def _walk_images(cap):
    """images of 2 x 3 tiles (two full, a ragged column and a ragged row of one pixel): at least WALK_TILES_PER_WORKGROUP tiles
    per workgroup of the capped grid, and cap = 4 mod 6, so a workgroup's consecutive tiles lie in different images at
    different places"""
    assert cap % 6 == 4 and cap >= 6
    return -(-int(2 * WALK_TILES_PER_WORKGROUP * cap) // (2 * 6))


def cases():
    return [Case('pixel', 1, 1, 1),                                       # every halo pixel of both stages is outside the image
            Case('edge', 2, TH + 1, TW + 1),                              # one tile plus one row and one column
            Case('general', 2, 37, 53),
            Case('walk', _walk_images(MAX_WORKGROUPS), TH + 1, 2 * TW + 1)]


def case_id(c):
    return '%s_%dx%dx%d' % (c.kind, c.n, c.h, c.w)


def _conv_case(c, which):
    """the conv_i8_cases.Case whose seed and magnitudes stand for conv `which` (1 | 2) of a block case"""
    return QC.Case(C, C, 3, 1, c.kind, c.n, c.h, c.w + 1000 * (which - 1))


@functools.lru_cache(maxsize=2)
def operands(c):
    """-> (x [n,h,w,128], w1, w2 [128,128,3,3]) int8 CPU tensors, full range"""
    s = QC.case_seed(_conv_case(c, 1)) + 9000011
    return QC._randint8((c.n, c.h, c.w, C), s), QC._randint8((C, C, 3, 3), s + 1), QC._randint8((C, C, 3, 3), s + 2)


def exact_constants(c, big_bias=False):
    """(k1, k2) conv_i8_cases.Consts of powers of two (conv_i8_cases.exact_constants, one draw per conv).  big_bias: conv1's
    biasq is BIG_BIAS in every channel"""
    k1, k2 = QC.exact_constants(_conv_case(c, 1)), QC.exact_constants(_conv_case(c, 2))
    if big_bias:
        k1 = k1._replace(biasq=torch.full((C,), BIG_BIAS))
    return k1, k2


def random_constants(c):
    return QC.random_constants(_conv_case(c, 1)), QC.random_constants(_conv_case(c, 2))


def block128_ref(x, w1, w2, k1, k2):
    """-> (mid int8, v float64, q int8, tap float64 = v * out_scale) on x's device; zero outside the image at both stages"""
    _, mid, _ = QC.epilogue_ref(QC.acc_ref(x, w1, 1), k1, None, True)
    v, q, f = QC.epilogue_ref(QC.acc_ref(mid, w2, 1), k2, x, True)
    return mid, v, q, f
