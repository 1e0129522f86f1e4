"""tests/golden/entry_i8_cases.py -- shapes, seeded operands and the integer reference for csrc/entry_i8.hip: lfd_entry_i8_fused,
a whole 64-channel stage-entry block in one launch, built on tests/golden/conv_i8_cases.py the way block_i8_cases.py is.

Operands are FULL-RANGE int8, independent per element.  The reference composes conv_i8_cases.acc_ref (exact integer sums over a
zero-padded input) and epilogue_ref (float64):
    y1 = q(ReLU(acc1(x) mult1 + biasq1))      3x3 stride 2
    id = q(accd(x) multd + biasqd)            1x1 stride 2, no ReLU
    v  = ReLU(acc2(y1) mult2 + biasq2 + id res_mult);  out = q(v)
acc_ref pads what it is given with zeros, so pixels outside the map are zero AT BOTH STAGES: the input halo, and the y1 map
(conv2's padding is 0, not conv1 evaluated outside the oh x ow map).

Two instruments, as for the single conv: exact constants (powers of two: every value of the three epilogues is exact in fp32, the
kernel must equal the reference bit for bit) and random constants (arbitrary fp32: the kernel must equal the launches it replaces
bit for bit -- both sides evaluate the same fp32 expressions on the same exact sums, so there is no near-tie allowance).

The fp16 input (in_format 1) has its own generator, f16_input: values whose product with in_inv_scale falls on half-integers and
on the fp16 neighbours of those, which is where a rounding mode other than one fp32 multiply + round-half-even shows.

Launch geometry restated (csrc/entry_i8.hip): tiles of 4 x 16 OUTPUT pixels, at most 256 workgroups (one per CU); workgroup b
runs tiles b, b + grid, ... of the order (image, tile row, tile column), one tile per step of a pipeline that alternates between two
LDS buffers of each kind."""
import collections
import functools

import torch

import conv_i8_cases as QC

TH, TW, MAX_WORKGROUPS = 4, 16, 256
BIG_BIAS = 64.0          # a conv1 bias under which "conv1 evaluated outside the map" is 64 in every channel, not 0
F16_CHANNELS = (32, 48, 64)

EntryCase = collections.namedtuple('EntryCase', 'kind n h w')              # h, w: the INPUT map


def out_hw(h, w):
    return (h - 1) // 2 + 1, (w - 1) // 2 + 1


def launch(c):
    """-> (tiles_x, tiles_y, ntiles, grid) of lfd_entry_i8_fused"""
    oh, ow = out_hw(c.h, c.w)
    tx, ty = -(-ow // TW), -(-oh // TH)
    nt = c.n * tx * ty
    return tx, ty, nt, min(nt, MAX_WORKGROUPS)


def _walk_images(cap, per_wg=1.5):
    """images of 2 x 3 tiles (two full, a ragged column and a ragged row of one pixel): per_wg tiles per workgroup of the capped
    grid, and cap = 4 mod 6, so a workgroup's next tile lies in another image at another place"""
    assert cap % 6 == 4
    return -(-int(2 * per_wg * cap) // (2 * 6))


def cases():
    return [EntryCase('pixel', 1, 1, 1),                                   # every halo pixel of both stages is outside the map
            EntryCase('edge_odd', 2, 2 * TH + 1, 2 * TW + 1),              # output 5 x 17: one tile plus one row and one column
            EntryCase('edge_even', 2, 2 * TH + 2, 2 * TW + 2),             # output 5 x 17, the 1x1 leaves the last input row / column unread
            EntryCase('general', 2, 37, 53),
            EntryCase('walk', _walk_images(MAX_WORKGROUPS), 2 * TH + 1, 4 * TW + 1),      # output 5 x 33
            # 3.5 tiles per workgroup: three or four steps, so every LDS buffer (input, y1, id) is written a second time while
            # its first contents have just been read -- where a missing barrier on buffer reuse would show
            EntryCase('walk_deep', _walk_images(MAX_WORKGROUPS, 3.5), 2 * TH + 1, 4 * TW + 1)]


def case_id(c):
    return '%s_%dx%dx%d' % (c.kind, c.n, c.h, c.w)


def _conv_case(c, which):
    """the conv_i8_cases.Case whose seed and magnitudes stand for conv1 (1), the identity branch ('d') or conv2 (2)"""
    if which == 1:
        return QC.Case(64, 64, 3, 2, c.kind, c.n, c.h, c.w)
    if which == 'd':
        return QC.Case(64, 64, 1, 2, c.kind, c.n, c.h, c.w)
    oh, ow = out_hw(c.h, c.w)
    return QC.Case(64, 64, 3, 1, c.kind, c.n, oh, ow + 1000)


@functools.lru_cache(maxsize=2)
def operands(c):
    """-> (x [n,h,w,64], w1 [64,64,3,3], wd [64,64,1,1], w2 [64,64,3,3]) int8 CPU tensors, full range"""
    s = QC.case_seed(_conv_case(c, 1)) + 9000011
    return (QC._randint8((c.n, c.h, c.w, 64), s), QC._randint8((64, 64, 3, 3), s + 1), QC._randint8((64, 64, 1, 1), s + 2),
            QC._randint8((64, 64, 3, 3), s + 3))


def exact_constants(c, big_bias=False):
    """(k1, kd, k2) conv_i8_cases.Consts of powers of two (conv_i8_cases.exact_constants, one draw per conv).  big_bias: conv1's
    biasq is BIG_BIAS in every channel"""
    k1, kd, k2 = (QC.exact_constants(_conv_case(c, which)) for which in (1, 'd', 2))
    if big_bias:
        k1 = k1._replace(biasq=torch.full((64,), BIG_BIAS))
    return k1, kd, k2


def random_constants(c):
    return tuple(QC.random_constants(_conv_case(c, which)) for which in (1, 'd', 2))


def entry_ref(x, w1, wd, w2, k1, kd, k2):
    """-> (y1 int8, id int8, v float64, q int8) on x's device; zero outside the map at both stages"""
    _, y1, _ = QC.epilogue_ref(QC.acc_ref(x, w1, 2), k1, None, True)
    _, ident, _ = QC.epilogue_ref(QC.acc_ref(x, wd, 2), kd, None, False)
    v, q, _ = QC.epilogue_ref(QC.acc_ref(y1, w2, 1), k2, ident, True)
    return y1, ident, v, q


def useful_share(q):
    """share of an int8 map that is neither 0 nor at a clamp: the values that carry information about the sums"""
    return float(((q != 0) & (q.abs() < QC.QMAX)).double().mean())


# ---------------------------------------------------------------------------------------------------- the fp16 input (format 1)
def _f16_step(x, up):
    """the next fp16 value above (up) or below x: +-1 on the sign-magnitude bit pattern (x finite, non-zero)"""
    b = x.view(torch.int16).clone()
    away = (x > 0) == up                                       # away from zero
    return (b + torch.where(away, torch.ones_like(b), -torch.ones_like(b))).view(torch.float16)


def f16_input(c, channels, exact=True):
    """-> (x [n,h,w,channels] fp16 CPU, in_inv_scale float).  A quarter of the elements each: a value whose product with
    in_inv_scale is (exact=True: exactly; else: as near as fp16 allows to) a half-integer k + 1/2 with |k + 1/2| up to 130 (past
    both clamps), its fp16 neighbour above, its neighbour below, and an unrelated value.
    exact=True: in_inv_scale = 4, x = (2 k + 1) / 8: the fp32 product is exact, so every tie is a true tie and round-half-even
    differs from round-half-away on every second one.  exact=False: an arbitrary fp32 in_inv_scale, where the one fp32 multiply
    rounds, so the side of the half-integer is decided by that one rounded product and by nothing else."""
    g = torch.Generator().manual_seed(QC.case_seed(_conv_case(c, 1)) + 1000 * channels + (77 if exact else 78))
    shape = (c.n, c.h, c.w, channels)
    inv = 4.0 if exact else float(torch.tensor(3.7193).float())
    k = torch.randint(-131, 130, shape, generator=g).double() + 0.5        # half-integers in [-130.5, 129.5]
    tie = (k / inv).half()
    kind = torch.randint(0, 4, shape, generator=g)
    other = ((torch.rand(shape, generator=g) * 2 - 1) * 40).half()
    x = torch.where(kind == 0, tie, torch.where(kind == 1, _f16_step(tie, True), torch.where(kind == 2, _f16_step(tie, False), other)))
    return x.contiguous(), inv


def quantize_ref(x, inv_scale, channels=64):
    """lfd_quantize_nhwc_f16_i8 / lfd_quantize_pad_nhwc_f16_i8 on the host: one fp32 multiply, round half even, clamp; channels
    above x's are 0"""
    q = torch.round(x.float() * torch.tensor(inv_scale, dtype=torch.float32)).clamp(-QC.QMAX, QC.QMAX).to(torch.int8)
    if channels != x.shape[-1]:
        q = torch.nn.functional.pad(q, (0, channels - x.shape[-1]))
    return q
