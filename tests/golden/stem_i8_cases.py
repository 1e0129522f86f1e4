"""tests/golden/stem_i8_cases.py -- the reference and the case tables for the int8-output forms of the RGB stem launches:
lfd_stem_conv_i8 (csrc/stem.hip, k_stem<2, FMT, true, true>) and lfd_stem_faster_fused_i8 (csrc/stem_fused.hip,
k_stem2x<U8, ALN, true>); the stem_int8 option of lfd_amd/engine_i8.py.  tests/test_stem_i8_host.py keeps the
reference honest on the CPU, tests/test_gpu_stem_i8_exact.py compares the kernels with it.

The reference: the float64 stem chain of stem_cases.py (imported, not restated), rounded to fp16 as the fp16 entry point stores
it, then the quantise launch's step in fp32 with numpy: q = clip(rint(float32(y16) * float32(inv_scale)), -127, 127), rint half
to even.  On the integer operands of stem_cases.py the chain is exact, and with a power-of-two inv_scale so is the product: the
kernel must equal the reference in every bit.  The integer outputs reach about 150 behind the pair and about 600 behind the
four-conv chain: inv_scale = 1/2 puts every odd output (a quarter of all) exactly on x.5, inv_scale = 2 clamps every output
above 63; the integer cases run with both."""
import collections

import numpy
import torch

import stem_cases as S

QMAX = 127
FILL = -128                 # a value the clamp never produces: what an unwritten output byte still holds
INT_INV_SCALES = (0.5, 2.0)  # powers of two: exact products; ties on x.5 with the first, the clamp with the second


def quantize_ref(y, inv_scale):
    """y: the stem chain's output in float64 / float32 (any shape, torch or numpy), NOT rounded -> numpy int8 of that shape:
    round to fp16 (through fp32, as stem_cases compares), then one fp32 multiply, rint (half to even), clamp"""
    if isinstance(y, torch.Tensor):
        y = y.detach().cpu().numpy()
    y16 = numpy.asarray(y).astype(numpy.float32).astype(numpy.float16)
    p = y16.astype(numpy.float32) * numpy.float32(inv_scale)
    assert p.dtype == numpy.float32
    return numpy.clip(numpy.rint(p), -QMAX, QMAX).astype(numpy.int8)


def stem_i8_ref(values, stages, inv_scale, chunk=128):
    """values NHWC float [n, h, w, 3], stages [(w OIHW, b, stride)] -> numpy int8 [n, oh, ow, c]: stem_cases.stem_ref in float64
    (on the device of `values`), then quantize_ref"""
    return quantize_ref(S.ref_in_chunks(values, stages, chunk=chunk), inv_scale)


# ------------------------------------------------------------------------------------------------ instances and shapes
PAIR_INSTANCES = [S.Inst('stem', 64, f, 1, 0) for f in (S.FMT_F32, S.FMT_F16, S.FMT_U8)]       # lfd_stem_conv_i8: all three formats
X2_INSTANCES = [S.Inst('stem2x', 64, f, 1, a) for f in (S.FMT_F16, S.FMT_U8) for a in (1, 0)]  # lfd_stem_faster_fused_i8: <U8, ALN>

# raw frames (n, h, w) of lfd_stem_conv_i8; output tile 4 x 32, grid min(tiles, 2048)
#   1 x 1; 8 x 64 = exactly one tile; 9 x 65 = one output pixel past the tile both ways; two ragged frames;
#   8 of 256 x 768 = 3072 tiles, 1.5 per workgroup
PAIR_SHAPES = [(1, 1, 1), (1, 8, 64), (1, 9, 65), (2, 37, 53), (8, 256, 768)]

# lfd_stem_faster_fused_i8; output tile 4 x 32 at stride 4, grid min(tiles rounded up to 8, 256).  route as in stem_cases.Case:
# 'aligned' (W % 8 == 0, 16-byte base: k_stem2x<., true>), 'knob' (X2_ALN = 0), 'misaligned' (fp16 frame 2 bytes past a 16-byte
# boundary), 'width' (W % 8 != 0): the last three reach k_stem2x<., false>
X2Case = collections.namedtuple('X2Case', 'n h w route stagger')
X2_ONE_PIXEL = X2Case(1, 1, 1, 'width', 0)
X2_ONE_TILE = X2Case(1, 16, 128, 'aligned', 0)
X2_PAST_TILE = X2Case(1, 17, 129, 'width', 0)                      # map 5 x 33: one output pixel past the tile both ways
X2_896 = X2Case(4, 448, 1024, 'aligned', 0)                         # map 112 x 256 = 28 x 8 tiles, x 4 = 896 = 3.5 per workgroup
X2_STAGGER = X2Case(*S.X2_C, 'aligned', 0)                          # 700 x 17 x 264: 4200 tiles >= 16 * 256
X2_WIDTH = X2Case(2, 37, 259, 'width', 0)                           # a width that is no multiple of 8, ragged maps


def x2_cases(inst):
    """the cases of one <U8, ALN> instantiation"""
    if inst.aln:
        return [X2_ONE_TILE, X2_896, X2_STAGGER, X2_STAGGER._replace(stagger=1)]
    general = 'misaligned' if inst.fmt == S.FMT_F16 else 'knob'
    return [X2_ONE_PIXEL, X2_PAST_TILE, X2_WIDTH, X2_ONE_TILE._replace(route=general), X2_896._replace(route=general),
            X2_STAGGER._replace(route=general), X2_STAGGER._replace(route=general, stagger=1)]


def x2_case_id(c):
    return '%dx%dx%d_%s%s' % (c.n, c.h, c.w, c.route, '_stagger' if c.stagger else '')


def as_case(inst, c):
    """-> a stem_cases.Case (for its seeds, knobs and launch geometry)"""
    if inst.kernel == 'stem':
        return S.Case(inst, 'i8', c[0], c[1], c[2], 'aligned', 0)
    return S.Case(inst, 'i8', c.n, c.h, c.w, c.route, c.stagger)
