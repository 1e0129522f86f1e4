"""lfd_stem7_conv_f16 (csrc/stem7.hip) alone through the C ABI against a float64 conv of the same operands
(tests/golden/resnet_cases.py): bit equality on integer operands (fp32 NCHW and fp16 NHWC frames) and on uint8 frames with
filters that keep every fp32 partial sum exact; the project's per-launch tolerance on Gaussian operands.  Maps: one tile corner
(1 x 7 x 7), ragged in both directions (2 x 37 x 53), one pixel, and a walk that gives every workgroup of the capped grid 1.5
tiles.  Every run: the guard halfs around the output untouched, no poison left inside, the same bits on a second launch, a
non-zero bias and negative pre-activations (ReLU matters)."""
import functools

import pytest
import torch

import resnet_cases as RC
from lfd_amd import _lib, engine_resnet

pytestmark = pytest.mark.gpu

GUARD = 4096                   # halfs on either side of the output (a multiple of 8: the output stays 16-byte aligned)
POISON = -12344.0              # an fp16 value no case produces


def _run(frame, fmt, n, h, w, wt, b):
    """-> out [n, oh, ow, 64] fp16 (a view into a poisoned buffer whose guards were checked)"""
    oh, ow = RC.out_hw(h, w)
    wp = engine_resnet.pack_stem7_weight(wt).cuda()
    bias = b.float().cuda().contiguous()
    x = frame.cuda()
    size = n * oh * ow * 64
    outs = []
    for _ in range(2):
        buf = torch.full((size + 2 * GUARD,), POISON, dtype=torch.float16, device='cuda')
        out = buf[GUARD:GUARD + size]
        _lib.check(_lib.lib().lfd_stem7_conv_f16(_lib.ptr(x), fmt, n, h, w, _lib.ptr(wp), _lib.ptr(bias), _lib.ptr(out),
                                                 _lib.stream_ptr()), 'lfd_stem7_conv_f16')
        torch.cuda.synchronize()
        assert bool((buf[:GUARD] == POISON).all()) and bool((buf[GUARD + size:] == POISON).all()), 'a guard was written'
        assert not bool((out == POISON).any()), 'an output element was not written'
        outs.append(out.view(n, oh, ow, 64))
    assert torch.equal(outs[0], outs[1]), 'two launches, different bits'
    return outs[0]


@functools.lru_cache(maxsize=2)
def _int_case(kind):
    """integer operands and their float64 pre-activation, shared by the two frame formats"""
    shape = RC.SHAPES[kind]
    x, wt, b = RC.int_operands(shape, 100 + len(kind))
    pre = RC.conv_ref(x.cuda(), wt, b)
    return x, wt, b, pre


@pytest.mark.parametrize('fmt', [RC.FMT_F32, RC.FMT_F16], ids=lambda f: RC.FMT_NAMES[f])
@pytest.mark.parametrize('kind', list(RC.SHAPES))
def test_integer_operands_are_exact(kind, fmt):
    n, h, w = RC.SHAPES[kind]
    if kind == 'walk':
        assert 2 * RC.ntiles(n, h, w) == 3 * RC.MAX_WGS
    x, wt, b, pre = _int_case(kind)
    assert float(pre.abs().max()) <= 2048 and bool(b.ne(0).all())
    if kind != 'pixel':
        assert bool((pre < 0).any()) and bool((pre > 0).any())
    got = _run(RC.to_frame(x, fmt), fmt, n, h, w, wt, b)
    assert torch.equal(got, pre.relu().half())


@pytest.mark.parametrize('kind', ['corner', 'ragged', 'pixel'])
def test_uint8_frames_are_exact(kind):
    """the normalisation fused into the load: the float64 conv of half((v / 255 - 0.5) / 0.5), rounded once to fp16"""
    n, h, w = RC.SHAPES[kind]
    codes, wt, b = RC.u8_operands((n, h, w), 200 + len(kind))
    seen = RC.normalize_u8(codes)
    pre = RC.conv_ref(seen.cuda(), wt, b)
    assert torch.equal(pre.float().double(), pre), 'the operands keep the sums exact in fp32'
    if kind != 'pixel':
        assert bool((pre < 0).any()) and bool((pre > 0).any())
    got = _run(RC.to_frame(codes, RC.FMT_U8), RC.FMT_U8, n, h, w, wt, b)
    assert torch.equal(got, pre.relu().half())


def test_uint8_equals_its_normalised_fp16_twin_on_gaussian_filters():
    n, h, w = RC.SHAPES['ragged']
    codes, _, _ = RC.u8_operands((n, h, w), 31)
    _, wt, b = RC.gauss_operands((n, h, w), 32)
    a = _run(RC.to_frame(codes, RC.FMT_U8), RC.FMT_U8, n, h, w, wt, b)
    twin = RC.normalize_u8(codes)
    assert torch.equal(a, _run(twin.contiguous(), RC.FMT_F16, n, h, w, wt, b))


@pytest.mark.parametrize('fmt', [RC.FMT_F32, RC.FMT_F16, RC.FMT_U8], ids=lambda f: RC.FMT_NAMES[f])
def test_gaussian_operands_pass_the_per_launch_tolerance(fmt):
    n, h, w = RC.SHAPES['ragged']
    x, wt, b = RC.gauss_operands((n, h, w), 300)
    if fmt == RC.FMT_U8:
        codes, _, _ = RC.u8_operands((n, h, w), 301)
        frame, x = codes, RC.normalize_u8(codes).float()
    else:
        frame = RC.to_frame(x, fmt)
    pre = RC.conv_ref(x.cuda(), wt, b)
    mag = RC.conv_ref(x.abs().cuda(), wt.abs(), b.abs())
    ref = pre.relu()
    got = _run(frame, fmt, n, h, w, wt, b)
    tol = 0.5005 * RC.ulp16(ref) + 2.0 ** -19 * mag
    ratio = float(((got.double() - ref).abs() / tol).max())
    print('STEM7 gauss %s: worst |got - ref| / tolerance %.3f' % (RC.FMT_NAMES[fmt], ratio))
    assert bool((pre < 0).any()) and ratio <= 1.0
