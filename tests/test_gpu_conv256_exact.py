"""csrc/conv256.hip (lfd_conv256_nhwc_f16: the large-map 3x3 / 1x1 conv from 256 channels) against the float64 reference of
tests/golden/conv_cases.py on the cases of tests/golden/conv256_cases.py -- the method of tests/test_gpu_conv_wide.py:

On INTEGER operands both output forms (fp16; the un-rounded fp32 accumulators) must equal the reference bit for bit, with and
without ReLU, the output placed in a sentinel-guarded buffer whose guards stay untouched, and a second launch gives the same
bits.  On Gaussian operands the gate is the project's per-launch tolerance: |got - ref| <= 0.5005 ulp16(ref) + 2^-19 sum |x||w|
for the fp16 form, the second term alone for the fp32 form.  The sibling engine's two routes for one layer (this kernel,
csrc/conv_wide.hip) agree bit for bit on the integer operands and within twice the tolerance on the Gaussian ones."""
import pytest
import torch

import conv_cases as CC
import conv256_cases as K
import resnet_cases as RC
from lfd_amd import engine_sibling, ops

pytestmark = pytest.mark.gpu

SENTINEL = -12344.0            # a value no case produces (|outputs| <= 2048), exact in fp16 and fp32


class Guarded(object):
    """an output placed in the middle of a sentinel-filled buffer: one image's worth of guard on each side, 16-byte aligned"""

    def __init__(self, shape, dtype):
        n = 1
        for s in shape:
            n *= s
        self.guard = -(-(n // shape[0]) // 8) * 8
        self.buf = torch.full((n + 2 * self.guard,), SENTINEL, dtype=dtype, device='cuda')
        self.view = self.buf[self.guard:self.guard + n].view(shape)
        assert self.view.data_ptr() % 16 == 0

    def untouched(self):
        g = self.guard
        return bool((self.buf[:g] == SENTINEL).all()) and bool((self.buf[-g:] == SENTINEL).all())


def _cuda(o):
    return CC.Operands(*[None if t is None else t.cuda() for t in o])


def _run(c, d, wp, relu, f32, out=None):
    return ops.conv256_nhwc(d.x, wp, d.b, c.cout, c.ks, relu=bool(relu), f32out=f32, out=out)


def _forms(c):
    return (True,) if c.ks == 1 else (False, True)       # the 1x1 instance exists for fp32 logits only


def _explain(got, ref, c, f32):
    bad = (got.double() != ref).nonzero()
    img, oy, ox, ch = bad[0].tolist()
    return ('%s %s: %d of %d elements differ; first at image %d pixel (%d, %d) channel %d: got %s, reference %s'
            % (K.case_id(c), 'fp32' if f32 else 'fp16', bad.size(0), ref.numel(), img, oy, ox, ch, float(got[img, oy, ox, ch]),
               float(ref[img, oy, ox, ch])))


@pytest.mark.parametrize('c', K.cases(), ids=K.case_id)
def test_conv256_is_exact_on_integer_operands(c):
    if c.kind == 'walk':
        _, _, nt, grid = K.launch(c.n, c.h, c.w)
        assert grid < nt <= 2 * grid                              # some workgroups run two tiles, some one
    o = K.int_operands(c)
    d = _cuda(o)
    wp = ops.pack_conv_weight(o.w).cuda()
    ref0 = K.case_ref(c, d, 0)
    assert float(ref0.abs().max()) <= CC.F16_EXACT
    for f32 in _forms(c):
        for relu in (0, 1):
            g = Guarded((c.n, c.h, c.w, c.cout), torch.float32 if f32 else torch.float16)
            got = _run(c, d, wp, relu, f32, out=g.view)
            torch.cuda.synchronize()
            ref = ref0.relu() if relu else ref0
            assert got.shape == ref.shape and got.dtype == (torch.float32 if f32 else torch.float16)
            assert torch.equal(got.double(), ref), _explain(got, ref, c, f32)
            assert g.untouched()
            assert torch.equal(_run(c, d, wp, relu, f32), got)    # the same bits on a second launch


def _tolerance(ref, mag, f32):
    tol = 2.0 ** -19 * mag
    return tol if f32 else tol + 0.5005 * RC.ulp16(ref)


@pytest.mark.parametrize('c', [c for c in K.cases() if c.kind in ('edge', 'walk')], ids=K.case_id)
def test_conv256_passes_the_per_launch_tolerance_on_gaussian_operands(c):
    o = K.gauss_operands(c)
    d = _cuda(o)
    wp = ops.pack_conv_weight(o.w).cuda()
    ref = K.case_ref(c, d, 0)
    mag = K.abs_ref(d)
    for f32 in _forms(c):
        got = _run(c, d, wp, 0, f32)
        ratio = float(((got.double() - ref).abs() / _tolerance(ref, mag, f32)).max())
        print('TOL %s %s worst_error_over_tolerance=%.3f' % (K.case_id(c), 'fp32' if f32 else 'fp16', ratio))
        assert ratio <= 1.0


def _engine_layer(o, cout):
    conv = torch.nn.Conv2d(K.CIN, cout, 3, 1, 1)
    with torch.no_grad():
        conv.weight.copy_(o.w)
        conv.bias.copy_(o.b)
        return engine_sibling._Conv(conv, None, True, K.CIN, torch.device('cuda'))


@pytest.mark.parametrize('cout', (256, 96))
def test_the_two_routes_of_the_engine_agree(cout, monkeypatch):
    """one engine layer (3x3 stride 1, 256 -> cout, ReLU) on the edge map, routed to csrc/conv256.hip and to csrc/conv_wide.hip by
    the crossover constant alone"""
    c = K.Case(cout, 3, 'edge', *dict(K.MAPS)['edge'])
    pixels = c.n * c.h * c.w
    for kind in ('int', 'gauss'):
        o = K.int_operands(c) if kind == 'int' else K.gauss_operands(c)
        d = _cuda(o)
        layer = _engine_layer(o, cout)
        assert layer.cout == (256 if cout > 128 else 128)         # the engine's padding (engine.pad_channels)
        monkeypatch.setattr(engine_sibling, 'CONV256_MIN_PIXELS', pixels)
        assert layer.route(pixels) == 'conv256'
        a = layer(d.x)
        monkeypatch.setattr(engine_sibling, 'CONV256_MIN_PIXELS', pixels + 1)
        assert layer.route(pixels) == 'conv_wide'
        b = layer(d.x)
        assert a.shape == b.shape == (c.n, c.h, c.w, layer.cout) and not bool(a[..., cout:].any())
        if kind == 'int':
            assert torch.equal(a, b)
            assert torch.equal(a[..., :cout].double(), K.case_ref(c, d, 1))
        else:
            ref = K.case_ref(c, d, 1)
            tol = _tolerance(ref, K.abs_ref(d), False)
            ratio = float(((a[..., :cout].double() - b[..., :cout].double()).abs() / (2 * tol)).max())
            print('ROUTES 256to%d worst_difference_over_twice_tolerance=%.3f' % (cout, ratio))
            assert ratio <= 1.0


def test_supported_answers_like_the_launch():
    assert ops.conv256_supported(256, 256, 3) and ops.conv256_supported(256, 32, 3, True) and ops.conv256_supported(256, 128, 1, True)
    assert not ops.conv256_supported(128, 128, 3) and not ops.conv256_supported(256, 288, 3) and not ops.conv256_supported(256, 48, 3)
    assert not ops.conv256_supported(256, 256, 1) and not ops.conv256_supported(256, 256, 5)
    z = lambda *s: torch.zeros(s, dtype=torch.float16, device='cuda')       # noqa: E731
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device='cuda')       # noqa: E731
    with pytest.raises(RuntimeError, match='unsupported'):
        ops.conv256_nhwc(z(1, 4, 4, 256), z(9, 144, 64, 8), f(288), 288, 3)
    with pytest.raises(RuntimeError, match='unsupported'):
        ops.conv256_nhwc(z(1, 4, 4, 256), z(8, 16, 64, 8), f(256), 256, 1)
    with pytest.raises(RuntimeError, match='256 channels'):
        ops.conv256_nhwc(z(1, 4, 4, 128), z(8, 72, 64, 8), f(256), 256, 3)
