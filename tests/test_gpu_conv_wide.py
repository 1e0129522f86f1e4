"""csrc/conv_wide.hip (every conv with cin or cout above 128, and the four <= 128 layers of FastBlock / FastestBlock bodies that
conv_dispatch routes there), against the float64 reference of
tests/golden/conv_cases.py on the cases of tests/golden/conv_wide_cases.py -- the method of tests/test_gpu_conv_exact.py:

On INTEGER operands the kernel must equal the reference bit for bit (torch.equal), with and without ReLU, the output placed in
a sentinel-guarded buffer whose guards stay untouched, and a second run gives the same bits.  Maps: 2 x 9 x 11, 2 x 8 x 10, one
pixel, and a walk map with about 1.5 tiles per workgroup of the capped grid.  On Gaussian operands the gate is
CC.GAUSS_GATE * max(|ref|, 1)."""
import pytest
import torch

import conv_cases as CC
import conv_wide_cases as WC
from lfd_amd import ops

pytestmark = pytest.mark.gpu

SENTINEL = -12344.0            # an fp16 value no case produces (|outputs| <= 2048)


class Guarded(object):
    """an output placed in the middle of a sentinel-filled buffer: one image's worth of guard on each side, 16-byte aligned"""

    def __init__(self, shape):
        n = 1
        for s in shape:
            n *= s
        self.guard = -(-(n // shape[0]) // 8) * 8
        self.buf = torch.full((n + 2 * self.guard,), SENTINEL, dtype=torch.float16, device='cuda')
        self.view = self.buf[self.guard:self.guard + n].view(shape)
        assert self.view.data_ptr() % 16 == 0

    def untouched(self):
        g = self.guard
        return bool((self.buf[:g] == SENTINEL).all()) and bool((self.buf[-g:] == SENTINEL).all())


def _cuda(o):
    return CC.Operands(*[None if t is None else t.cuda() for t in o])


def _run(c, d, wp, relu, out=None):
    return ops.conv2d_nhwc(d.x, wp, d.b, c.cin, c.cout, c.ks, c.stride, bool(relu), residual=d.res if c.res else None, out=out)


def _explain(got, ref, c):
    bad = (got.double() != ref).nonzero()
    img, oy, ox, ch = bad[0].tolist()
    return ('%s: %d of %d elements differ; first at image %d pixel (%d, %d) channel %d: got %s, reference %s'
            % (WC.case_id(c), bad.size(0), ref.numel(), img, oy, ox, ch, float(got[img, oy, ox, ch]), float(ref[img, oy, ox, ch])))


def _exact(c):
    o = WC.int_operands(c)
    d = _cuda(o)
    wp = ops.pack_conv_weight(o.w).cuda()
    oh, ow = CC.out_hw(c.h, c.w, c.ks, c.stride)
    ref0 = WC.case_ref(c, d, 0)
    assert float(ref0.abs().max()) <= CC.F16_EXACT
    for relu in (0, 1):
        g = Guarded((c.n, oh, ow, c.cout))
        got = _run(c, d, wp, relu, out=g.view)
        torch.cuda.synchronize()
        ref = ref0.relu() if relu else ref0
        assert got.shape == ref.shape
        assert torch.equal(got.double(), ref), _explain(got, ref, c)
        assert g.untouched()
        assert torch.equal(_run(c, d, wp, relu), got)           # the same bits on a second run


@pytest.mark.parametrize('c', WC.wide_cases(), ids=WC.case_id)
def test_wide_conv_is_exact_on_integer_operands(c):
    if c.kind == 'walk':
        _, _, nt, gx = WC.launch(c.n, *CC.out_hw(c.h, c.w, c.ks, c.stride), c.cout)
        assert gx < nt <= 2 * gx                                # some workgroups run two tiles, some one
    _exact(c)


@pytest.mark.parametrize('c', [c for c in WC.wide_cases() if c.kind in ('9x11', 'walk')], ids=WC.case_id)
def test_passes_the_gate_on_gaussian_operands(c):
    o = WC.gauss_operands(c)
    d = _cuda(o)
    got = _run(c, d, ops.pack_conv_weight(o.w).cuda(), 0)
    ref = WC.case_ref(c, d, 0)
    ratio = float(((got.double() - ref).abs() / (CC.GAUSS_GATE * ref.abs().clamp(min=1.0))).max())
    print('GATE %s worst_error_over_gate=%.3f' % (WC.case_id(c), ratio))
    assert ratio <= 1.0


def test_supported_answers_like_the_launch():
    """lfd_conv2d_nhwc_f16_supported and the real call agree: every case's key is supported; 640 channels, 160 inputs, a
    chained 1x1 on a wide layer and a residual on a wide stride-2 layer are refused loudly"""
    for s in WC.WIDE_SHAPES + WC.ROUTED_SHAPES:
        assert ops.conv2d_supported(s[0], s[1], s[2], s[3])
    z = lambda *s: torch.zeros(s, dtype=torch.float16, device='cuda')       # noqa: E731
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device='cuda')       # noqa: E731
    assert not ops.conv2d_supported(640, 128, 1, 1) and not ops.conv2d_supported(128, 640, 1, 1)
    assert not ops.conv2d_supported(160, 256, 1, 1) and not ops.conv2d_supported(256, 256, 3, 2, tail=True)
    with pytest.raises(RuntimeError, match='unsupported'):
        ops.conv2d_nhwc(z(1, 4, 4, 640), z(4, 40, 64, 8), f(128), 640, 128, 1, 1, True)
    with pytest.raises(RuntimeError, match='unsupported'):
        ops.conv2d_nhwc(z(1, 4, 4, 160), z(8, 10, 64, 8), f(256), 160, 256, 1, 1, True)
    with pytest.raises(RuntimeError, match='unsupported'):
        ops.conv2d_nhwc(z(1, 8, 8, 256), z(8, 144, 64, 8), f(256), 256, 256, 3, 2, True, tail=(z(8, 16, 64, 8), f(256), True))
    with pytest.raises(RuntimeError, match='unsupported'):
        ops.conv2d_nhwc(z(1, 8, 8, 256), z(8, 144, 64, 8), f(256), 256, 256, 3, 2, True, residual=z(1, 4, 4, 256))
