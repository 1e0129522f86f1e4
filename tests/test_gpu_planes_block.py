"""lfd_pl_block64 (csrc/planes_block.hip, k_pl_blk64): a 64-channel residual block of the planes mode (lfd_resnet.py:96-154
without a downsample branch) in one launch, against
  * two lfd_pl_conv2d launches (conv1, then conv2 with the residual) -- bit for bit, at the maps of 1080p frames and odd shapes;
  * float64 PyTorch of the block on the values the planes hold;
  * the whole network with LFD_P2_BLOCK=0 (two launches per block) -- identical cls / reg;
  * itself under concurrent work (the rings are ordered by one workgroup barrier per step);
and its argument checks."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

from lfd_amd import _lib, configs, engine_p2, ops
from lfd_amd._lib import check, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu


def _block_inputs(seed, n, h, w):
    g = torch.Generator().manual_seed(seed)
    xp = engine_p2.to_planes(torch.randn(n, h, w, 64, generator=g)).cuda()
    w1 = torch.randn(64, 64, 3, 3, generator=g) * (1.0 / 576 ** 0.5)
    w2 = torch.randn(64, 64, 3, 3, generator=g) * (1.0 / 576 ** 0.5)
    b1, b2 = torch.randn(64, generator=g) * 0.1, torch.randn(64, generator=g) * 0.1
    return xp, w1, b1, w2, b2


def _packed(w1, b1, w2, b2):
    return [engine_p2.pack_planes_weight(w1).cuda(), engine_p2._pad_bias(b1, 128).cuda(),
            engine_p2.pack_planes_weight(w2).cuda(), engine_p2._pad_bias(b2, 128).cuda()]


def _fused(xp, keep, out=None):
    n, h, w = xp.shape[1:4]
    if out is None:
        out = torch.full_like(xp, float('nan'))
    check(lib().lfd_pl_block64(n, h, w, ptr(xp), xp[0].numel(), ptr(out), out[0].numel(), *[ptr(k) for k in keep],
                               ptr(ops.zero_line(xp.device)), stream_ptr()), 'lfd_pl_block64')
    return out


def _conv(xp, wp, bp, res, out):
    d = _lib.PlConvDesc()
    d.n, d.h, d.w = xp.shape[1:4]
    d.cin, d.cout, d.ks, d.stride, d.relu = 64, 64, 3, 1, 1
    d.in_plane_halfs, d.out_plane_halfs = xp[0].numel(), out[0].numel()
    if res is not None:
        d.res_plane_halfs = res[0].numel()
    check(lib().lfd_pl_conv2d(C.byref(d), ptr(xp), ptr(out), ptr(wp), ptr(bp), ptr(res), None, None, None, None, None, None, None, None,
                              None, None, None, None, ptr(ops.zero_line(xp.device)), stream_ptr()), 'lfd_pl_conv2d')


def _two_launches(xp, keep):
    assert _lib.tune('PL_C3') == 2
    mid, out = torch.full_like(xp, float('nan')), torch.full_like(xp, float('nan'))
    _conv(xp, keep[0], keep[1], None, mid)
    _conv(mid, keep[2], keep[3], xp, out)
    return out


_SHAPES = [(n, h, w) for n in (1, 2, 8) for h, w in ((135, 240), (68, 120), (34, 60))] + \
          [(n, h, w) for n in (1, 2) for h, w in ((1, 1), (7, 13), (33, 61), (135, 241))]


@pytest.mark.parametrize('n,h,w', _SHAPES)
def test_pl_block64_equals_two_conv_launches(n, h, w):
    xp, w1, b1, w2, b2 = _block_inputs(n * 1000 + h + w, n, h, w)
    keep = _packed(w1, b1, w2, b2)
    ref = _two_launches(xp, keep)
    got = _fused(xp, keep)
    torch.cuda.synchronize()
    assert not torch.isnan(got.float()).any()
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16)), 'max diff %g' % float(
        (engine_p2.from_planes(got.float()) - engine_p2.from_planes(ref.float())).abs().max())


@pytest.mark.parametrize('n,h,w', [(2, 19, 37), (1, 70, 130), (2, 5, 3)])
def test_pl_block64_vs_float64(n, h, w):
    xp, w1, b1, w2, b2 = _block_inputs(7 + h * w, n, h, w)
    got = engine_p2.from_planes(_fused(xp, _packed(w1, b1, w2, b2)).cpu()).double()
    x = engine_p2.from_planes(xp.cpu()).double().permute(0, 3, 1, 2)
    m = F.conv2d(x, w1.double(), b1.double(), padding=1).relu()
    y = (F.conv2d(m, w2.double(), b2.double(), padding=1) + x).relu().permute(0, 2, 3, 1)
    err, mag = float((got - y).abs().max()), float(y.abs().max())
    print('block vs float64: %.2e (max |y| %.2f)' % (err, mag))
    assert err <= 1e-5 * max(1.0, mag)


def test_pl_block64_is_deterministic_under_concurrent_work():
    xp, w1, b1, w2, b2 = _block_inputs(99, 3, 135, 240)
    keep = _packed(w1, b1, w2, b2)
    out = torch.empty_like(xp)

    def run():
        out.fill_(float('nan'))
        _fused(xp, keep, out)
        torch.cuda.synchronize()
    run()
    ref = out.clone()
    assert not torch.isnan(ref.float()).any()
    side, junk = torch.cuda.Stream(), torch.rand(2048, 2048, device='cuda')
    for i in range(30):
        if i % 2 == 0:
            with torch.cuda.stream(side):
                junk = (junk @ junk).clamp_(-1, 1)
        run()
        assert torch.equal(out.view(torch.int16), ref.view(torch.int16)), 'launch %d differs from the first one' % i
    torch.cuda.synchronize()


def test_pl_block64_argument_checks():
    xp, w1, b1, w2, b2 = _block_inputs(3, 1, 8, 8)
    keep = [ptr(k) for k in _packed(w1, b1, w2, b2)]
    out = torch.empty_like(xp)
    z, sp, L = ptr(ops.zero_line(xp.device)), stream_ptr(), lib()
    ok = (1, 8, 8, ptr(xp), xp[0].numel(), ptr(out), out[0].numel())
    assert L.lfd_pl_block64(*ok, *keep, z, sp) == 0
    assert L.lfd_pl_block64(0, 8, 8, *ok[3:], *keep, z, sp) == -1                                  # n < 1
    assert L.lfd_pl_block64(*ok, None, *keep[1:], z, sp) == -1                                     # null filter
    assert L.lfd_pl_block64(*ok, *keep, None, sp) == -1                                            # null zero line
    assert L.lfd_pl_block64(1, 8, 8, ptr(xp), xp[0].numel() - 8, ptr(out), out[0].numel(), *keep, z, sp) == -1   # short plane
    assert L.lfd_pl_block64(1, 8, 8, ptr(xp), xp[0].numel(), ptr(xp), xp[0].numel(), *keep, z, sp) == -1         # in place
    assert L.lfd_pl_block64(1, 8, 8, xp.data_ptr() + 2, xp[0].numel(), ptr(out), out[0].numel(), *keep, z, sp) == -1
    assert L.lfd_pl_block64(1, 65536, 65536, ptr(xp), 1 << 40, ptr(out), 1 << 40, *keep, z, sp) == -4   # beyond 32-bit offsets
    torch.cuda.synchronize()


@pytest.mark.parametrize('n', [8, 1])
def test_network_fused_blocks_equal_two_launches(n):
    """whole network, 1080p frames: LFD_P2_BLOCK=0 (two launches per block) == the default (one), bit for bit"""
    m = configs.build_model('WIDERFACE_LFD_S')
    configs.perturb_weights(m)
    m.eval().cuda()
    m.precision = 'fp32_storage'
    x = (torch.rand(n, 3, 1080, 1920, generator=torch.Generator().manual_seed(11)) * 2 - 1).cuda()
    from lfd_amd import engine_p32
    with torch.no_grad():
        plan = engine_p32.get_plan(m, x.device)
        assert isinstance(plan, engine_p2.PlanesPlan) and len(plan.block_pairs) >= 1
        c, r = [t.clone() for t in m(x)]
        os.environ['LFD_P2_BLOCK'] = '0'
        try:
            c0, r0 = m(x)
        finally:
            del os.environ['LFD_P2_BLOCK']
    assert torch.equal(c, c0) and torch.equal(r, r0)
