"""Grayscale (input_channels=1) models on the inference path, host side (no GPU): the three launch plans build for the gray
twins of the named configurations, the RGB plans are untouched, the input-format rules, the packed gray stem weights, and the
fp32 oracle against the reference's own gray forward (tests/golden/make_golden_gray.py)."""
import hashlib

import numpy as np
import pytest
import torch

from conftest import load_golden
from lfd_amd import configs, engine, engine_p2, engine_p32
from oracle import net_oracle

CPU = torch.device('cpu')
PLANE_TWINS = ['WIDERFACE_LFD_XS', 'WIDERFACE_LFD_S', 'WIDERFACE_LFD_M', 'WIDERFACE_LFD_L', 'TT100K_LFD_S', 'TT100K_LFD_L']
TL_TWINS = ['TL_LFD_S', 'TL_LFD_L']


def _gray(name):
    m = configs.build_model(name, input_channels=1)
    m.eval()
    return m


@pytest.mark.parametrize('name', PLANE_TWINS + TL_TWINS)
def test_gray_twin_plans_build(name):
    m = _gray(name)
    assert m._backbone._input_channels == 1
    p = engine.EnginePlan(m._backbone, m._neck, m._head, CPU)
    assert p.input_channels == 1 and p.stem_fused is None
    assert tuple(p.stem_first[1].shape) == (p.stem_first[0] // 32, 64, 8)
    pp = engine_p32.PrecisePlan(m, CPU)
    assert pp.ops[0].cin == 1 and pp.ops[0].patch
    if name in TL_TWINS:       # as their RGB versions: no plane kernel for the BatchNorm head towers
        with pytest.raises(engine_p2.Unsupported):
            engine_p2.PlanesPlan(m, CPU)
        assert isinstance(engine_p32.get_plan(m, CPU), engine_p32.PrecisePlan)
    else:
        p2 = engine_p2.PlanesPlan(m, CPU)
        assert p2.ops[0].kind == 'stem_gray' and p2.stem2x is None
        assert isinstance(engine_p32.get_plan(m, CPU), engine_p2.PlanesPlan)


@pytest.mark.parametrize('name', ['WIDERFACE_LFD_S', 'TT100K_LFD_S', 'WIDERFACE_LFD_XS'])
def test_gray_faster_stem_plane_plan(name):
    """a gray 'faster' stem: the gray stem op, then the second pair on lfd_pl_conv2d (3x3 s2 with its chained 1x1)"""
    m = _gray(name)
    assert m._backbone._stem_mode == 'faster'
    p2 = engine_p2.PlanesPlan(m, CPU)
    o, c = p2.ops[0], p2.ops[1]
    assert o.kind == 'stem_gray' and o.channels == configs.ARCHS[name]['stem_channels']
    assert tuple(o.w1.shape) == (2, o.channels // 32, 64, 8)
    assert c.kind == 'conv' and (c.cin, c.ks, c.stride) == (o.channels, 3, 2) and c.tail is not None and c.src == o.dst
    assert p2.stem2x is None


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b)
    if isinstance(a, (tuple, list)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if hasattr(a, '__slots__'):
        return type(a) is type(b) and all(_same(getattr(a, k, None), getattr(b, k, None)) for k in a.__slots__)
    return a == b


@pytest.mark.parametrize('name', sorted(configs.ARCHS))
def test_rgb_plans_are_unchanged(name):
    """input_channels=3 through the new option == the untouched named configuration, launch list for launch list"""
    a, b = configs.build_model(name).eval(), configs.build_model(name, input_channels=3).eval()
    pa, pb = engine.EnginePlan(a._backbone, a._neck, a._head, CPU), engine.EnginePlan(b._backbone, b._neck, b._head, CPU)
    assert pa.input_channels == 3 and pa.stem_first[1].shape == engine.pack_stem_weight(torch.zeros(pa.stem_first[0], 3, 3, 3)).shape
    assert _same(pa.stem_first, pb.stem_first) and _same(pa.stem_fused, pb.stem_fused) and _same(pa.convs, pb.convs)
    qa, qb = engine_p32.PrecisePlan(a, CPU), engine_p32.PrecisePlan(b, CPU)
    assert qa.ops[0].cin == 3 and _same(qa.ops, qb.ops)
    if name not in TL_TWINS:
        ra, rb = engine_p2.PlanesPlan(a, CPU), engine_p2.PlanesPlan(b, CPU)
        assert ra.ops[0].kind == 'stem' and _same(ra.ops, rb.ops) and _same(ra.stem2x, rb.stem2x)


def test_input_format_rules():
    f = engine._input_format
    # RGB (unchanged)
    assert f(torch.zeros(2, 3, 5, 7)) == (0, 2, 5, 7)
    assert f(torch.zeros(2, 5, 7, 3, dtype=torch.float16)) == (1, 2, 5, 7)
    assert f(torch.zeros(2, 5, 7, 3, dtype=torch.uint8)) == (2, 2, 5, 7)
    # gray
    assert f(torch.zeros(2, 1, 5, 7), 1) == (0, 2, 5, 7)
    assert f(torch.zeros(2, 5, 7, 1, dtype=torch.float16), 1) == (1, 2, 5, 7)
    assert f(torch.zeros(2, 5, 7, 1, dtype=torch.uint8), 1) == (2, 2, 5, 7)
    # gray frames for an RGB model and the other way round: RuntimeError naming the expected shapes
    for x in (torch.zeros(2, 1, 5, 7), torch.zeros(2, 5, 7, 1, dtype=torch.float16), torch.zeros(2, 5, 7, 1, dtype=torch.uint8)):
        with pytest.raises(RuntimeError, match=r'\[N,3,H,W\]'):
            f(x)
    for x in (torch.zeros(2, 3, 5, 7), torch.zeros(2, 5, 7, 3, dtype=torch.float16), torch.zeros(2, 5, 7, 3, dtype=torch.uint8),
              torch.zeros(2, 5, 7, 1, dtype=torch.float32), torch.zeros(2, 1, 5, 7, dtype=torch.float16)):
        with pytest.raises(RuntimeError, match=r'\[N,1,H,W\].*\[N,H,W,1\]'):
            f(x, 1)
    with pytest.raises(RuntimeError, match='4-D'):
        f(torch.zeros(1, 5, 7), 1)
    with pytest.raises(RuntimeError, match='unsupported input: NCHW float32'):     # the RGB message stays as it was
        f(torch.zeros(2, 4, 5, 7))
    with pytest.raises(engine.Unsupported):
        f(torch.zeros(2, 2, 5, 7), 2)


def test_other_channel_counts_stay_unsupported():
    m = configs.build_modules(configs.ARCHS['WIDERFACE_LFD_XS'], *_classes(), input_channels=2).eval()
    with pytest.raises(engine.Unsupported):
        engine.EnginePlan(m._backbone, m._neck, m._head, CPU)
    with pytest.raises(engine.Unsupported):
        engine_p32.PrecisePlan(m, CPU)
    with pytest.raises(engine_p2.Unsupported):
        engine_p2.PlanesPlan(m, CPU)


def _classes():
    from lfd_amd.model.backbone import LFDResNet
    from lfd_amd.model.head import LFDHead
    from lfd_amd.model.lfd import LFD
    from lfd_amd.model.losses import CrossEntropyLoss, FocalLoss, IoULoss
    from lfd_amd.model.neck import SimpleNeck
    return LFDResNet, SimpleNeck, LFDHead, LFD, FocalLoss, IoULoss, CrossEntropyLoss


def _gray_weight_numpy(w):
    """restatement of the layout in include/lfd_hip.h: [C/32][64 lanes][8], lane = 32 h + co_l, slot j = tap k = 8 h + j
    (k = 3 ky + kx), zero for k >= 9"""
    c = w.shape[0]
    out = np.zeros((c // 32, 64, 8), np.float16)
    for co in range(c):
        for lane_h in range(2):
            for j in range(8):
                k = 8 * lane_h + j
                if k < 9:
                    out[co // 32, 32 * lane_h + co % 32, j] = np.float16(w[co, 0, k // 3, k % 3])
    return out


@pytest.mark.parametrize('c', [32, 64])
def test_packed_gray_weight_layout(c):
    w = torch.randn(c, 1, 3, 3, generator=torch.Generator().manual_seed(c))
    np.testing.assert_array_equal(engine.pack_stem_gray_weight(w).numpy(), _gray_weight_numpy(w.numpy()))
    pl = engine_p2.pack_planes_stem_gray_weight(w)
    hi = w.half().float()
    lo = (w - hi) * 2048.0
    np.testing.assert_array_equal(pl[0].numpy(), _gray_weight_numpy(hi.numpy()))
    np.testing.assert_array_equal(pl[1].numpy(), _gray_weight_numpy(lo.numpy()))


def test_precise_plan_gray_patch_weight():
    """the fp32-tensor plan's first conv on a gray frame: 9 taps k = dy*3 + dx as the first 9 of one 32-wide k chunk"""
    m = _gray('TL_LFD_S')
    pp = engine_p32.PrecisePlan(m, CPU)
    o = pp.ops[0]
    w = o.ref_w
    assert tuple(w.shape[1:]) == (1, 3, 3)
    w32 = torch.cat([w.reshape(w.shape[0], 9), w.new_zeros(w.shape[0], 23)], 1).reshape(w.shape[0], 32, 1, 1)
    assert torch.equal(o.w, engine_p32.pack_weight(w32))


def _state_sha(sd):
    h = hashlib.sha256()
    for k in sd:
        h.update(k.encode())
        h.update(sd[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


@pytest.mark.parametrize('name', ['WIDERFACE_LFD_S', 'TL_LFD_S'])
def test_net_oracle_vs_reference_gray_forward(name):
    """the package's gray twin reproduces the reference's seeded input_channels=1 weights bit for bit, and the fp32 oracle its
    forward on a [N,1,H,W] batch (the bound of the RGB fixtures)"""
    g = load_golden('ref_model_gray_%s.npz' % name)
    arch = configs.ARCHS[name]
    m = configs.build_model(name, seed=666, input_channels=1)
    assert _state_sha(m.state_dict()) == str(g['sha_init']), 'seeded init differs from the reference'
    configs.perturb_weights(m, seed=1)
    assert _state_sha(m.state_dict()) == str(g['sha'])
    N, H, W = [int(v) for v in g['shape']]
    x = torch.rand(N, 1, H, W, generator=torch.Generator().manual_seed(int(g['x_seed']))) * 2 - 1
    with torch.no_grad():
        cls, reg, sizes = net_oracle.lfd_forward(m.state_dict(), arch, x)
    assert [list(s) for s in sizes] == g['sizes'].tolist()
    np.testing.assert_allclose(cls.numpy(), g['cls'], atol=2e-5, rtol=1e-5)
    np.testing.assert_allclose(reg.numpy(), g['reg'], atol=2e-5, rtol=1e-5)
