"""Grayscale (input_channels=1) models on the MI355X: the gray stem unit (csrc/stem_gray.hip) in both output forms and the
fp32-tensor plan's cin = 1 frame path against float64, then whole gray networks in both precision modes against the oracles,
format / graph / determinism equalities and the public entry points (predict_for_single_image, siblings, the image-parallel
map)."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import net_oracle
from lfd_amd import _lib, configs, engine, engine_p2, engine_p32, ops, parallel
from lfd_amd._lib import check, lib, ptr, stream_ptr

pytestmark = pytest.mark.gpu
PL_TOL = 4e-6     # the gate of test_pl_stem_pair_vs_float64 (relative to max(1, max |y|))

SHAPES = [(2, 45, 71), (1, 37, 131), (3, 1, 1), (2, 2, 3), (1, 4, 1), (2, 3, 4), (1, 19, 33), (2, 64, 128)]


def _frame(fmt, n, h, w, g):
    """(device input, float64 [n,1,h,w] values the kernel sees before any rounding)"""
    if fmt == 0:
        x = torch.rand(n, 1, h, w, generator=g) * 2 - 1
        return x, x.double()
    if fmt == 1:
        x = (torch.rand(n, h, w, 1, generator=g) * 2 - 1).half()
        return x, x.double().permute(0, 3, 1, 2)
    x = torch.randint(0, 256, (n, h, w, 1), generator=g, dtype=torch.uint8)
    return x, ((x.float() / 255 - 0.5) / 0.5).double().permute(0, 3, 1, 2)


def _weights(c, tail, g):
    w1, b1 = torch.randn(c, 1, 3, 3, generator=g) * 0.5, torch.randn(c, generator=g) * 0.1
    w2 = b2 = None
    if tail:
        w2, b2 = torch.randn(c, c, 1, 1, generator=g) * (1.0 / c ** 0.5), torch.randn(c, generator=g) * 0.1
    return w1, b1, w2, b2


def _run_f16(fmt, n, h, w, c, tail, seed):
    g = torch.Generator().manual_seed(seed)
    x, xv = _frame(fmt, n, h, w, g)
    w1, b1, w2, b2 = _weights(c, tail, g)
    w1 = w1.half().float()
    ref = F.conv2d(xv.float().half().double(), w1.double(), b1.double(), stride=2, padding=1).relu()
    keep = [x.cuda(), engine.pack_stem_gray_weight(w1).cuda(), b1.cuda(), None, None]
    if tail:
        w2 = w2.half().float()
        ref = F.conv2d(ref.float().half().double(), w2.double(), b2.double()).relu()
        keep[3], keep[4] = ops.pack_conv_weight(w2).cuda(), b2.cuda()
    out = torch.full((n, (h + 1) // 2, (w + 1) // 2, c), float('nan'), dtype=torch.float16, device='cuda')
    check(lib().lfd_stem_gray_f16(ptr(keep[0]), fmt, n, h, w, c, ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), ptr(keep[4]),
                                  ptr(out), stream_ptr()), 'lfd_stem_gray_f16')
    torch.cuda.synchronize()
    got = out.float().cpu().permute(0, 3, 1, 2).double()
    assert not torch.isnan(got).any(), 'unwritten output'
    # the gate of the RGB lfd_stem_conv_f16 test (tests/test_gpu_conv.py): fp16 output rounding + accumulation noise
    tol = 1.2e-3 * ref.abs().clamp(min=1.0)
    assert bool(((got - ref).abs() <= tol).all()), float((got - ref).abs().max())


def _run_planes(fmt, n, h, w, c, tail, seed):
    g = torch.Generator().manual_seed(seed)
    x, xv = _frame(fmt, n, h, w, g)
    w1, b1, w2, b2 = _weights(c, tail, g)
    xr = engine_p2.from_planes(engine_p2.to_planes(xv.float().permute(0, 2, 3, 1))).double().permute(0, 3, 1, 2)
    ref = F.conv2d(xr, w1.double(), b1.double(), stride=2, padding=1).relu()
    keep = [x.cuda(), engine_p2.pack_planes_stem_gray_weight(w1).cuda(), engine_p2._pad_bias(b1).cuda(), None, None]
    if tail:
        mid = engine_p2.from_planes(engine_p2.to_planes(ref.float().permute(0, 2, 3, 1))).double().permute(0, 3, 1, 2)
        ref = F.conv2d(mid, w2.double(), b2.double()).relu()
        keep[3], keep[4] = engine_p2.pack_planes_weight(w2).cuda(), engine_p2._pad_bias(b2).cuda()
    oh, ow = (h + 1) // 2, (w + 1) // 2
    out = torch.full((2, n, oh, ow, c), float('nan'), dtype=torch.float16, device='cuda')
    check(lib().lfd_pl_stem_gray_pair(ptr(keep[0]), fmt, n, h, w, c, ptr(keep[1]), ptr(keep[2]), ptr(keep[3]), ptr(keep[4]),
                                      ptr(out), out[0].numel(), stream_ptr()), 'lfd_pl_stem_gray_pair')
    torch.cuda.synchronize()
    got = engine_p2.from_planes(out.cpu()).double().permute(0, 3, 1, 2)
    assert not torch.isnan(got).any(), 'unwritten output'
    err, mag = float((got - ref).abs().max()), float(ref.abs().max())
    assert err <= PL_TOL * max(1.0, mag), (err, mag)


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('tail', [True, False])
@pytest.mark.parametrize('c', [32, 64])
@pytest.mark.parametrize('fmt', [0, 1, 2])
def test_stem_gray_f16_vs_float64(fmt, c, tail, shape):
    _run_f16(fmt, *shape, c, tail, seed=fmt * 100 + c + int(tail) + sum(shape))


@pytest.mark.parametrize('shape', SHAPES)
@pytest.mark.parametrize('tail', [True, False])
@pytest.mark.parametrize('c', [32, 64])
@pytest.mark.parametrize('fmt', [0, 1, 2])
def test_pl_stem_gray_pair_vs_float64(fmt, c, tail, shape):
    _run_planes(fmt, *shape, c, tail, seed=fmt * 100 + c + int(tail) + sum(shape))


@pytest.mark.parametrize('fmt', [0, 1, 2])
def test_stem_gray_1080p(fmt):
    _run_f16(fmt, 1, 1080, 1920, 64, True, seed=11)
    _run_planes(fmt, 1, 1080, 1920, 64, True, seed=12)


@pytest.mark.parametrize('tail', [False, True])
@pytest.mark.parametrize('fmt', [0, 1, 2])
def test_p32_conv_gray_frame_vs_float64(fmt, tail):
    """lfd_p32_conv2d_(tail_)nhwc_f32 with cin = 1: the 9 taps of a one-channel frame in one k chunk"""
    g = torch.Generator().manual_seed(40 + fmt)
    n, h, w, c = 2, 37, 53, 64
    x, xv = _frame(fmt, n, h, w, g)
    w1, b1, w2, b2 = _weights(c, tail, g)
    ref = F.conv2d(xv, w1.double(), b1.double(), stride=2, padding=1).relu()
    w32 = torch.cat([w1.reshape(c, 9), w1.new_zeros(c, 23)], 1).reshape(c, 32, 1, 1)
    keep = [x.cuda(), engine_p32.pack_weight(w32).cuda(), engine_p32._pad_bias(b1).cuda()]
    oh, ow = (h + 1) // 2, (w + 1) // 2
    out = torch.full((n, oh, ow, c), float('nan'), device='cuda')
    d = _lib.P32ConvDesc(n, h, w, 1, c, 3, 2, 1, fmt, 0, 0)
    if tail:
        ref = F.conv2d(ref, w2.double(), b2.double()).relu()
        keep += [engine_p32.pack_weight(w2).cuda(), engine_p32._pad_bias(b2).cuda()]
        check(lib().lfd_p32_conv2d_tail_nhwc_f32(C.byref(d), ptr(keep[0]), ptr(out), ptr(keep[1]), ptr(keep[2]), ptr(keep[3]),
                                                 ptr(keep[4]), 1, stream_ptr()), 'lfd_p32_conv2d_tail_nhwc_f32')
    else:
        check(lib().lfd_p32_conv2d_nhwc_f32(C.byref(d), ptr(keep[0]), ptr(out), ptr(keep[1]), ptr(keep[2]), None, None,
                                            stream_ptr()), 'lfd_p32_conv2d_nhwc_f32')
    torch.cuda.synchronize()
    got = out.cpu().double().permute(0, 3, 1, 2)
    err, mag = float((got - ref).abs().max()), float(ref.abs().max())
    assert err <= 1e-5 * max(1.0, mag), (err, mag)
    # cin other than 1 / 3 on the frame path stays unsupported
    d.cin = 2
    assert lib().lfd_p32_conv2d_nhwc_f32(C.byref(d), ptr(keep[0]), ptr(out), ptr(keep[1]), ptr(keep[2]), None, None,
                                         stream_ptr()) == -4


def test_gray_entry_points_check_their_arguments():
    n, h, w, c = 1, 8, 8, 64
    x = torch.zeros(n, h, w, 1, dtype=torch.float16, device='cuda')
    w1 = torch.zeros(2, 2, 64, 8, dtype=torch.float16, device='cuda')
    b = torch.zeros(64, device='cuda')
    w2 = torch.zeros(2, 2, 4, 64, 8, dtype=torch.float16, device='cuda')
    out = torch.zeros(2, n, 4, 4, c, dtype=torch.float16, device='cuda')
    plane = out[0].numel()
    L, sp = lib(), stream_ptr()

    def f16(**k):
        a = dict(x=ptr(x), fmt=1, n=n, h=h, w=w, c=c, w1=ptr(w1), b1=ptr(b), w2=ptr(w2), b2=ptr(b), out=ptr(out))
        a.update(k)
        return L.lfd_stem_gray_f16(a['x'], a['fmt'], a['n'], a['h'], a['w'], a['c'], a['w1'], a['b1'], a['w2'], a['b2'],
                                   a['out'], sp)

    def pl(**k):
        a = dict(x=ptr(x), fmt=1, n=n, h=h, w=w, c=c, w1=ptr(w1), b1=ptr(b), w2=ptr(w2), b2=ptr(b), out=ptr(out), plane=plane)
        a.update(k)
        return L.lfd_pl_stem_gray_pair(a['x'], a['fmt'], a['n'], a['h'], a['w'], a['c'], a['w1'], a['b1'], a['w2'], a['b2'],
                                       a['out'], a['plane'], sp)

    for call in (f16, pl):
        for bad in (dict(x=None), dict(w1=None), dict(b1=None), dict(out=None), dict(b2=None), dict(w2=None)):
            assert call(**bad) == -1, (call.__name__, bad)
        for bad in (dict(n=0), dict(h=0), dict(w=-3)):
            assert call(**bad) == -1, (call.__name__, bad)
        for fmt in (-1, 3, 7):
            assert call(fmt=fmt) == -1, (call.__name__, fmt)
        assert call(out=C.c_void_p(out.data_ptr() + 2)) == -1
        assert call(b1=C.c_void_p(b.data_ptr() + 4)) == -1
        for cc in (16, 48, 128):
            assert call(c=cc) == -4, (call.__name__, cc)
        assert call() == 0
    assert pl(plane=plane + 4) == -1                     # plane stride not a multiple of 8 halfs
    assert pl(plane=plane - 8) == -1                     # planes would overlap
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- whole networks
SMALL = [('WIDERFACE_LFD_XS', (1, 96, 128)), ('WIDERFACE_LFD_S', (2, 135, 241)), ('WIDERFACE_LFD_M', (1, 64, 96)),
         ('WIDERFACE_LFD_L', (1, 100, 156)), ('TT100K_LFD_S', (1, 64, 64)), ('TT100K_LFD_L', (2, 90, 161)),
         ('TL_LFD_L', (1, 128, 192)), ('TL_LFD_S', (1, 96, 160))]


def _model(name):
    m = configs.build_model(name, input_channels=1)
    configs.perturb_weights(m)
    m.eval()
    return m, {k: v.clone() for k, v in m.state_dict().items()}


def _scores(arch, t):
    return t.softmax(-1) if arch['classification_loss_type'] == 'CrossEntropyLoss' else t.sigmoid()


def _gate_fp32(arch, c, r, rc, rr):
    """the gates of test_precise_mode_every_configuration_vs_fp32_oracle"""
    raw = max(float((c - rc).abs().max()), float((r - rr).abs().max()))
    sg = max(float((_scores(arch, c) - _scores(arch, rc)).abs().max()), float((r.sigmoid() - rr.sigmoid()).abs().max()))
    print('raw %.2e sigma %.2e' % (raw, sg))
    assert raw <= 1e-4 and sg <= 1e-3, (raw, sg)


def _gate_fp16(c, r, rc, rr):
    """the gates tests/test_gpu_forward.py applies to RGB against the fp16-storage-emulating oracle"""
    ec, er = (c - rc).abs(), (r - rr).abs()
    print('max %.2e / %.2e  mean %.2e / %.2e' % (ec.max(), er.max(), ec.mean(), er.mean()))
    assert float(ec.max()) < 1e-2 and float(er.max()) < 1e-2
    assert float(ec.mean()) < 1.5e-3 and float(er.mean()) < 1.5e-3


@pytest.mark.parametrize('name,shape', SMALL)
def test_gray_precise_mode_vs_fp32_oracle(name, shape):
    arch = configs.ARCHS[name]
    m, sd = _model(name)
    x = torch.rand(shape[0], 1, shape[1], shape[2], generator=torch.Generator().manual_seed(5)) * 2 - 1
    with torch.no_grad():
        rc, rr, rsizes = net_oracle.lfd_forward(sd, arch, x)
        m.cuda()
        m.precision = 'fp32_storage'
        c, r = m(x.cuda())
    assert [tuple(m.head_indexes_to_feature_map_sizes[i]) for i in range(len(rsizes))] == [tuple(s) for s in rsizes]
    _gate_fp32(arch, c.cpu(), r.cpu(), rc, rr)


@pytest.mark.parametrize('name', ['WIDERFACE_LFD_S', 'TT100K_LFD_L'])
def test_gray_precise_mode_fp32_tensor_plan(name, monkeypatch):
    """LFD_P32_PLANES=0: the fp32-tensor plan (lfd_p32_* with cin = 1) on its own"""
    monkeypatch.setenv('LFD_P32_PLANES', '0')
    arch = configs.ARCHS[name]
    m, sd = _model(name)
    x = torch.rand(1, 1, 90, 161, generator=torch.Generator().manual_seed(6)) * 2 - 1
    with torch.no_grad():
        rc, rr, _ = net_oracle.lfd_forward(sd, arch, x)
        m.cuda()
        m.precision = 'fp32_storage'
        c, r = m(x.cuda())
    assert isinstance(engine_p32.get_plan(m, x.cuda().device), engine_p32.PrecisePlan)
    _gate_fp32(arch, c.cpu(), r.cpu(), rc, rr)


@pytest.mark.parametrize('name,shape', SMALL)
def test_gray_fp16_mode_vs_fp16_emulating_oracle(name, shape):
    arch = configs.ARCHS[name]
    m, sd = _model(name)
    x = (torch.rand(shape[0], 1, shape[1], shape[2], generator=torch.Generator().manual_seed(3)) * 2 - 1).half().float()
    with torch.no_grad():
        rc, rr, _ = net_oracle.lfd_forward_fp16(sd, arch, x)
        m.cuda()
        c, r = m(x.cuda())
    _gate_fp16(c.cpu(), r.cpu(), rc, rr)


@pytest.mark.parametrize('precision', ['fp16', 'fp32_storage'])
def test_gray_widerface_s_8x1080p(precision):
    name = 'WIDERFACE_LFD_S'
    arch = configs.ARCHS[name]
    m, sd = _model(name)
    x = (torch.rand(8, 1080, 1920, 1, generator=torch.Generator().manual_seed(11)) * 2 - 1).half()
    m.cuda()
    m.precision = precision
    with torch.no_grad():
        c, r = m.forward_resident(x.cuda())
        c, r = c[5].cpu(), r[5].cpu()
        xi = x[5:6].float().permute(0, 3, 1, 2).contiguous()
        if precision == 'fp16':
            rc, rr, _ = net_oracle.lfd_forward_fp16(sd, arch, xi)
            _gate_fp16(c, r, rc[0], rr[0])
        else:
            rc, rr, _ = net_oracle.lfd_forward(sd, arch, xi)
            _gate_fp32(arch, c, r, rc[0], rr[0])


@pytest.mark.parametrize('precision', ['fp16', 'fp32_storage'])
def test_gray_input_formats_agree(precision):
    """uint8 frames (simple_normalize on the load) == their normalised fp16 / fp32 frames"""
    m, _ = _model('WIDERFACE_LFD_XS')
    m.cuda()
    m.precision = precision
    img = torch.randint(0, 256, (2, 120, 168, 1), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    xf = (img.float() / 255 - 0.5) / 0.5
    with torch.no_grad():
        a = [t.clone() for t in m.forward_resident(img.cuda())]
        c = [t.clone() for t in m.forward_resident(xf.permute(0, 3, 1, 2).contiguous().cuda())]
        if precision == 'fp16':
            b = [t.clone() for t in m.forward_resident(xf.half().cuda())]
            assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
            assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
        else:
            assert max(float((a[i] - c[i]).abs().max()) for i in (0, 1)) <= 1e-5


@pytest.mark.parametrize('precision', ['fp16', 'fp32_storage'])
def test_gray_rgb_frames_are_refused(precision):
    m, _ = _model('WIDERFACE_LFD_XS')
    m.cuda()
    m.precision = precision
    with pytest.raises(RuntimeError, match=r'\[N,1,H,W\]'):
        m(torch.zeros(1, 3, 64, 64, device='cuda'))
    rgb = configs.build_model('WIDERFACE_LFD_XS').eval().cuda()
    rgb.precision = precision
    with pytest.raises(RuntimeError, match=r'\[N,3,H,W\]'):
        rgb(torch.zeros(1, 1, 64, 64, device='cuda'))


@pytest.mark.parametrize('precision', ['fp16', 'fp32_storage'])
def test_gray_deterministic_and_graphed_detect_matches_eager(precision):
    m, _ = _model('WIDERFACE_LFD_S')
    m.cuda()
    m.precision = precision
    x = (torch.rand(2, 270, 480, 1, generator=torch.Generator().manual_seed(4)) * 2 - 1).half().cuda()
    meta = torch.tensor([[480.0, 270.0, 1.0]] * 2).cuda()
    with torch.no_grad():
        a = [t.clone() for t in m.forward_resident(x)]
        b = [t.clone() for t in m.forward_resident(x)]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        thr = float(torch.quantile(a[0].float().sigmoid().reshape(-1), 0.99))
        m.use_graph = False
        e = m.detect_resident(x, meta, score_thr=thr)
        torch.cuda.synchronize()
        ref = [t.clone() for t in (e.counts, e.dets, e.labels)]
        m.use_graph = True
        for _ in range(3):
            o = m.detect_resident(x, meta, score_thr=thr)
        torch.cuda.synchronize()
        c = [t.clone() for t in m.forward_resident(x)]
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    assert torch.equal(o.counts, ref[0])
    for n in range(2):
        k = int(ref[0][n, 1])
        assert k > 0 and torch.equal(o.dets[n, :k], ref[1][n, :k]) and torch.equal(o.labels[n, :k], ref[2][n, :k])
    # get_results on the same logits (host path of the reference's API)
    res = m.get_results((a[0], a[1]), [dict(resized_height=270, resized_width=480, resize_scale=1.0)] * 2)
    assert len(res) == 2


@pytest.mark.parametrize('precision', ['fp16', 'fp32_storage'])
def test_gray_predict_for_single_image(precision):
    m, _ = _model('WIDERFACE_LFD_XS')
    m.precision = precision
    img = np.random.default_rng(0).integers(0, 256, (150, 211, 1)).astype(np.uint8)

    def simple_normalize(sample):                       # augmentation_pipeline.py:31-36
        sample['image'] = ((sample['image'].astype(np.float32) / 255 - 0.5) / 0.5)
        return sample

    with torch.no_grad():
        c, r = m.cuda()(torch.from_numpy(simple_normalize({'image': img})['image'].transpose(2, 0, 1)[None].copy()).cuda())
    m._classification_threshold = float(torch.quantile(c.sigmoid().reshape(-1), 0.98))
    res = m.predict_for_single_image(img, simple_normalize)
    assert isinstance(res, list) and len(res) > 0
    assert all(len(d) == 6 for d in res)


def test_gray_sibling_runs_in_fp16_mode():
    """an FCOS sibling on a gray LFDResNet: the backbone's gray stem through engine.get_plan, the rest layer by layer"""
    from lfd_amd.model.backbone import LFDResNet
    m = configs.build_sibling_model('FCOS_FPN', input_channels=1).eval()
    assert isinstance(m._backbone, LFDResNet) and m._backbone._input_channels == 1
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    bbk = configs.SIBLINGS['FCOS_FPN']['backbone']
    x = (torch.rand(1, 1, 96, 128, generator=torch.Generator().manual_seed(2)) * 2 - 1).half().float()
    with torch.no_grad():
        ref_taps = net_oracle.backbone_forward(sd, bbk, x)
        m.cuda()
        outs = m(x.cuda())
        taps = m._backbone(x.cuda())
    assert len(outs) == 3 and all(bool(torch.isfinite(t).all()) for t in outs)
    assert len(taps) == len(ref_taps)
    for t, r in zip(taps, ref_taps):
        assert t.shape == r.shape
        assert float((t.cpu() - r).abs().max()) <= 2e-2 * max(1.0, float(r.abs().max()))


def test_gray_image_parallel_map():
    """lfd_amd.parallel.sharded_map over gray frames (one rank here): the per-image detections of the batched step"""
    m, _ = _model('WIDERFACE_LFD_XS')
    m.cuda()
    frames = (torch.rand(5, 96, 128, 1, generator=torch.Generator().manual_seed(8)) * 2 - 1).half().cuda()
    meta = torch.tensor([[128.0, 96.0, 1.0]] * 5).cuda()
    with torch.no_grad():
        c, _ = m.forward_resident(frames)
        thr = float(torch.quantile(c.float().sigmoid().reshape(-1), 0.98))
        full = m.detect_resident(frames, meta, score_thr=thr)
        torch.cuda.synchronize()
        want = [full.dets[i, :int(full.counts[i, 1])].cpu() for i in range(5)]

        def fn(lo, hi):
            outs = []
            for i in range(lo, hi):
                o = m.detect_resident(frames[i:i + 1].contiguous(), meta[i:i + 1], score_thr=thr, slot=1)
                torch.cuda.synchronize()
                outs.append(o.dets[0, :int(o.counts[0, 1])].cpu())
            return outs
        got = parallel.sharded_map(5, fn)
    assert len(got) == 5
    for a, b in zip(got, want):
        assert a.shape == b.shape and float((a - b).abs().max() if a.numel() else 0) < 1e-3
