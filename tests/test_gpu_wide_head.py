"""The 128-row instantiation of csrc/head_out.hip -- the glue around output convs padded to 128 rows -- and what it opens: heads with up to 124 (merged)
/ 128 (separate towers) class channels on the all-HIP training path, eager and as one graph.

Kernel tests: against a plain torch restatement (split = float(y) * scale, dy = half(grad * scale * loss_scale), dbias / dscale
fp64 sums), n = 2 and hw in {1, 33, 600}: 33 pixels x 16 pieces is not a multiple of the 256-thread block, 600 pixels give more
than one block of partials (75).  out and dy are single roundings of fp32 products: compared with ==.  dbias / dscale accumulate
onto non-zero values; their tolerance (rtol 1e-6, atol 1e-7 against the fp64 sums) is the one of the 64-row test
tests/test_gpu_train_convs.py::test_head_output_glue_kernels_vs_torch_ops, with the same magnitudes (y ~ 2 N(0,1), gradients
~ 1e-3 N(0,1), initial values 0.5 / 0.25).  Guard bytes around out, dy, dbias and the workspace follow
tests/test_gpu_resident_loader.py (_guarded: 256 bytes of 0xA5 on both sides)."""
import copy
import json
import os

import numpy as np
import pytest
import torch

from lfd_amd import _lib, configs, data, ops, optim, train, train_engine

pytestmark = pytest.mark.gpu

GUARD = 256
S = 1024.0
WS_BYTES = 1 << 20         # 1024 blocks x 2 x 128 floats

# (name, [(channels, row0, Scale?)])
LAYOUTS = [('coco_80+4', [(80, 0, False), (4, 80, True)]),
           ('124+4', [(124, 0, False), (4, 124, True)]),
           ('61+4', [(61, 0, False), (4, 61, True)]),
           ('single_128', [(128, 0, False)]),
           ('single_4', [(4, 0, False)])]


def _guarded(shape, dtype, fill=None):
    """-> (tensor view, whole uint8 buffer): the view sits between two runs of GUARD bytes of 0xA5"""
    nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
    pad = -nbytes % 16
    whole = torch.full((nbytes + pad + 2 * GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
    t = whole[GUARD:GUARD + nbytes].view(dtype).view(shape)
    if fill is not None:
        t.fill_(fill)
    return t, whole, nbytes


def _guards_intact(whole, nbytes):
    return bool((whole[:GUARD] == 0xA5).all()) and bool((whole[GUARD + nbytes:] == 0xA5).all())


def _seg_array(segs, field):
    arr = (_lib.HeadOutSeg * len(segs))()
    for i, sg in enumerate(segs):
        arr[i].channels, arr[i].row0 = sg['channels'], sg['row0']
        arr[i].scale = ops.ptr(sg['scale'])
        setattr(arr[i], field, ops.ptr(sg[field]))
        if field == 'grad':
            arr[i].dbias, arr[i].dscale = ops.ptr(sg['dbias']), ops.ptr(sg['dscale'])
    return arr


@pytest.mark.parametrize('hw', [1, 33, 600])
@pytest.mark.parametrize('layout', LAYOUTS, ids=[l[0] for l in LAYOUTS])
def test_wide_glue_kernels_vs_torch_restatement(layout, hw):
    n, P, p0 = 2, hw + 11, 7
    g = torch.Generator(device='cuda').manual_seed(100 + hw)
    y, y_whole, y_bytes = _guarded((n, hw, 128), torch.float16)
    y.copy_((torch.randn((n, hw, 128), generator=g, device='cuda') * 2).half())
    segs, keep = [], []
    for ch, r0, sc in layout[1]:
        out, ow, ob = _guarded((n, P, ch), torch.float32, -7.0)
        dbias, bw, bb = _guarded((ch,), torch.float32, 0.5)
        keep += [(ow, ob), (bw, bb)]
        segs.append(dict(channels=ch, row0=r0, scale=torch.tensor(1.37, device='cuda') if sc else None, out=out, dbias=dbias,
                         dscale=torch.full((), 0.25, device='cuda') if sc else None,
                         grad=torch.randn((n, P, ch), generator=g, device='cuda') * 1e-3))
    l = _lib.lib()
    st = ops.stream_ptr()
    # ---- forward
    assert l.lfd_head_out_split_w_f16(ops.ptr(y), n, hw, P, p0, _seg_array(segs, 'out'), len(segs), 128, st) == 0
    torch.cuda.synchronize()
    for sg in segs:
        ref = y[..., sg['row0']:sg['row0'] + sg['channels']].float()
        if sg['scale'] is not None:
            ref = ref * sg['scale']
        assert torch.equal(sg['out'][:, p0:p0 + hw], ref)
        assert bool((sg['out'][:, :p0] == -7).all()) and bool((sg['out'][:, p0 + hw:] == -7).all())      # nothing outside the level
    # ---- backward: an undersized workspace is refused and nothing is written
    dy, dy_whole, dy_bytes = _guarded((n, hw, 128), torch.float16, 3.0)
    ws, ws_whole, _ = _guarded((WS_BYTES,), torch.uint8, 0x5C)
    arr = _seg_array(segs, 'grad')
    assert l.lfd_head_out_grad_w_f16(ops.ptr(y), n, hw, P, p0, arr, len(segs), 128, S, ops.ptr(dy), ops.ptr(ws), WS_BYTES - 4, st) \
        == -2                                                                                     # LFD_ERR_WORKSPACE_TOO_SMALL
    torch.cuda.synchronize()
    assert bool((dy == 3.0).all()) and bool((ws == 0x5C).all())
    assert all(bool((sg['dbias'] == 0.5).all()) for sg in segs)
    assert l.lfd_head_out_grad_w_f16(ops.ptr(y), n, hw, P, p0, arr, len(segs), 128, S, ops.ptr(dy), ops.ptr(ws), WS_BYTES, st) == 0
    torch.cuda.synchronize()
    ref_dy = torch.zeros((n, hw, 128), dtype=torch.float16, device='cuda')
    covered = torch.zeros(128, dtype=torch.bool, device='cuda')
    for sg in segs:
        rows = slice(sg['row0'], sg['row0'] + sg['channels'])
        covered[rows] = True
        d = sg['grad'][:, p0:p0 + hw]
        raw = y[..., rows].float()
        if sg['scale'] is not None:
            ref_dscale = 0.25 + (d.double() * raw.double()).sum()
            d = d * sg['scale']
            print(layout[0], hw, 'dscale', float(sg['dscale']), float(ref_dscale))
            torch.testing.assert_close(sg['dscale'].double(), ref_dscale, rtol=1e-6, atol=1e-7)
        ref_dbias = 0.5 + d.double().sum((0, 1))
        print(layout[0], hw, 'dbias max abs err', float((sg['dbias'].double() - ref_dbias).abs().max()))
        torch.testing.assert_close(sg['dbias'].double(), ref_dbias, rtol=1e-6, atol=1e-7)
        ref_dy[..., rows] = (d * S).half()
    assert torch.equal(dy, ref_dy)
    assert not bool(dy[..., ~covered].any())                      # rows outside every segment: exactly zero
    assert _guards_intact(y_whole, y_bytes) and _guards_intact(dy_whole, dy_bytes) and _guards_intact(ws_whole, WS_BYTES)
    assert all(_guards_intact(w, b) for w, b in keep)
    # the ops wrappers pick the 128-row entry points from y's last dimension: same bits, and the gradients accumulate again
    y4 = y.view(n, 1, hw, 128)
    outs2 = [torch.full((n, P, sg['channels']), -7.0, device='cuda') for sg in segs]
    ops.head_out_split(y4, segs, outs2, p0)
    assert all(torch.equal(o, sg['out']) for o, sg in zip(outs2, segs))
    before = [sg['dbias'].clone() for sg in segs]
    dy2 = ops.head_out_grad(y4, segs, [sg['grad'] for sg in segs], p0, S)
    assert torch.equal(dy2.view(n, hw, 128), dy)
    assert all(not torch.equal(b, sg['dbias']) for b, sg in zip(before, segs))


@pytest.mark.parametrize('ncls', [80, 61])
def test_wide_glue_of_all_levels_in_one_launch_is_bit_identical(ncls):
    """lfd_head_out_split_levels_w_f16 / lfd_head_out_grad_levels_w_f16 against the per-level `_concat_w` calls: outputs, dy, the
    shared bias gradients and the per-level Scale gradients bit for bit (the property
    tests/test_gpu_train_convs.py::test_head_output_glue_of_all_levels_in_one_launch_is_bit_identical checks for 64 rows)"""
    n, hws = 2, [35, 12, 1]
    starts = [0, 35, 47]
    P = 48
    g = torch.Generator(device='cuda').manual_seed(7 + ncls)
    y = (torch.randn((n, P, 128), generator=g, device='cuda') * 2).half()
    scales = [torch.tensor(0.7 + 0.2 * l, device='cuda') for l in range(len(hws))]
    grads = [torch.randn((n, P, c), generator=g, device='cuda') * 1e-3 for c in (ncls, 4)]

    def run(batched):
        outs = [torch.full((n, P, c), -7.0, device='cuda') for c in (ncls, 4)]
        dbias = [torch.full((c,), 0.5, device='cuda') for c in (ncls, 4)]
        dscale = [torch.full((), 0.25, device='cuda') for _ in hws]
        dy = torch.full((n, P, 128), 3.0, dtype=torch.float16, device='cuda')
        lv_f, lv_b = [], []
        for l, hw in enumerate(hws):
            segs = [dict(kind='cls', channels=ncls, row0=0, scale=None, dbias=dbias[0], dscale=None),
                    dict(kind='reg', channels=4, row0=ncls, scale=scales[l], dbias=dbias[1], dscale=dscale[l])]
            lv_f.append((hw, starts[l], segs, outs))
            lv_b.append((hw, starts[l], segs, grads))
        if batched:
            ops.head_out_split_levels(y, lv_f)
            ops.head_out_grad_levels(y, lv_b, S, dy)
        else:
            for hw, p0, segs, o in lv_f:
                ops.head_out_split_concat(y, hw, segs, o, p0)
            for hw, p0, segs, gr in lv_b:
                ops.head_out_grad_concat(y, hw, segs, gr, p0, S, dy)
        torch.cuda.synchronize()
        return outs + [dy] + dbias + dscale

    a, b = run(True), run(False)
    assert all(torch.equal(x, z) for x, z in zip(a, b))
    # and the values are the restatement's: every point belongs to one level
    assert torch.equal(a[0], y[..., :ncls].float())
    lvl = torch.zeros(P, dtype=torch.long, device='cuda')
    lvl[35:47], lvl[47:] = 1, 2
    sc = torch.stack(scales)[lvl]
    assert torch.equal(a[1], y[..., ncls:ncls + 4].float() * sc[None, :, None])
    ref_dy = torch.zeros_like(a[2])
    ref_dy[..., :ncls] = (grads[0] * S).half()
    ref_dy[..., ncls:ncls + 4] = (grads[1] * sc[None, :, None] * S).half()
    assert torch.equal(a[2], ref_dy)
    assert float(a[3][0]) != 0.5 and float(a[5]) != 0.25


# ------------------------------------------------------------------------------------------------ whole iterations
def _annotations(rng, n, hw, num_classes, k=5, largest=90):
    ann = []
    for _ in range(n):
        wh = np.exp(rng.uniform(np.log(8), np.log(largest), (k, 2)))
        xy = rng.uniform(0, 1, (k, 2)) * (np.array([hw[1], hw[0]]) - wh).clip(1)
        ann.append((np.concatenate([xy, wh], 1).astype(np.float32), rng.integers(0, num_classes, k).astype(np.int64)))
    return ann


def _device_annotations(ann, max_boxes):
    da = data.DeviceAnnotations(len(ann), max_boxes, 'cuda')
    boxes = np.concatenate([b for b, _ in ann], 0)
    labels = np.concatenate([l for _, l in ann], 0)
    offs = np.cumsum([0] + [len(b) for b, _ in ann]).astype(np.int32)
    da.boxes[:len(boxes)].copy_(torch.from_numpy(boxes))
    da.labels[:len(labels)].copy_(torch.from_numpy(labels))
    da.offsets.copy_(torch.from_numpy(offs))
    return da


def test_coco_sized_head_one_iteration_hip_vs_pytorch_autograd(monkeypatch):
    """build_model('WIDERFACE_LFD_S', num_classes=80), Focal + IoU, one iteration from identical state: the all-HIP route (the
    128-row output conv and its glue inside) against the same module tree through PyTorch-ROCm autograd (LFD_HIP_TRAIN=0) with
    the op-by-op loss.  Batch 8 x 512 x 512 = the case 'WIDERFACE_LFD_S@8x512x512' of
    tests/test_train_golden.py::test_every_hip_iteration_from_the_fp32_routes_state (tests/test_gpu_gray_train.py has its gray
    twin): every BatchNorm sees >= 512 elements per channel, below that the fp16 / fp32 routes drift.  Gates of that test for
    iteration 1 of a large case: loss values 1 %, total gradient norm 3 %, 1 - cosine of the whole gradient <= 0.001; per
    parameter tensor the gate of tests/test_gpu_train_convs.py::test_whole_network_train_forward_backward (cosine > 0.9, norm
    ratio in (0.8, 1.25)); BatchNorm running statistics after the forward 0.1 %, that test's gate for a large case.  The fp32
    route runs without MIOpen, as tests/test_gpu_gray_train.py::_reproducible_fp32_route
    explains.  Then the same model with CrossEntropyLoss + IoULoss (81 + 4 rows): forward and loss only."""
    monkeypatch.setattr(torch.backends.cudnn, 'enabled', False)
    rng = np.random.default_rng(17)
    hw = (512, 512)
    x = torch.rand(8, 3, *hw, generator=torch.Generator().manual_seed(11)).cuda() * 2 - 1
    # box sides logU[8, 300]: every pyramid level (ranges up to 320) gets positives, so every Scale has a gradient to compare
    ann = _annotations(rng, 8, hw, 80, k=8, largest=300)
    assert len({int(v) for _, l in ann for v in l}) > 10          # boxes of several classes
    ma = configs.build_model('WIDERFACE_LFD_S', num_classes=80).cuda().train()
    mb = copy.deepcopy(ma)
    assert train_engine.network_supported(mb)
    monkeypatch.setenv('LFD_HIP_TRAIN', '0')
    monkeypatch.setenv('LFD_FUSED_LOSS', '0')
    la = ma.get_loss(ma(x), ann)
    la['loss'].backward()
    monkeypatch.setenv('LFD_HIP_TRAIN', '1')
    monkeypatch.setenv('LFD_FUSED_LOSS', '1')
    calls = []
    real = ops.lib
    monkeypatch.setattr(ops, 'lib', lambda: _Recorder(real, calls))
    lb = mb.get_loss(mb(x), ann)
    lb['loss'].backward()
    monkeypatch.setattr(ops, 'lib', real)
    assert 'lfd_head_out_split_levels_w_f16' in calls and 'lfd_head_out_grad_levels_w_f16' in calls
    assert not [c for c in calls if c.startswith('lfd_head_out') and '_w_' not in c]
    for k in ('loss', 'classification_loss', 'regression_loss'):
        va, vb = la['loss_values'][k], lb['loss_values'][k]
        print('80-class WF-S', k, 'fp32 route', va, 'HIP', vb)
        assert abs(vb - va) <= 0.01 * abs(va), (k, va, vb)
    st = (0.0, '')
    for (k, a), (_, b) in zip(ma.state_dict().items(), mb.state_dict().items()):
        if k.endswith('running_mean') or k.endswith('running_var'):
            st = max(st, (float((a - b).double().norm() / a.double().norm().clamp_min(1e-3)), k))
    print('80-class WF-S running statistics, worst relative difference %.3g (%s)' % st)
    assert st[0] <= 0.001, st
    ga = torch.cat([p.grad.reshape(-1) for p in ma.parameters()]).double()
    gb = torch.cat([p.grad.reshape(-1) for p in mb.parameters()]).double()
    na, nb = float(ga.norm()), float(gb.norm())
    cos = float(ga @ gb / (ga.norm() * gb.norm()))
    print('80-class WF-S gradient norm fp32 route %.6g HIP %.6g, 1 - cos %.3g' % (na, nb, 1 - cos))
    assert abs(nb - na) <= 0.03 * na
    assert 1 - cos <= 0.001
    worst = (2.0, '')
    for (k, pa), pb in zip(ma.named_parameters(), mb.parameters()):
        assert pb.grad is not None and pb.grad.shape == pa.grad.shape, k
        a, b = pa.grad.double().reshape(-1), pb.grad.double().reshape(-1)
        assert float(a.norm()) > 0 and float(b.norm()) > 0, k
        c, ratio = float(a @ b / (a.norm() * b.norm())), float(b.norm() / a.norm())
        worst = min(worst, (c, k))
        assert c > 0.9 and 0.8 < ratio < 1.25, (k, c, ratio)
    print('80-class WF-S worst per-parameter gradient cosine %.6f (%s)' % worst)
    # CrossEntropyLoss + IoULoss: 81 class channels (background) + 4, forward and loss
    arch = dict(configs.ARCHS['WIDERFACE_LFD_S'], num_classes=80, classification_loss_type='CrossEntropyLoss')
    mc = configs.build_model(arch).cuda().train()
    md = copy.deepcopy(mc)
    assert mc._head.num_cls_channels == 81 and train_engine.network_supported(mc)
    monkeypatch.setenv('LFD_HIP_TRAIN', '0')
    monkeypatch.setenv('LFD_FUSED_LOSS', '0')
    with torch.no_grad():
        pc = mc(x)
        lc = mc.get_loss(pc, ann)['loss_values']
    monkeypatch.setenv('LFD_HIP_TRAIN', '1')
    monkeypatch.setenv('LFD_FUSED_LOSS', '1')
    assert md._fused_loss_supported(x)
    with torch.no_grad():
        pd = md(x)
        ld = md.get_loss(pd, ann)['loss_values']
    assert pd[0].shape == pc[0].shape and pd[0].shape[2] == 81
    for k in ('loss', 'classification_loss', 'regression_loss'):
        print('80-class WF-S CE', k, 'fp32 route', lc[k], 'HIP', ld[k])
        assert abs(ld[k] - lc[k]) <= 0.01 * abs(lc[k]), (k, lc[k], ld[k])


def test_graphed_train_step_on_a_coco_sized_head_equals_eager():
    """GraphedTrainStep constructs for the 80-class model and runs three iterations; iterations 2 and 3 are graph replays and
    equal the eager train_step from the same state bit for bit in loss values, gradient norm, parameters and buffers (the
    property tests/test_gpu_train.py::test_graphed_train_step_equals_the_eager_iterations checks for the shipped configs);
    iteration 3 is fed DeviceAnnotations."""
    rng = np.random.default_rng(3)
    torch.manual_seed(5)
    ma = configs.build_model('WIDERFACE_LFD_S', num_classes=80).cuda().train()
    mb = configs.build_model('WIDERFACE_LFD_S', num_classes=80).cuda().train()
    mb.load_state_dict(ma.state_dict())
    kw = dict(lr=0.02, momentum=0.9, weight_decay=1e-4)
    oa, ob = optim.SGD(ma.parameters(), **kw), optim.SGD(mb.parameters(), **kw)
    clip = dict(max_norm=10, norm_type=2)
    step = train.GraphedTrainStep(mb, ob, clip, max_boxes=64)
    for it in range(3):
        x = torch.from_numpy(rng.normal(0, 1, (4, 3, 160, 192)).astype(np.float32)).cuda()
        ann = _annotations(rng, 4, (160, 192), 80)
        lva, na = train.train_step(ma, oa, x, ann, clip, True)
        lvb, nb = step(x, _device_annotations(ann, 64) if it == 2 else ann, True)
        assert len(step.graphs) == (1 if it >= 1 else 0), it       # the first call runs eagerly, the second captures and replays
        assert lva == lvb, (it, lva, lvb)
        assert float(na) == float(nb), it
        for (k, pa), pb in zip(ma.named_parameters(), mb.parameters()):
            assert torch.equal(pa, pb), (it, k)
        for (k, ba), bb in zip(ma.named_buffers(), mb.buffers()):
            assert torch.equal(ba, bb), (it, k)
    assert lva['classification_loss'] > 0 and lva['regression_loss'] > 0


class _Recorder(object):
    """ops' view of the library with every entry point it fetches appended to `calls`"""

    def __init__(self, real, calls):
        self._real, self._calls = real, calls

    def __getattr__(self, name):
        self._calls.append(name)
        return getattr(self._real(), name)


def test_separate_towers_with_80_classes_run_wide_and_narrow_glue_in_one_iteration(monkeypatch):
    """TT100K_LFD_S's separate towers with an 80-class FocalLoss head: per level a 128-row class conv and a 64-row regression
    conv, so both instantiations of the glue serve one iteration.  Forward and loss from identical state against the module tree through
    PyTorch-ROCm autograd (1 % on the loss values: the iteration-1 gate of
    tests/test_train_golden.py::test_every_hip_iteration_from_the_fp32_routes_state for every case), then one whole train_step:
    nothing network_supported admits may fail at launch."""
    monkeypatch.setattr(torch.backends.cudnn, 'enabled', False)
    rng = np.random.default_rng(23)
    hw = (256, 256)
    arch = dict(configs.ARCHS['TT100K_LFD_S'], num_classes=80, classification_loss_type='FocalLoss')
    ma = configs.build_model(arch).cuda().train()
    mb = copy.deepcopy(ma)
    assert train_engine.network_supported(mb)
    x = torch.rand(4, 3, *hw, generator=torch.Generator().manual_seed(12)).cuda() * 2 - 1
    ann = _annotations(rng, 4, hw, 80, k=6, largest=200)
    monkeypatch.setenv('LFD_HIP_TRAIN', '0')
    monkeypatch.setenv('LFD_FUSED_LOSS', '0')
    with torch.no_grad():
        la = ma.get_loss(ma(x), ann)['loss_values']
    monkeypatch.setenv('LFD_HIP_TRAIN', '1')
    monkeypatch.setenv('LFD_FUSED_LOSS', '1')
    with torch.no_grad():
        lb = mb.get_loss(mb(x), ann)['loss_values']
    for k in ('loss', 'classification_loss', 'regression_loss'):
        print('80-class separate towers', k, 'fp32 route', la[k], 'HIP', lb[k])
        assert abs(lb[k] - la[k]) <= 0.01 * abs(la[k]), (k, la[k], lb[k])
    opt = optim.SGD(mb.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    before = [p.detach().clone() for p in mb.parameters()]
    calls = []
    real = ops.lib
    monkeypatch.setattr(ops, 'lib', lambda: _Recorder(real, calls))
    lv, gn = train.train_step(mb, opt, x, ann, dict(max_norm=10, norm_type=2), True)
    monkeypatch.setattr(ops, 'lib', real)
    assert np.isfinite(lv['loss']) and np.isfinite(float(gn)) and float(gn) > 0
    head = sorted(set(c for c in calls if c.startswith('lfd_head_out')))
    assert head == ['lfd_head_out_grad_levels_f16', 'lfd_head_out_grad_levels_w_f16', 'lfd_head_out_split_levels_f16',
                    'lfd_head_out_split_levels_w_f16'], head
    assert all(not torch.equal(a, b) for a, b in zip(before, mb.parameters()))


def test_one_class_model_runs_the_launches_it_ran_before(monkeypatch):
    """The shipped WIDERFACE_LFD_S (1 class, 5 rows of 64): the library entry points of one steady-state training iteration, in
    order, are those recorded on the commit before the 128-row kernels existed (tests/golden/
    wf_s_train_iteration_entry_points.json: same model, batch shape and iteration) -- same names, same count, same order; the
    head_out ones are the 64-row forms, once per iteration each."""
    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                                       'wf_s_train_iteration_entry_points.json')))['calls']
    rng = np.random.default_rng(4)
    torch.manual_seed(0)
    m = configs.build_model('WIDERFACE_LFD_S').cuda().train()
    opt = optim.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    x = torch.from_numpy(rng.normal(0, 1, (4, 3, 160, 192)).astype(np.float32)).cuda()
    ann = _annotations(rng, 4, (160, 192), 1)
    clip = dict(max_norm=10, norm_type=2)
    train.train_step(m, opt, x, ann, clip, True)          # (first iteration: buffers, packs)
    calls = []
    real = ops.lib
    monkeypatch.setattr(ops, 'lib', lambda: _Recorder(real, calls))
    train.train_step(m, opt, x, ann, clip, True)
    monkeypatch.setattr(ops, 'lib', real)
    head = [c for c in calls if c.startswith('lfd_head_out')]
    print('1-class WF-S iteration: %d entry-point calls through ops (recorded before: %d), head_out: %s' % (len(calls), len(want), head))
    assert head == ['lfd_head_out_split_levels_f16', 'lfd_head_out_grad_levels_f16']
    assert len(want) > 200 and calls == want
