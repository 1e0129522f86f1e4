"""GPU tests of the training pass of the FPN / SimpleFPN necks on the HIP path: the four kernels of csrc/sibling_train.hip per
element against float64 PyTorch on the CPU (same fp16 inputs), the backbone + neck autograd node (train_engine.PyramidTrainFunction)
against the package's own route with the neck under autograd (LFD_HIP_NECK=0), and whole training iterations of the two pyramid
siblings.

Bounds of the kernel tests: a result is ONE fp16 rounding of an fp32 accumulation of K addends,
    |got - ref| <= 2^-11 |ref| + K 2^-24 sum|addends|
(K additions, each within 2^-24 relative of a partial sum that sum|addends| bounds), evaluated per element."""
import copy
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sibling_cases as SC
from lfd_amd import _lib, configs, ops, train_engine as te
from lfd_amd.model import backbone as B, neck as N

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U16, U32 = 2.0 ** -11, 2.0 ** -24


def _nchw64(t):
    return t.double().permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


def _assert_within(got, ref, bound, what):
    err = (got.double() - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print('%s: max error / bound %.3g (max error %.3g)' % (what, worst, float(err.max())))
    assert bool((err <= bound).all()), (what, worst)


# ----------------------------------------------------------------------------------------------- (a) upsample-add backward
@pytest.mark.parametrize('shape', [((12, 16), (6, 8)), ((13, 17), (7, 9)), ((7, 9), (4, 5)), ((5, 5), (1, 1)), ((6, 8), (6, 8))])
def test_upsample_nearest_add_backward_vs_float64_autograd(shape):
    (H, W), (h, w) = shape
    g = torch.Generator().manual_seed(13)
    g_dst = torch.randn(2, H, W, 64, generator=g).half()
    g_src = torch.randn(2, h, w, 64, generator=g).half()

    def adjoint(t):          # the float64 adjoint of F.interpolate(mode='nearest') applied to t [2,H,W,64]
        x = torch.zeros(2, 64, h, w, dtype=torch.float64, requires_grad=True)
        F.interpolate(x, size=(H, W), mode='nearest').backward(_nchw64(t))
        return _nhwc(x.grad)

    ref = g_src.double() + adjoint(g_dst)
    mag = g_src.double().abs() + adjoint(g_dst.abs())
    K = adjoint(torch.ones_like(g_dst))                      # additions per element
    assert float(K.max()) <= 25 and float(K.sum()) == 2 * 64 * H * W
    got = ops.upsample_nearest_add_backward_(g_src.to(DEV).contiguous(), g_dst.to(DEV).contiguous()).cpu()
    _assert_within(got, ref, U16 * ref.abs() + K * U32 * mag, 'upsample-add backward %s' % (shape,))


# ----------------------------------------------------------------------------------------------- (b) maxpool backward
@pytest.mark.parametrize('shape', [(2, 9, 11, 128), (2, 8, 10, 64)])
@pytest.mark.parametrize('accumulate', [0, 1])
def test_maxpool_backward_vs_float64_autograd_with_ties(shape, accumulate):
    n, h, w, c = shape
    g = torch.Generator().manual_seed(17)
    x = torch.randn(shape, generator=g).clamp_(min=0).half()           # after a ReLU: about half of the values tie at 0
    x[:, 2:7, 3:8, :] = 1.5                                            # and a constant patch: whole windows tie
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    g_out = torch.randn(n, oh, ow, c, generator=g).half()
    g_in = torch.randn(shape, generator=g).half()
    win = F.unfold(F.pad(x.float().permute(0, 3, 1, 2), (1, 1, 1, 1), value=float('-inf')).reshape(n * c, 1, h + 2, w + 2), 3, stride=2)
    assert int(((win == win.max(1, keepdim=True).values).sum(1) > 1).sum()) > 0          # a maximum attained more than once

    def adjoint(t):
        xx = _nchw64(x).clone().requires_grad_(True)
        F.max_pool2d(xx, 3, 2, 1).backward(_nchw64(t))
        return _nhwc(xx.grad)

    ref, mag = adjoint(g_out), adjoint(g_out.abs())
    if accumulate:
        ref, mag = ref + g_in.double(), mag + g_in.double().abs()
    got = ops.maxpool3x3s2_backward(x.to(DEV), g_out.to(DEV), g_in.to(DEV).clone() if accumulate else None).cpu()
    _assert_within(got, ref, U16 * ref.abs() + 4 * U32 * mag, 'maxpool backward %s accumulate=%d' % (shape, accumulate))
    # the tie rule itself on an all-zero input: the gradient lands on the first valid element of each window
    z = torch.zeros(1, 4, 4, 8, dtype=torch.float16)
    go = torch.ones(1, 2, 2, 8, dtype=torch.float16)
    gz = ops.maxpool3x3s2_backward(z.to(DEV), go.to(DEV)).cpu()
    want = torch.zeros(1, 4, 4, 8)
    want[0, 0, 0], want[0, 0, 1], want[0, 1, 0], want[0, 1, 1] = 1, 1, 1, 1
    assert torch.equal(gz.float(), want)


# ----------------------------------------------------------------------------------------------- (c) ReLU backward + add
def test_relu_backward_add_is_the_fp32_expression_rounded_once():
    g = torch.Generator().manual_seed(19)
    y = torch.randn(2, 9, 11, 64, generator=g).half()
    y[0, :3] = 0
    ga, gb = torch.randn(2, 9, 11, 64, generator=g).half(), torch.randn(2, 9, 11, 64, generator=g).half() * 3
    zero = torch.zeros((), dtype=torch.float16)
    both = torch.where(y > 0, (ga.float() + gb.float()).half(), zero)
    one = torch.where(y > 0, ga, zero)
    yd, gad, gbd = y.to(DEV), ga.to(DEV), gb.to(DEV)
    assert torch.equal(ops.relu_backward_add(yd, gad, gbd).cpu(), both)
    assert torch.equal(ops.relu_backward_add(yd, gad).cpu(), one)
    buf = gad.clone()
    assert ops.relu_backward_add(yd, buf, gbd, out=buf) is buf and torch.equal(buf.cpu(), both)      # in place over g_a


# ----------------------------------------------------------------------------------------------- (d) bias gradient
@pytest.mark.parametrize('c', [64, 128])
@pytest.mark.parametrize('rows', [1, 63, 442, 5000, 9000])      # 9000 x 128: more vectors than the grid of partial rows
@pytest.mark.parametrize('inv', [1.0, 1.0 / 1024])
def test_bias_gradient_vs_float64_column_sum(rows, c, inv):
    """bound rows 2^-24 sum|dy_c| (times the power-of-two inv_scale).  That bound has no term for the rounding of the fp32
    accumulator itself, so the inputs keep the `+=` exact where it matters (rows = 1): |dy| >= 2^-6 and the gradient already
    in dbias on a 2^-3 grid (times inv_scale) -- fewer than 24 bits between its top bit and the lowest bit of any dy."""
    g = torch.Generator().manual_seed(23 + rows + c)
    dy = torch.randn(rows, c, generator=g).half()
    dy = torch.where(dy.abs() < 2.0 ** -6, torch.full_like(dy, 2.0 ** -6), dy)
    dbias0 = (torch.randint(1, 9, (c,), generator=g).float() * (torch.randint(0, 2, (c,), generator=g).float() * 2 - 1) / 8) * inv
    assert bool((dbias0 != 0).all())
    ref = dbias0.double() + inv * dy.double().sum(0)
    bound = rows * U32 * dy.double().abs().sum(0) * inv
    got = ops.bias_grad_(dy.to(DEV), inv, dbias0.to(DEV).clone()).cpu()
    _assert_within(got, ref, bound, 'bias gradient rows=%d c=%d inv=%g' % (rows, c, inv))
    dy4 = dy[:rows - rows % 3].reshape(-1, 3, c) if rows >= 3 else None           # leading axes are just rows
    if dy4 is not None:
        a = ops.bias_grad_(dy4.to(DEV).contiguous(), inv, torch.zeros(c, device=DEV))
        b = ops.bias_grad_(dy4.reshape(-1, c).to(DEV).contiguous(), inv, torch.zeros(c, device=DEV))
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------------------------- (e) node vs autograd
def _backbone():
    k = configs.SIBLING_BACKBONE
    return B.LFDResNet(block_mode=k['block_mode'], stem_mode=k['stem_mode'], body_mode=None, input_channels=3,
                       stem_channels=k['stem_channels'], body_architecture=list(k['body_architecture']),
                       body_channels=list(k['body_channels']), out_indices=k['out_indices'], frozen_stages=-1,
                       activation_cfg=dict(type='ReLU', inplace=True), norm_cfg=dict(type='BatchNorm2d'),
                       init_with_weight_file=None, norm_eval=False)


class _BackboneNeck(torch.nn.Module):
    def __init__(self, kind, kw):
        super().__init__()
        self.bb = _backbone()
        self.neck = getattr(N, kind)(num_input_channels_list=list(self.bb.num_output_channels_list),
                                     num_input_strides_list=list(self.bb.num_output_strides_list), **kw)


def _neck_out_of_place(neck, inputs):
    """_PyramidNeck.forward with its in-place ops written out of place but with their in-place MEANING: the merge as
    `lat = lat + upsample(..)` (the literal `+=` rewrites a ReLU lateral that ReluBackward saved), the ReLU in front of an extra
    level as F.relu whose result replaces its source for every later consumer (the previous output level goes to the head
    ReLU'd; the literal form rewrites a tap the lateral conv saved).  The reference of the configurations whose literal form
    autograd refuses."""
    lat = [getattr(neck, 'lateral%d' % i)(x) for i, x in enumerate(inputs)]
    order = range(neck._num_inputs - 1) if neck._bottom_up else range(neck._num_inputs - 1, 0, -1)
    for i in order:
        dst, src = (i, i + 1) if neck._bottom_up else (i - 1, i)
        lat[dst] = lat[dst] + F.interpolate(lat[src], size=lat[dst].shape[2:], mode='nearest')
    outs = []
    for i in range(neck._num_outputs):
        mods = list(getattr(neck, 'fpn_out%d' % i))
        if i < neck._num_inputs:
            src = lat[i]
        elif i == neck._num_inputs and neck._extra_on_input:
            src = inputs[-1]
            if isinstance(mods[0], torch.nn.ReLU):
                src, mods = F.relu(src), mods[1:]
        else:
            src = outs[-1]
            if isinstance(mods[0], torch.nn.ReLU):
                src, mods = F.relu(src), mods[1:]
                outs[-1] = src
        for m in mods:
            src = m(src)
        outs.append(src)
    return tuple(outs)


def _autograd_route(m, x, seeds):
    """backbone node + neck under autograd: what LFD_HIP_NECK=0 runs.  -> outputs (gradients land in .grad)"""
    try:
        outs = m.neck(list(te.backbone_train_forward(m.bb, x)))
        sum((o * s).sum() for o, s in zip(outs, seeds)).backward()
        return outs, 'modules'
    except RuntimeError as e:
        if 'inplace' not in str(e) and 'in-place' not in str(e):
            raise
    return None, 'refused'


_GATES = dict(out_max=2e-2, out_mean=2e-3, cos=0.9, ratio=(0.8, 1.25), norm=0.03, whole_cos=0.02)


def _compare_gradients(pa, pb, what):
    """per parameter tensor the gate of test_gpu_train_convs.py::test_whole_network_train_forward_backward (cosine > 0.9, norm
    ratio in (0.8, 1.25)); all gradients as one vector: norm within 3 %, 1 - cosine <= 0.02 (test_gpu_finetune.py)"""
    worst_cos, worst_ratio = 1.0, 1.0
    fa, fb = [], []
    for (k, a), (_, b) in zip(pa, pb):
        assert a.grad is not None and b.grad is not None and a.grad.shape == b.grad.shape, k
        ga, gb = a.grad.double().flatten(), b.grad.double().flatten()
        cos = float(ga @ gb / (ga.norm() * gb.norm() + 1e-300))
        ratio = float(ga.norm() / gb.norm())
        worst_cos = min(worst_cos, cos)
        worst_ratio = max(worst_ratio, ratio, 1 / ratio)
        assert cos > _GATES['cos'] and _GATES['ratio'][0] < ratio < _GATES['ratio'][1], (what, k, cos, ratio)
        fa.append(ga)
        fb.append(gb)
    fa, fb = torch.cat(fa), torch.cat(fb)
    e_norm = abs(float(fa.norm()) - float(fb.norm())) / float(fb.norm())
    e_cos = 1 - float(fa @ fb / (fa.norm() * fb.norm()))
    print('%s: per tensor worst cosine %.6f, worst norm ratio %.4f; whole gradient: norm %.3g, 1 - cosine %.3g'
          % (what, worst_cos, worst_ratio, e_norm, e_cos))
    assert e_norm <= _GATES['norm'] and e_cos <= _GATES['whole_cos'], (what, e_norm, e_cos)


@pytest.mark.parametrize('hw', [(96, 128), (50, 66)], ids=['96x128', 'odd-taps'])
@pytest.mark.parametrize('case', SC.NECK_CASES, ids=[c[0] for c in SC.NECK_CASES])
def test_backbone_neck_node_vs_the_autograd_route(case, hw):
    """one forward + backward with a seeded output gradient, node vs backbone node + neck under autograd, identical state.
    (50, 66): taps of 13x17 / 7x9 / 4x5 -- odd, and not in ratio 2.  Where autograd refuses the neck's literal in-place ops (they
    rewrite a tensor another backward saved: fpn_pool_on_input, fpn_conv_on_input_gn), the reference is the same modules
    with those ops out of place and their in-place meaning (_neck_out_of_place).  Measured worst values over the ten cases:
    outputs 7.6e-4 / 7.9e-4 (max relative to max(1, |ref|) / mean), per tensor cosine 0.999657 and norm ratio 1.0084, whole
    gradient norm 1.3e-4 and 1 - cosine 8.6e-5."""
    name, kind, kw = case
    ma = configs.synthetic_weights(_BackboneNeck(kind, kw), seed=5).to(DEV).train()
    mb, fresh = copy.deepcopy(ma), copy.deepcopy(ma)
    assert te.pyramid_supported(ma.bb, ma.neck)
    x = (torch.rand(2, 3, hw[0], hw[1], generator=torch.Generator().manual_seed(7)) * 2 - 1).to(DEV)
    outs_a = te.backbone_neck_train_forward(ma.bb, ma.neck, x)
    if hw == (50, 66):
        assert [tuple(o.shape[2:]) for o in outs_a[:3]][:len(outs_a)] == [(13, 17), (7, 9), (4, 5)][:len(outs_a)]
    g = torch.Generator().manual_seed(9)
    seeds = [(torch.randn(o.shape, generator=g) / o.numel() ** 0.5).to(DEV) for o in outs_a]
    sum((o * s).sum() for o, s in zip(outs_a, seeds)).backward()
    outs_b, how = _autograd_route(mb, x, seeds)
    if outs_b is None:
        mb = fresh          # (the refused pass left half a backward in the first copy's .grad)
        outs_b = _neck_out_of_place(mb.neck, list(te.backbone_train_forward(mb.bb, x)))
        sum((o * s).sum() for o, s in zip(outs_b, seeds)).backward()
    assert len(outs_a) == len(outs_b) == kw['num_outputs']
    e_max = e_mean = 0.0
    for i, (a, b) in enumerate(zip(outs_a, outs_b)):
        assert a.shape == b.shape and a.dtype == torch.float32
        err = (a.detach() - b.detach()).abs()
        e_max = max(e_max, float(err.max()) / max(1.0, float(b.detach().abs().max())))
        e_mean = max(e_mean, float(err.mean()))
        assert float(err.max()) <= _GATES['out_max'] * max(1.0, float(b.detach().abs().max())), (i, float(err.max()))
        assert float(err.mean()) <= _GATES['out_mean'], (i, float(err.mean()))
    print('%s %s (reference: %s): outputs max %.3g (relative to max(1, |ref|)), mean %.3g' % (name, hw, how, e_max, e_mean))
    _compare_gradients(list(ma.named_parameters()), list(mb.named_parameters()), '%s %s' % (name, hw))
    for (k, a), (_, b) in zip(ma.named_buffers(), mb.named_buffers()):
        if k.endswith('num_batches_tracked'):
            assert int(a) == int(b) == 1, k
        elif k.startswith('neck.'):           # the lateral BatchNorms' running statistics move as under autograd
            assert float((a - b).abs().max()) <= 2e-3 * max(1.0, float(b.abs().max())), k


# ----------------------------------------------------------------------------------------------- (f) (g) (h) whole iterations
def _batch(name):
    spec = configs.SIBLINGS[name]
    x = (torch.rand(2, 3, 128, 160, generator=torch.Generator().manual_seed(7)) * 2 - 1).to(DEV)
    return x, SC.synth_annotations(5, 2, 128, 160, spec['head']['num_classes'])


def test_lfdv2_sfpn_trains():
    """ReLU laterals + the in-place ReLU in front of the pooled extra level: an autograd error on the module route (the extra
    level rewrites a tensor ReluBackward saved), a plain schedule in the node.  Three SGD steps lower the loss on one batch."""
    name = 'LFDV2_SFPN'
    model = configs.build_sibling_model(name, seed=1).to(DEV).train()
    assert te.pyramid_supported(model._backbone, model._neck)
    x, ann = _batch(name)
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        lo = model.get_loss(model(x), ann)
        lo['loss'].backward()
        opt.step()
        losses.append(lo['loss_values']['loss'])
    print('LFDV2_SFPN losses', losses)
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())


def _iteration(model, x, ann):
    model.zero_grad()
    lo = model.get_loss(model(x), ann)
    lo['loss'].backward()
    return float(lo['loss_values']['loss'])


def test_fcos_fpn_iteration_node_vs_autograd_neck(monkeypatch):
    """get_loss + backward with LFD_HIP_NECK on and off from identical state: loss 1 %, gradient norm 3 %, 1 - cosine <= 0.02"""
    name = 'FCOS_FPN'
    ma = configs.build_sibling_model(name, seed=1).to(DEV).train()
    mb = copy.deepcopy(ma)
    x, ann = _batch(name)
    monkeypatch.setenv('LFD_HIP_NECK', '1')
    la = _iteration(ma, x, ann)
    assert '_lfd_pyramid_plan' in ma._neck.__dict__
    monkeypatch.setenv('LFD_HIP_NECK', '0')
    lb = _iteration(mb, x, ann)
    assert '_lfd_pyramid_plan' not in mb._neck.__dict__
    print('FCOS_FPN loss node %.6g autograd neck %.6g (relative %.3g)' % (la, lb, abs(la - lb) / abs(lb)))
    assert abs(la - lb) <= 0.01 * abs(lb)
    fa = torch.cat([p.grad.double().flatten() for p in ma.parameters()])
    fb = torch.cat([p.grad.double().flatten() for p in mb.parameters()])
    e_norm = abs(float(fa.norm()) - float(fb.norm())) / float(fb.norm())
    e_cos = 1 - float(fa @ fb / (fa.norm() * fb.norm()))
    print('FCOS_FPN whole gradient: norm %.3g, 1 - cosine %.3g' % (e_norm, e_cos))
    assert e_norm <= 0.03 and e_cos <= 0.02


@pytest.mark.parametrize('name', ['FCOS_FPN', 'LFDV2_SFPN'])
def test_iteration_twice_from_identical_state_gives_equal_bits(name, monkeypatch):
    """no atomics in the node: backbone and neck gradients of two runs are the same bits (the head runs under autograd on
    PyTorch-ROCm's convs, asked for their deterministic algorithms)"""
    monkeypatch.setattr(torch.backends.cudnn, 'deterministic', True)
    monkeypatch.setattr(torch.backends.cudnn, 'benchmark', False)
    ma = configs.build_sibling_model(name, seed=1).to(DEV).train()
    mb = copy.deepcopy(ma)
    x, ann = _batch(name)
    la, lb = _iteration(ma, x, ann), _iteration(mb, x, ann)
    assert la == lb
    for (k, a), (_, b) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(a.grad, b.grad), k
    for (k, a), (_, b) in zip(ma.named_buffers(), mb.named_buffers()):
        assert torch.equal(a, b), k


# ----------------------------------------------------------------------------------------------- (i) argument validation
def test_argument_validation_returns_status_codes():
    l = _lib.lib()
    t = torch.zeros(1, 4, 4, 64, dtype=torch.float16, device=DEV)
    s = torch.zeros(1, 2, 2, 64, dtype=torch.float16, device=DEV)
    f = torch.zeros(64, device=DEV)
    ws = torch.empty(l.lfd_bias_grad_workspace_bytes(), dtype=torch.uint8, device=DEV)
    p = ops.ptr
    INVALID, SMALL, UNSUPPORTED = -1, -2, -4
    assert l.lfd_upsample_nearest_add_bwd_nhwc_f16(None, p(t), 1, 4, 4, 2, 2, 64, None) == INVALID
    assert l.lfd_upsample_nearest_add_bwd_nhwc_f16(p(s), None, 1, 4, 4, 2, 2, 64, None) == INVALID
    assert l.lfd_upsample_nearest_add_bwd_nhwc_f16(p(t), p(t), 1, 4, 4, 4, 4, 64, None) == INVALID        # aliased
    assert l.lfd_upsample_nearest_add_bwd_nhwc_f16(p(s), p(t), 0, 4, 4, 2, 2, 64, None) == INVALID
    assert l.lfd_upsample_nearest_add_bwd_nhwc_f16(p(s), p(t), 1, 4, 4, 0, 2, 64, None) == INVALID
    assert l.lfd_upsample_nearest_add_bwd_nhwc_f16(p(s), p(t), 1, 4, 4, 2, 2, 12, None) == UNSUPPORTED
    assert l.lfd_upsample_nearest_add_bwd_nhwc_f16(C.c_void_p(s.data_ptr() + 2), p(t), 1, 4, 4, 2, 2, 64, None) == INVALID
    assert l.lfd_maxpool3x3s2_bwd_nhwc_f16(None, p(s), p(t), 1, 4, 4, 64, 0, None) == INVALID
    assert l.lfd_maxpool3x3s2_bwd_nhwc_f16(p(t), p(s), p(t), 1, 4, 4, 64, 0, None) == INVALID              # g_in over x
    assert l.lfd_maxpool3x3s2_bwd_nhwc_f16(p(t), p(s), None, 1, 4, 4, 64, 1, None) == INVALID
    assert l.lfd_maxpool3x3s2_bwd_nhwc_f16(p(t), p(s), p(t.clone()), 1, 4, 0, 64, 0, None) == INVALID
    assert l.lfd_maxpool3x3s2_bwd_nhwc_f16(p(t), p(s), p(t.clone()), 1, 4, 4, 20, 0, None) == UNSUPPORTED
    assert l.lfd_relu_bwd_add_f16(None, p(t), None, p(t), 64, None) == INVALID
    assert l.lfd_relu_bwd_add_f16(p(t), p(t), None, None, 64, None) == INVALID
    assert l.lfd_relu_bwd_add_f16(p(t), p(t), None, p(t), -8, None) == INVALID
    assert l.lfd_relu_bwd_add_f16(p(t), p(t), None, p(t), 63, None) == UNSUPPORTED
    assert l.lfd_relu_bwd_add_f16(p(t), p(t), None, p(t), 0, None) == 0
    assert l.lfd_bias_grad_nhwc_f16(None, 16, 64, 1.0, p(f), p(ws), ws.numel(), None) == INVALID
    assert l.lfd_bias_grad_nhwc_f16(p(t), 16, 64, 1.0, None, p(ws), ws.numel(), None) == INVALID
    assert l.lfd_bias_grad_nhwc_f16(p(t), 0, 64, 1.0, p(f), p(ws), ws.numel(), None) == INVALID
    assert l.lfd_bias_grad_nhwc_f16(p(t), 16, 64, 1.0, p(f), None, ws.numel(), None) == INVALID
    assert l.lfd_bias_grad_nhwc_f16(p(t), 16, 96, 1.0, p(f), p(ws), ws.numel(), None) == UNSUPPORTED
    assert l.lfd_bias_grad_nhwc_f16(p(t), 16, 64, 1.0, p(f), p(ws), ws.numel() - 1, None) == SMALL
    torch.cuda.synchronize()
    assert not bool(t.any()) and not bool(s.any()) and not bool(f.any())        # nothing was launched
    with pytest.raises(RuntimeError):
        ops.upsample_nearest_add_backward_(s, torch.zeros(2, 4, 4, 64, dtype=torch.float16, device=DEV))
    with pytest.raises(RuntimeError):
        ops.maxpool3x3s2_backward(t, torch.zeros(1, 3, 3, 64, dtype=torch.float16, device=DEV))
    with pytest.raises(RuntimeError):
        ops.bias_grad_(t.cpu(), 1.0, f)
