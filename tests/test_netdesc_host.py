"""lfd_amd/netdesc.py describes the module tree it is given: executing its records with plain torch.nn.functional calls gives,
bit for bit, what calling the modules themselves gives (same fp32 ops in the same order; CPU, no GPU), and every conv of the
model is in the description exactly once per level that uses it."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import plan_fingerprint as PF
from lfd_amd import netdesc

BACKBONES = ['WIDERFACE_LFD_S', 'WIDERFACE_LFD_L', 'preset_fastest_fastest_fastest', 'XS_backbone_without_norm']
HEADS = ['WIDERFACE_LFD_S', 'TT100K_LFD_S']          # a merged tower, two towers
COUNTED = BACKBONES + ['TT100K_LFD_S', 'XS_unshared_head', 'XS_batchnorm_towers', 'TL_LFD_L']


def _ramp(*shape):
    """closed-form input (the rule of plan_fingerprint.fill)"""
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, dtype=torch.int64)
    return (((i * 2654435761) % 257 - 128).double() / 256).float().reshape(shape)


def _run(l, x, relu=None):
    """one netdesc.Layer as functional calls on the modules' tensors (eval mode)"""
    x = F.conv2d(x, l.conv.weight, l.conv.bias, stride=l.stride, padding=l.ks // 2)
    if isinstance(l.norm, nn.BatchNorm2d):
        x = F.batch_norm(x, l.norm.running_mean, l.norm.running_var, l.norm.weight, l.norm.bias, False, 0.0, l.norm.eps)
    elif isinstance(l.norm, nn.GroupNorm):
        x = F.group_norm(x, l.norm.num_groups, l.norm.weight, l.norm.bias, l.norm.eps)
    else:
        assert l.norm is None
    return F.relu(x) if (l.relu if relu is None else relu) else x


def _taps_from_description(bb, x):
    net = netdesc.backbone_layers(bb)
    for l in net.stem:
        x = _run(l, x)
    taps = []
    for blk in net.blocks:
        ident = x if blk.downsample is None else _run(blk.downsample, x)
        for l in blk.convs[:-1]:
            x = _run(l, x)
        last = blk.convs[-1]
        x = _run(last, x, relu=False) + ident          # the last conv's `relu` comes after the residual add
        if last.relu:
            x = F.relu(x)
        if blk.tap:
            taps.append(x)
    return taps


def _block_by_modules(blk, x):
    """a residual block through its children: conv, its norm where the block has norms, the activation between the convs;
    then the identity (through the downsample branch where there is one) is added and the activation applied once more"""
    kids = dict(blk.named_children())
    convs = [n for n in kids if n.startswith('_conv')]
    out = x
    for k, name in enumerate(convs):
        out = kids[name](out)
        norm = kids.get(name.replace('_conv', '_norm'))
        if norm is not None:
            out = norm(out)
        if k + 1 < len(convs):
            out = kids['_activation'](out)
    identity = kids['_downsample'](x) if '_downsample' in kids else x
    return kids['_activation'](out + identity)


def _taps_from_modules(bb, x):
    kids = dict(bb.named_children())
    for _, m in kids['_stem'].named_children():
        x = m(x)
    taps = []
    for name in [n for n in kids if n.startswith('stage')]:
        for j, (_, blk) in enumerate(kids[name].named_children()):
            x = _block_by_modules(blk, x)
            if (int(name[5:]), j) in [tuple(t) for t in bb._out_indices]:
                taps.append(x)
    return taps


@pytest.mark.parametrize('config', BACKBONES)
def test_backbone_description_executes_like_the_modules(config):
    bb = PF.model_of(config)._backbone
    x = _ramp(1, 3, 64, 64)
    with torch.no_grad():
        a, b = _taps_from_description(bb, x), _taps_from_modules(bb, x.clone())
    assert len(a) == len(b) == len(bb._out_indices)
    for ta, tb in zip(a, b):
        assert torch.isfinite(ta).all() and float(ta.abs().max()) > 0
        assert ta.shape == tb.shape and torch.equal(ta, tb)


@pytest.mark.parametrize('config', HEADS)
def test_head_description_executes_like_the_paths(config):
    m = PF.model_of(config)
    neck, head = m._neck, m._head
    levels = netdesc.lfd_head_levels(neck, head)
    assert len(levels) == head._num_heads
    assert bool(levels[0].merge) == head._merge_path_flag and bool(levels[0].cls) == (not head._merge_path_flag)
    with torch.no_grad():
        for i, d in enumerate(levels):
            f = _ramp(1, d.neck.conv.in_channels, 6, 5 + i)
            t = _run(d.neck, f)
            want = getattr(neck, 'neck%d' % i)(f.clone())
            assert torch.equal(t, want)
            for l in d.merge:
                t = _run(l, t)
            c, r = t, t
            for l in d.cls:
                c = _run(l, c)
            for l in d.reg:
                r = _run(l, r)
            c = F.conv2d(c, d.cls_out.weight, d.cls_out.bias)
            r = F.conv2d(r, d.reg_out.weight, d.reg_out.bias) * d.scale._scale
            wt = getattr(head, 'head%d_merge_path' % i)(want)
            wc = getattr(head, 'head%d_classification_path' % i)(wt.clone())
            wr = head._scales[i](getattr(head, 'head%d_regression_path' % i)(wt.clone()))
            assert torch.isfinite(c).all() and torch.isfinite(r).all() and float(c.abs().max()) > 0
            assert torch.equal(c, wc) and torch.equal(r, wr)
            assert c.shape[1] == head.num_cls_channels and r.shape[1] == 4


def _conv_ids(mod):
    return [id(x) for x in mod.modules() if isinstance(x, nn.Conv2d)]


@pytest.mark.parametrize('config', COUNTED)
def test_every_conv_is_described_once(config):
    m = PF.model_of(config)
    net = netdesc.backbone_layers(m._backbone)
    bb = [l.conv for l in net.stem]
    for blk in net.blocks:
        bb += [l.conv for l in ([blk.downsample] if blk.downsample is not None else []) + blk.convs]
    assert sorted(map(id, bb)) == sorted(_conv_ids(m._backbone))                 # each backbone conv exactly once
    assert [(b.stage, b.index) for b in net.blocks if b.tap] == [tuple(t) for t in m._backbone._out_indices]
    assert all((l.norm is None) == (m._backbone._norm_cfg is None) for l in net.stem + [l for b in net.blocks for l in b.convs])
    per_level = []
    for d in netdesc.lfd_head_levels(m._neck, m._head):
        convs = [l.conv for l in [d.neck] + d.merge + d.cls + d.reg] + [d.cls_out, d.reg_out]
        assert len(set(map(id, convs))) == len(convs)                             # once per level that uses it
        per_level.append(convs)
    flat = [id(c) for convs in per_level for c in convs]
    assert set(flat) == set(_conv_ids(m._neck) + _conv_ids(m._head))
    if not m._head._share_head_flag:
        assert len(flat) == len(_conv_ids(m._neck)) + len(_conv_ids(m._head))     # Layers + output convs = the nn.Conv2d modules
    else:       # shared towers: the same module objects at every level
        assert all(a is b for a, b in zip(per_level[0][1:], per_level[-1][1:]))


def test_split_sequential_groups_and_refuses():
    conv, bn, gn = nn.Conv2d(4, 8, 3, 2, 1), nn.BatchNorm2d(8), nn.GroupNorm(2, 8)
    act = nn.ReLU()
    steps = netdesc.split_sequential(nn.Sequential(nn.ReLU(), conv, bn, act, nn.MaxPool2d(3, 2, 1), conv, gn, conv))
    assert steps[0] == 'relu' and steps[2] == 'pool' and len(steps) == 5
    assert steps[1] == netdesc.Layer(conv, bn, True, 3, 2, act) and steps[3] == netdesc.Layer(conv, gn, False, 3, 2, None)
    assert steps[4] == netdesc.Layer(conv, None, False, 3, 2, None)
    assert netdesc.split_sequential([steps[1], steps[4]]) == [steps[1], steps[4]]         # grouped Layers pass through
    with pytest.raises(netdesc.UnknownModule, match='module Sigmoid in a neck / head path'):
        netdesc.split_sequential([netdesc.layer(conv, bn, nn.Sigmoid())])
    for bad in (nn.Sequential(nn.Sigmoid()), nn.Sequential(nn.MaxPool2d(2, 2))):
        with pytest.raises(netdesc.UnknownModule):
            netdesc.split_sequential(bad)


def _swapped(config, old, new):
    """a fresh model of `config` whose head towers have every `old` module replaced by new()"""
    m = PF.fill(PF.configurations()[config][0]()).eval()
    n = 0
    for name, path in m._head.named_children():
        if isinstance(path, nn.Sequential):
            for k, mod in enumerate(path):
                if isinstance(mod, old):
                    path[k] = new(mod)
                    n += 1
    assert n
    return m


@pytest.mark.parametrize('config', ['WIDERFACE_LFD_XS', 'XS_two_towers', 'XS_batchnorm_towers', 'sibling_LFDV2_SFPN',
                                    'sibling_LFDV2_SIMPLE', 'sibling_LFDV2_HEADV1'])
@pytest.mark.parametrize('what', ['LeakyReLU', 'InstanceNorm2d'])
def test_layer_by_layer_plans_refuse_towers_they_have_no_kernel_for(config, what):
    """the plans without a PyTorch fallback build nothing for a tower activation other than ReLU or a norm other than
    BatchNorm2d / GroupNorm: each raises its own error type, with the splitter's wording"""
    from lfd_amd import engine, engine_sibling, engine_sibling_p32
    if what == 'LeakyReLU':
        m = _swapped(config, nn.ReLU, lambda old: nn.LeakyReLU(0.1))
    else:
        m = _swapped(config, (nn.BatchNorm2d, nn.GroupNorm), lambda old: nn.InstanceNorm2d(old.weight.numel(), affine=True))
    msg = 'module %s in a neck / head path' % what
    with torch.no_grad():
        with pytest.raises(RuntimeError, match=msg) as e:
            engine_sibling.SiblingPlan(m._backbone, m._neck, m._head, PF.CPU)
        assert not isinstance(e.value, engine.Unsupported) and 'sibling engine' in str(e.value)
        for merge in (True, False):
            with pytest.raises(engine.Unsupported, match=msg):
                engine_sibling_p32.SiblingPrecisePlan(m, PF.CPU, merge=merge)
