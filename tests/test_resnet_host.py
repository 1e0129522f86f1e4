"""The torchvision-style ResNet mirror (lfd_amd/model/backbone/resnet.py) and its host-side plumbing, without a GPU:
state_dict keys / shapes, CPU forward, train() flags and the layer walk against what the REFERENCE classes gave
(tests/golden/resnet_*.npz, made by tests/golden/make_golden_resnet.py); the stem7 weight packer against a plain-loop unpack
of the layout csrc/stem7.hip documents; the refusals of the engines."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from lfd_amd import _lib, configs, engine, engine_resnet, netdesc, train_engine
from lfd_amd.model.backbone import ResNet

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = list(configs.RESNET_SIBLINGS)
VARIANTS = {'r18': dict(depth=18), 'r34': dict(depth=34), 'r50': dict(depth=50), 'r18_deep_stem': dict(depth=18, deep_stem=True)}


def _gold(name):
    return np.load(os.path.join(GOLDEN, 'resnet_%s.npz' % name))


def _key_shapes(sd):
    return [[k, list(v.shape)] for k, v in sd.items()]


def _state_sha(sd):
    h = hashlib.sha256()
    for k in sd:
        h.update(k.encode())
        h.update(sd[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def _model(name):
    m = configs.build_resnet_model(name)
    m.eval()
    return m


@pytest.mark.parametrize('tag', list(VARIANTS))
def test_state_dict_keys_and_shapes_are_the_references(tag):
    want = json.loads(str(_gold('module')['keys_' + tag]))
    assert _key_shapes(ResNet(**VARIANTS[tag]).state_dict()) == want
    assert any(k.startswith('stem.') for k, _ in want) == (tag == 'r18_deep_stem')


@pytest.mark.parametrize('name', CASES)
def test_configuration_has_the_references_keys_and_weights(name):
    gold, m = _gold(name), _model(name)
    assert _key_shapes(m.state_dict()) == json.loads(str(gold['keys']))
    assert _state_sha(m.state_dict()) == str(gold['sha'])
    # synthetic_weights draws per key: the norm2 weights zero_init_residual zeroes are not left at 0
    assert all(bool(b.norm2.weight.abs().min() > 0) for b in m._backbone.modules() if hasattr(b, 'norm2'))


@pytest.mark.parametrize('name,suffix', [(n, '') for n in CASES] + [('R18_FCOS_FPN', '_odd')])
def test_cpu_forward_gives_the_references_taps(name, suffix):
    """the same torch ops in the same order on the same weights: equal, not close"""
    gold, m = _gold(name), _model(name)
    x = torch.from_numpy(gold['x_codes' + suffix]).float() / 128 - 1
    with torch.no_grad():
        taps = m._backbone(x)
    assert [list(t.shape) for t in taps] == gold['tap_shapes' + suffix].tolist()
    for i, t in enumerate(taps):
        s = int(gold['tap_steps' + suffix][i])
        assert torch.equal(t[:, :, ::s, ::s], torch.from_numpy(gold['tap%d%s' % (i, suffix)])), i
    if suffix:
        assert [list(t.shape[2:]) for t in taps] == [[13, 19], [7, 10], [4, 5]]
    assert m._backbone.num_output_channels_list == [int(s[1]) for s in gold['tap_shapes' + suffix]]


@pytest.mark.parametrize('frozen_stages', [-1, 0, 2])
@pytest.mark.parametrize('norm_eval', [True, False])
def test_train_sets_the_references_freeze_and_norm_flags(frozen_stages, norm_eval):
    want = json.loads(str(_gold('module')['flags_fs%d_ne%d' % (frozen_stages, int(norm_eval))]))
    bb = ResNet(18, frozen_stages=frozen_stages, norm_eval=norm_eval)
    assert bb.train() is None                  # the quirk: train() / eval() return None
    assert sorted(k for k, p in bb.named_parameters() if p.requires_grad) == want['requires_grad']
    assert sorted(k for k, m in bb.named_modules() if m.training) == want['training']
    if frozen_stages >= 0:
        assert not bb.conv1.weight.requires_grad and not bb.norm1.training
    assert bb.layer3[0].bn1.training == (not norm_eval)


def test_eval_returns_none_like_the_reference():
    assert str(_gold('module')['eval_returns']) == 'None'
    assert ResNet(18).eval() is None


def test_constructor_attributes_and_assertions():
    bb = ResNet(34, out_indices=((3, 5), (1, 0), (2, 3)))
    assert bb.out_indices == [(1, 0), (2, 3), (3, 5)] and bb.num_stages == 3 and not hasattr(bb, 'layer4')
    assert bb.num_output_channels_list == [64, 128, 256] and bb.num_output_strides_list == [4, 8, 16]
    assert isinstance(bb.layer1, torch.nn.ModuleList) and bb.norm1 is bb.bn1 and bb.layer1[0].norm2 is bb.layer1[0].bn2
    assert ResNet(50).layer1[0].norm3.num_features == 256 and ResNet(50).num_output_channels_list == [256, 512, 1024, 2048]
    g = ResNet(18, norm_cfg=dict(type='GN', num_groups=32))
    assert g.norm1 is g.gn1 and isinstance(g.layer2[0].downsample[1], torch.nn.GroupNorm)
    for bad in (dict(depth=19), dict(depth=18, out_indices=((5, 0),)), dict(depth=18, out_indices=((1, 2),)),
                dict(depth=18, norm_cfg=dict(type='GN')), dict(depth=18, norm_cfg=dict(type='LN'))):
        with pytest.raises(AssertionError):
            ResNet(**bad)
    # zero_init_residual: the last norm of every block starts at 0, kaiming fan_out convs
    z = ResNet(18)
    assert all(not bool(b.norm2.weight.any()) for s in (z.layer1, z.layer4) for b in s) and bool(z.bn1.weight.eq(1).all())
    assert bool(ResNet(18, zero_init_residual=False).layer1[0].bn2.weight.eq(1).all())


def test_init_with_weight_file_loads_non_strictly_and_warns(tmp_path, capsys):
    src = ResNet(18, out_indices=((2, 1),))
    sd = {k: v + 1 for k, v in src.state_dict().items() if not k.startswith('layer2.1.')}
    sd['fc.weight'] = torch.zeros(3, 3)
    path = str(tmp_path / 'w.pth')
    torch.save(dict(state_dict=sd), path)
    bb = ResNet(18, out_indices=((2, 1),), init_with_weight_file=path)
    out = capsys.readouterr().out
    assert '[WARNING: ResNet pretrained weights load] missing keys:' in out and 'layer2.1.conv1.weight' in out
    assert '[WARNING: ResNet pretrained weights load] unexpected keys:' in out and 'fc.weight' in out
    assert torch.equal(bb.conv1.weight, sd['conv1.weight'])
    with pytest.raises(AssertionError):
        ResNet(18, init_with_weight_file=str(tmp_path / 'missing.pth'))


@pytest.mark.parametrize('depth,nblocks,first', [(18, 8, [0, 2, 4, 6]), (34, 16, [0, 3, 7, 13])])
def test_layer_walk(depth, nblocks, first):
    bb = ResNet(depth, out_indices=((4, 1), (2, 0), (3, 1)))
    net = netdesc.resnet_layers(bb)
    assert len(net.stem) == 2 and net.stem[1] == 'pool'
    s = net.stem[0]
    assert s.conv is bb.conv1 and s.norm is bb.bn1 and s.relu and (s.ks, s.stride) == (7, 2)
    assert len(net.blocks) == nblocks
    # a 1x1 stride-2 branch opens stages 2..4; stage 1 (64 -> 64, stride 1) has none
    assert [i for i, b in enumerate(net.blocks) if b.downsample is not None] == first[1:]
    assert [i for i, b in enumerate(net.blocks) if b.index == 0] == first
    for b in net.blocks:
        blk = getattr(bb, 'layer%d' % b.stage)[b.index]
        assert [l.conv for l in b.convs] == [blk.conv1, blk.conv2] and [l.norm for l in b.convs] == [blk.bn1, blk.bn2]
        assert all(l.relu and l.ks == 3 for l in b.convs) and b.convs[0].stride == (2 if b.downsample is not None else 1)
        if b.downsample is not None:
            d = b.downsample
            assert d.conv is blk.downsample[0] and d.norm is blk.downsample[1] and not d.relu and (d.ks, d.stride) == (1, 2)
    assert [(b.stage, b.index) for b in net.blocks if b.tap] == [(2, 0), (3, 1), (4, 1)] == bb.out_indices
    assert len(netdesc.resnet_layers(ResNet(50)).blocks[0].convs) == 3
    assert len(netdesc.resnet_layers(ResNet(18, deep_stem=True)).stem) == 4


def _unpack_stem7(packed):
    """plain loops over the layout include/lfd_hip.h documents for lfd_stem7_conv_f16's w_packed -> [64, 3, 7, 7]"""
    p = packed.float().numpy()
    assert p.shape == (2, 10, 64, 8)
    w = np.zeros((64, 3, 7, 7), np.float32)
    seen = np.zeros((64, 3, 7, 7), np.int64)
    for ct in range(2):
        for s in range(10):
            for lane in range(64):
                hk, col = lane // 32, lane % 32
                for j in range(8):
                    v = p[ct, s, lane, j]
                    if s < 7:
                        ky, e = s, 8 * hk + j
                    else:
                        i = 8 * (2 * (s - 7) + hk) + j
                        if i >= 35:
                            assert v == 0
                            continue
                        ky, e = i // 5, 16 + i % 5
                    w[32 * ct + col, e % 3, ky, e // 3] = v
                    seen[32 * ct + col, e % 3, ky, e // 3] += 1
    assert (seen == 1).all()
    return w


def test_pack_stem7_weight_round_trips():
    w = torch.randn(64, 3, 7, 7, generator=torch.Generator().manual_seed(5)).half().float()
    packed = engine_resnet.pack_stem7_weight(w)
    assert packed.dtype == torch.float16 and packed.numel() == _lib.lib().lfd_stem7_packed_weight_halfs() == 64 * 160
    assert np.array_equal(_unpack_stem7(packed), w.numpy())


def test_stem7_case_tables_hold_what_they_claim():
    """tests/golden/resnet_cases.py: the restated launch geometry is the kernel's, the walk gives every workgroup 1.5 tiles, the
    integer case stays inside fp16's integers, and the uint8 operands keep EVERY partial sum of a random summation order exact in
    fp32 (so the kernel's result does not depend on the order inside the MFMA)"""
    import resnet_cases as RC
    from conftest import ROOT
    src = open(os.path.join(ROOT, 'lfd-a-light-and-fast-detector_amd', 'csrc', 'stem7.hip')).read()
    assert 'MAX_WGS = %d }' % RC.MAX_WGS in src and 'PG = 2, PT = 2, TW = %d, TH = PG * PT' % RC.TW in src and RC.TH == 4
    assert 2 * RC.ntiles(*RC.WALK_SHAPE) == 3 * RC.MAX_WGS and all(v % 2 == 1 for v in RC.WALK_SHAPE[1:])
    x, wt, b = RC.int_operands(RC.SHAPES['ragged'], 1)
    assert float(x.abs().max()) == 2 and float(wt.abs().max()) == 1 and 2 * 147 + float(b.abs().max()) < 2048 and bool(b.ne(0).all())
    codes, wt, b = RC.u8_operands((1, 9, 11), 2)
    seen = RC.normalize_u8(codes).double()
    assert bool((seen * 2 ** 18 == (seen * 2 ** 18).round()).all()) and float(seen.abs().max()) <= 1
    xp = torch.zeros(1, 15, 17, 3, dtype=torch.float64)
    xp[:, 3:12, 3:14] = seen
    g = torch.Generator().manual_seed(3)
    for oy, ox in ((0, 0), (2, 3), (4, 5)):
        patch = xp[0, 2 * oy:2 * oy + 7, 2 * ox:2 * ox + 7].permute(2, 0, 1).reshape(147)          # [c][ky][kx] like OIHW
        terms = torch.cat([wt.reshape(64, 147).double() * patch, b.double()[:, None]], 1)
        order = torch.randperm(148, generator=g)
        partial = terms[:, order].cumsum(1)
        assert torch.equal(partial.float().double(), partial)
        ref = RC.conv_ref(seen.float(), wt, b)[0, oy, ox]
        assert torch.equal(partial[:, -1], ref)


def test_stem7_argument_checks_are_status_codes():
    import ctypes as C
    l = _lib.lib()
    buf = (C.c_char * 64)()
    al = C.c_void_p((C.addressof(buf) + 15) & ~15)
    assert l.lfd_stem7_conv_f16(None, 0, 1, 8, 8, al, al, al, None) == -1
    assert l.lfd_stem7_conv_f16(al, 0, 1, 8, 8, None, al, al, None) == -1
    assert l.lfd_stem7_conv_f16(al, 0, 1, 8, 8, al, None, al, None) == -1
    assert l.lfd_stem7_conv_f16(al, 0, 1, 8, 8, al, al, None, None) == -1
    for fmt, n, h, w in ((3, 1, 8, 8), (-1, 1, 8, 8), (0, 0, 8, 8), (1, 1, 0, 8), (2, 1, 8, 0)):
        assert l.lfd_stem7_conv_f16(al, fmt, n, h, w, al, al, al, None) == -1


def test_training_engine_declines_without_raising():
    for name in CASES:
        m = configs.build_resnet_model(name)
        m.train()
        assert train_engine.supported(m._backbone) is False
    m = configs.build_resnet_model('R18_LFD_SIMPLE')
    m.train()
    assert train_engine.network_supported(m) is False
    assert m._fused_plan_ok(torch.device('cpu')) is False


@pytest.mark.parametrize('kw,word', [(dict(depth=50), 'depth=50'), (dict(depth=18, deep_stem=True), 'deep_stem'),
                                     (dict(depth=18, norm_cfg=dict(type='GN', num_groups=32)), 'norm_cfg'),
                                     (dict(depth=18, dilations=(1, 1, 2, 2)), 'dilations'), (dict(depth=18, strides=(1, 2, 2, 1)), 'strides'),
                                     (dict(depth=18, base_channels=32), 'base_channels'), (dict(depth=18, in_channels=1), 'in_channels'),
                                     (dict(depth=34, avg_down=True), 'avg_down')])
def test_uncovered_options_raise_unsupported_naming_the_option(kw, word):
    with pytest.raises(engine.Unsupported, match=word):
        engine_resnet.check_covered(ResNet(**kw))
    engine_resnet.check_covered(ResNet(34, out_indices=((2, 0),)))


def test_fp32_storage_is_refused_with_a_message():
    m = _model('R18_LFD_SIMPLE')
    with pytest.raises(engine.Unsupported, match='fp32-tensor kernel'):
        engine_resnet.require_fp16_mode(m)


def test_backbones_are_told_apart_by_class_not_by_name():
    """a foreign class that happens to be called ResNet (torchvision's is) is not this package's: the layer engine refuses it
    with Unsupported instead of reading attributes it does not have; subclasses of the package's classes keep their plans"""
    from lfd_amd import engine_sibling
    from lfd_amd.model.backbone import LFDResNet

    class Mine(ResNet):
        pass

    foreign = type('ResNet', (torch.nn.Module,), {})()
    assert engine_resnet.is_resnet(Mine(18)) and not engine_resnet.is_resnet(foreign) and not engine_resnet.is_lfd_resnet(foreign)
    assert engine_resnet.is_lfd_resnet(type('Sub', (LFDResNet,), {}).__new__(type('Sub', (LFDResNet,), {})))
    assert train_engine.supported(foreign) is False
    with pytest.raises(engine.Unsupported, match='backbone ResNet'):
        engine_sibling.SiblingPlan(foreign, None, None, torch.device('cpu'))
