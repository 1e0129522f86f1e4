"""The 256-channel siblings (lfd_amd.configs.WIDE_SIBLINGS) on the host: the models build from this package's classes with the
reference's state_dict (tests/golden/wide_sibling_<case>.npz, made by tests/golden/make_golden_wide_siblings.py from the
reference classes), the fp16 inference plan builds and routes every layer as DESIGN 4i says, and what stays unsupported says so.
No device: the plans are built on CPU tensors."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from lfd_amd import configs, engine, engine_sibling, engine_sibling_p32, train_engine

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CPU = torch.device('cpu')
CASES = list(configs.WIDE_SIBLINGS)
LARGE, SMALL = engine_sibling.CONV256_MIN_PIXELS, engine_sibling.CONV256_MIN_PIXELS - 1

TOWER = [(256, 256, 3, 1)] * 4
# (where, cin, cout, ks, stride) in launch order -> the route on a batch of at least / fewer than CONV256_MIN_PIXELS pixels
EXPECTED = {
    'R18_FCOS_FPN256': (
        [('lateral0', 128, 256, 1, 1), ('lateral1', 256, 256, 1, 1), ('lateral2', 512, 256, 1, 1),
         ('out0', 256, 256, 3, 1), ('out1', 256, 256, 3, 1), ('out2', 256, 256, 3, 1), ('out3', 256, 256, 3, 2), ('out4', 256, 256, 3, 2)]
        + [('cls_t',) + t for t in TOWER] + [('reg_t',) + t for t in TOWER]
        + [('cls_o', 256, 128, 3, 1), ('ctr_o', 256, 32, 3, 1), ('reg_o', 256, 32, 3, 1)]),
    'LFDV2_SFPN256': (
        [('lateral0', 64, 256, 1, 1), ('lateral1', 64, 256, 1, 1), ('lateral2', 128, 256, 1, 1)]
        + [('cls_p', 256, 256, 3, 1)] * 2 + [('cls_p', 256, 32, 1, 1)] + [('reg_p', 256, 256, 3, 1)] * 2 + [('reg_p', 256, 32, 1, 1)]),
}


def _expected_route(layer, large):
    where, cin, cout, ks, stride = layer
    if where.endswith('_o') or cout == 32:
        return 'conv256_f32'                  # fp32 logits from 256 channels: csrc/conv256.hip at every size
    if cin == 256 and ks == 3 and stride == 1 and large:
        return 'conv256'
    return 'conv_wide'


def _state_sha(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(sd[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _plan(m):
    with torch.no_grad():
        return engine_sibling.SiblingPlan(m._backbone, m._neck, m._head, CPU)


@pytest.mark.parametrize('name', CASES)
def test_builds_with_the_reference_state_dict(name):
    gold = np.load(os.path.join(GOLDEN, 'wide_sibling_%s.npz' % name))
    m = configs.build_wide_sibling_model(name)
    sd = m.state_dict()
    assert [[k, list(v.shape)] for k, v in sd.items()] == json.loads(str(gold['keys']))
    assert _state_sha(sd) == str(gold['sha'])
    if name == 'R18_FCOS_FPN256':             # the class defaults: nothing but the class count and the input width is passed
        odd = np.load(os.path.join(GOLDEN, 'wide_sibling_%s_odd.npz' % name))
        assert str(odd['sha']) == str(gold['sha'])
        assert m._head._num_head_channels == 256 and m._head._num_layers == 4 and m._head._num_classes == 80


@pytest.mark.parametrize('name', CASES)
def test_the_fp16_plan_builds_and_routes_every_layer(name):
    """on the parent commit this fails with 'neck / head convs with more than 128 output channels'"""
    m = configs.build_wide_sibling_model(name).eval()
    plan = _plan(m)
    for pixels, large in ((LARGE, True), (SMALL, False), (8 * 135 * 240, True), (1, False)):
        got = plan.routes(pixels)
        assert [g[:5] for g in got] == EXPECTED[name]
        assert [g[5] for g in got] == [_expected_route(layer, large) for layer in EXPECTED[name]], pixels
    assert plan.laterals[0].cout == 256 and all(c in (32, 64, 128, 256, 512) for c in plan.tap_have)


def test_the_route_depends_on_the_shape_alone():
    """the crossover is one module constant; a layer's route is a function of (layer, pixel count)"""
    m = configs.build_wide_sibling_model('R18_FCOS_FPN256').eval()
    layer = _plan(m).levels[0]['cls_t'].ops[0]
    assert engine_sibling.CONV256_MIN_PIXELS == 12288
    assert layer.route(12288) == 'conv256' and layer.route(12287) == 'conv_wide'
    assert 8 * 34 * 60 >= engine_sibling.CONV256_MIN_PIXELS > 8 * 17 * 30      # between the maps DESIGN 4i measured


def test_a_320_channel_head_raises_naming_256():
    spec = dict(configs.WIDE_SIBLINGS['R18_FCOS_FPN256'])
    spec['head'] = dict(spec['head'], num_head_channels=320, norm_cfg=dict(type='GroupNorm', num_groups=40))
    m = configs.build_wide_sibling_model(spec).eval()
    with pytest.raises(RuntimeError, match=r'more than 256 output channels \(320\)'):
        _plan(m)


def test_groupnorm_16_of_256_raises_the_groupnorm_message():
    spec = dict(configs.WIDE_SIBLINGS['R18_FCOS_FPN256'])
    spec['head'] = dict(spec['head'], norm_cfg=dict(type='GroupNorm', num_groups=16))
    m = configs.build_wide_sibling_model(spec).eval()
    with pytest.raises(RuntimeError, match=r'GroupNorm\(16, 256\): the kernels take 8 channels per group'):
        _plan(m)


def test_a_192_channel_neck_is_padded_to_256():
    spec = dict(configs.WIDE_SIBLINGS['R18_FCOS_FPN256'])
    spec['neck'] = dict(spec['neck'], num_output_channels=192)
    spec['head'] = dict(spec['head'], num_head_channels=192, norm_cfg=dict(type='GroupNorm', num_groups=24))
    m = configs.build_wide_sibling_model(spec).eval()
    # GroupNorm runs on the un-padded width only (the statistics of a padded group would change): the towers refuse ...
    with pytest.raises(RuntimeError, match=r'GroupNorm\(24, 192\)'):
        _plan(m)
    # ... and without a norm the 192-channel convs run zero-padded to 256
    spec['head'] = dict(spec['head'], norm_cfg=None)
    plan = _plan(configs.build_wide_sibling_model(spec).eval())
    assert all(r[2] == 256 for r in plan.routes(LARGE) if r[0].startswith(('lateral', 'out', 'cls_t', 'reg_t')))


def test_fp32_storage_keeps_refusing():
    """(the ResNet of R18_FCOS_FPN256 is refused before a plan is built: tests/test_gpu_wide_siblings.py)"""
    m = configs.build_wide_sibling_model('LFDV2_SFPN256').eval()
    with torch.no_grad():
        for merge in (True, False):
            with pytest.raises(engine.Unsupported, match=r'more than 128 output channels \(256\)'):
                engine_sibling_p32.SiblingPrecisePlan(m, CPU, merge=merge)


@pytest.mark.parametrize('name', CASES)
def test_the_training_gates_answer_false_without_raising(name):
    m = configs.build_wide_sibling_model(name)
    m.train()
    assert train_engine.pyramid_supported(m._backbone, m._neck) is False
    assert train_engine.network_supported(m) is False
    assert isinstance(m._head, nn.Module)
