"""Host-side checks (no GPU) for LFDResNet's own presets on the HIP path: every layer of all 27 (block, stem, body) combinations,
and of a 192-channel custom body (zero-padded to 256), has a kernel behind lfd_conv2d_nhwc_f16 -- asked through
lfd_conv2d_nhwc_f16_supported, the dispatch of the real call without a launch; width 640 is refused; the other engines and
training keep their 128-channel limit; the fixtures' weights are the ones this package rebuilds from the seed; the integer
operands of tests/golden/conv_wide_cases.py keep every reference output inside fp16's exact integers."""
import itertools
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import conv_cases as CC
import conv_wide_cases as WC
from lfd_amd import configs, engine, engine_p32, ops, train_engine
from lfd_amd.model.backbone import LFDResNet
from lfd_amd.model.neck import SimpleNeck

MODES = ('fast', 'faster', 'fastest')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def _backbone(block, stem, body, **kw):
    ba = configs.PRESET_BODY_ARCHITECTURES[body] if body is not None else kw['body_architecture']
    return LFDResNet(block_mode=block, stem_mode=stem, body_mode=body, out_indices=tuple((i, n - 1) for i, n in enumerate(ba)), **kw)


def _layers(bb):
    """(cin, cout, ks, stride) of every conv of the backbone but the one on the frame, and of a SimpleNeck(128) on its taps,
    channels as the engine pads them"""
    neck = SimpleNeck(num_neck_channels=128, num_input_channels_list=bb.num_output_channels_list,
                      num_input_strides_list=bb.num_output_strides_list, norm_cfg=dict(type='BatchNorm2d'),
                      activation_cfg=dict(type='ReLU', inplace=True))
    out = []
    for part in (bb, neck):
        for m in part.modules():
            if isinstance(m, nn.Conv2d) and m is not bb._stem[0]:
                out.append((engine.pad_channels(m.in_channels), engine.pad_channels(m.out_channels), m.kernel_size[0], m.stride[0]))
    return out


@pytest.mark.parametrize('block,stem,body', list(itertools.product(MODES, MODES, MODES)))
def test_every_layer_of_every_preset_has_a_kernel(block, stem, body):
    bb = _backbone(block, stem, body)
    layers = _layers(bb)
    assert len(layers) >= 15
    for cin, cout, ks, stride in layers:
        assert ops.conv2d_supported(cin, cout, ks, stride), (cin, cout, ks, stride)
    # and what the plan really launches, chained 1x1s and downsample pairs included
    plan = engine.EnginePlan(bb, device=torch.device('cpu'))
    for c in plan.convs:
        assert ops.conv2d_supported(c.cin, c.cout, c.ks, c.stride, tail=c.tail is not None), (c.cin, c.cout, c.ks, c.stride, c.tail is not None)
        if c.ds is not None or c.tail is not None:
            assert not engine.wide_conv(c.cin, c.cout, c.ks, c.stride)
    if max(bb._body_channels) > 128:          # training is unchanged: those models stay on the autograd route
        assert not train_engine.supported(bb.train())


def test_a_192_channel_body_runs_padded_to_256_and_640_is_refused():
    for block in MODES:
        bb = _backbone(block, 'fast', None, body_architecture=[1, 1, 2], body_channels=[64, 128, 192])
        layers = _layers(bb)
        assert any(256 in l[:2] for l in layers)
        for cin, cout, ks, stride in layers:
            assert ops.conv2d_supported(cin, cout, ks, stride), (cin, cout, ks, stride)
        assert not train_engine.supported(bb.train())
    assert engine.pad_channels(192) == 256 and engine.pad_channels(257) == 512
    with pytest.raises(engine.Unsupported, match='more than 512 channels'):
        engine.pad_channels(640)
    for ks, stride in ((1, 1), (3, 1), (3, 2), (1, 2)):
        assert not ops.conv2d_supported(640, 128, ks, stride) and not ops.conv2d_supported(128, 640, ks, stride)
        assert not ops.conv2d_supported(640, 640, ks, stride)
    assert not ops.conv2d_supported(160, 256, 3, 1)          # the wide kernel moves the input in chunks of 64 channels


def test_fp32_storage_plans_refuse_wide_backbones_by_name():
    m = configs.build_model(configs.PRESETS['faster_faster_faster'])
    with pytest.raises(engine.Unsupported, match="'fp16' mode"):
        engine.require_narrow(m._backbone, "precision='fp32_storage'")
    with pytest.raises(engine.Unsupported, match="'fp16' mode"):
        engine_p32.PrecisePlan(m, torch.device('cpu'))
    engine.require_narrow(configs.build_model('WIDERFACE_LFD_S')._backbone, "precision='fp32_storage'")


@pytest.mark.parametrize('name', list(configs.PRESETS))
def test_fixture_weights_are_rebuilt_from_the_seed(name):
    import hashlib
    gold = np.load(os.path.join(GOLDEN, 'presets_%s.npz' % name))
    m = configs.build_model(configs.PRESETS[name])
    configs.perturb_weights(m)
    h = hashlib.sha256()
    sd = m.state_dict()
    for k in sd:
        h.update(k.encode())
        h.update(sd[k].detach().cpu().contiguous().numpy().tobytes())
    assert h.hexdigest() == str(gold['sha'])
    assert gold['x_codes'].shape == (2, 3, 128, 192) and gold['x_codes'].dtype == np.uint8
    assert all(os.path.getsize(os.path.join(GOLDEN, f)) < 2 ** 20 for f in os.listdir(GOLDEN) if f.startswith('presets_'))


@pytest.mark.parametrize('c', [c for c in WC.wide_cases() if c.kind != 'walk'], ids=WC.case_id)
def test_integer_references_stay_inside_fp16_exact_integers(c):
    """(float32 on the CPU: every partial sum is an integer below 2^24, so it is the float64 value)"""
    o = WC.int_operands(c)
    ref = CC.conv_ref(o.x, o.w, o.b, c.stride, residual=o.res if c.res else None, dtype=torch.float32)
    assert 0 < float(ref.abs().max()) <= CC.F16_EXACT
    assert WC.X_HI * WC.W_HI * c.ks * c.ks * c.cin + WC.BIAS_HI + WC.RES_HI < CC.F32_EXACT
