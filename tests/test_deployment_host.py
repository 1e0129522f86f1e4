"""Host logic of the INT8 deployment mode (lfd_amd/deployment.py, lfd_amd/engine_i8.py): the calibrator's batching, the cache, the
weight and epilogue constants of the contract, the plan's layer list, and the refusals.  No GPU."""
import json

import numpy as np
import pytest
import torch

import lfd_amd
from conftest import load_golden
from lfd_amd import INT8Calibrator, build_int8_engine, configs, deployment, engine, engine_i8, netdesc
from lfd_amd.model import LFD


def test_calibrator_batches_and_none_at_the_end(tmp_path):
    data = np.arange(7 * 3 * 4 * 5, dtype=np.float32).reshape(7, 3, 4, 5)
    cal = INT8Calibrator(data, str(tmp_path / 'c.json'), batch_size=3, device='cpu')
    assert cal.get_batch_size() == 3
    a, b = cal.get_batch([]), cal.get_batch(['input'])
    assert isinstance(a, torch.Tensor) and a.dtype == torch.float32 and tuple(a.shape) == (3, 3, 4, 5)
    assert np.array_equal(a.numpy(), data[:3]) and np.array_equal(b.numpy(), data[3:6])
    assert cal.get_batch([]) is None and cal.get_batch([]) is None           # one frame is left: fewer than a batch
    assert INT8Calibrator(data, 'x', batch_size=8, device='cpu').get_batch([]) is None
    assert INT8Calibrator(data, 'x').get_batch_size() == 8                   # the reference's default
    # the reference's asserts on the data
    with pytest.raises(AssertionError):
        INT8Calibrator(data.astype(np.float64), 'x')
    with pytest.raises(AssertionError):
        INT8Calibrator(data[0], 'x')
    # a Fortran-ordered array is taken in C order
    f = INT8Calibrator(np.asfortranarray(data), 'x', batch_size=7, device='cpu').get_batch([])
    assert f.is_contiguous() and np.array_equal(f.numpy(), data)


def test_cache_round_trip_and_a_cache_for_other_weights_is_ignored(tmp_path):
    path = str(tmp_path / 'cal.json')
    cal = INT8Calibrator(np.zeros((1, 3, 8, 8), np.float32), path)
    assert cal.read_calibration_cache() is None
    names = ['stem', 'stage0.block0.conv1']
    amax = {'stem': 2.7182818284590451, 'stage0.block0.conv1': 0.1}
    blob = deployment.encode_cache('ab' * 32, amax)
    cal.write_calibration_cache(blob)
    assert cal.read_calibration_cache() == blob
    d = json.loads(blob.decode('utf-8'))
    assert d['format'] == deployment.CACHE_FORMAT and d['version'] == deployment.CACHE_VERSION == 1 and d['state_sha256'] == 'ab' * 32
    assert deployment.decode_cache(blob, 'ab' * 32, names) == amax            # floats survive bit for bit
    assert deployment.decode_cache(blob, 'cd' * 32, names) is None            # other weights
    assert deployment.decode_cache(blob, 'ab' * 32, names + ['stage0.block0.conv2']) is None     # another layer list
    assert deployment.decode_cache(blob, 'ab' * 32, names[:1]) is None
    assert deployment.decode_cache(b'TRT-7103-EntropyCalibration2\n', 'ab' * 32, names) is None   # not this format
    assert deployment.decode_cache(blob.replace(b'"version": 1', b'"version": 2'), 'ab' * 32, names) is None
    # the sha is the one the fixtures carry (tests/test_gpu_resnet.py: _state_sha)
    m = configs.build_model('WIDERFACE_LFD_XS', seed=666)
    configs.perturb_weights(m, seed=1)
    g = load_golden('ref_model_WIDERFACE_LFD_XS.npz')
    assert deployment.state_sha256(m.state_dict()) == str(g['sha'])


def test_weight_scale_rules():
    w = torch.zeros(4, 3, 3, 3)
    w[0] = torch.linspace(-2.54, 1.0, 27).reshape(3, 3, 3)
    w[1, 0, 0, 0] = 1e-3
    w[3] = torch.linspace(-1.0, 0.5, 27).reshape(3, 3, 3)
    s_w, q = engine_i8.weight_scales(w)
    assert s_w.dtype == torch.float64 and q.dtype == torch.int8
    assert float(s_w[0]) == float(w[0].double().abs().max()) / 127 and float(s_w[2]) == 1.0       # a zero row: scale 1
    assert int(q[0].min()) == -127 and int(q[1, 0, 0, 0]) == 127 and int(q[1].abs().sum()) == 127 and not bool(q[2].any())
    assert torch.equal(q.double(), torch.round(w.double() / s_w.view(-1, 1, 1, 1)).clamp(-127, 127))
    assert int(q[3].min()) == -127 and int(q[3].max()) == 64                                      # symmetric: 0.5 / (1 / 127) = 63.5 -> 64


def test_plan_layers_scales_of_padded_channels_and_constants():
    m = configs.build_model('TL_LFD_S', seed=666)            # 48-channel stem and first stage: padded to 64
    configs.perturb_weights(m, seed=1)
    m.eval()
    plan = engine_i8.Int8Plan(m._backbone, m._neck, m._head, torch.device('cpu'))
    blocks = netdesc.backbone_layers(m._backbone).blocks
    assert len(plan.layers) == sum(len(b.convs) + (b.downsample is not None) for b in blocks)
    assert plan.tensor_names == ['stem'] + [c.name for c in plan.layers] and len(set(plan.tensor_names)) == len(plan.tensor_names)
    first = plan.layers[0]
    assert (first.name, first.ks, first.stride, first.relu, first.res) == ('stage0.block0.downsample', 1, 2, False, None)
    c1, c2 = plan.layers[1], plan.layers[2]
    assert (c1.src, c1.res, c1.relu) == (0, None, True) and (c2.src, c2.res, c2.res_name) == (c1.dst, first.dst, first.name)
    assert (first.cin, first.cout, first.cout_real) == (64, 64, 48)
    assert float(first.ref_w[48:].abs().max()) == 0 and float(first.ref_w[:, 48:].abs().max()) == 0
    assert bool((first.s_w[48:] == 1).all()) and not bool(first.q_w[48:].any()) and not bool(first.q_w[:, 48:].any())
    assert [c.tap is not None for c in plan.layers].count(True) == len(plan.taps) == len(m._point_strides)
    assert all(plan.layers[i - 1 - len(plan.convs)].tap is not None for i in plan.tap_ready_after)
    # the parent's fold, the plan's padding
    w, b = engine._fold_conv_norm(blocks[0].downsample.conv, blocks[0].downsample.norm)
    assert torch.equal(first.ref_w[:48, :48], w) and torch.equal(first.ref_b[:48], b)
    # no scales yet: running is an error, not a silent fp16 forward
    with pytest.raises(RuntimeError, match='no scales'):
        plan.run_backbone(None, 0, None)
    with pytest.raises(KeyError):
        plan.set_scales({'stem': 1.0})
    amax = dict((k, 0.5 + 0.25 * i) for i, k in enumerate(plan.tensor_names))
    amax[c1.name] = 0.0                                       # a dead tensor: scale 1
    plan.set_scales(amax)
    assert plan.scales[c1.name] == (0.0, 1.0) and plan.scales['stem'] == (0.5, 0.5 / 127)
    s_in, s_out, s_res = plan.scales[c2.src_name][1], plan.scales[c2.name][1], plan.scales[first.name][1]
    assert (c2.s_in, c2.s_out, c2.s_res) == (1.0, s_out, s_res)
    assert torch.equal(c2.mult, (c2.s_w * s_in / s_out).float()) and torch.equal(c2.biasq, (c2.ref_b.double() / s_out).float())
    assert c2.res_mult == float(np.float32(s_res / s_out)) and first.res_mult == 0.0
    assert plan.inv_stem_scale == float(np.float32(127 / 0.5))


def test_epilogue_constants_of_a_hand_made_layer():
    s_w = torch.tensor([0.5, 1.0, 1.0 / 3], dtype=torch.float64)
    bias = torch.tensor([1.0, -0.25, 0.1])
    mult, biasq, res_mult = engine_i8.epilogue_constants(0.1, s_w, bias, 0.3, 0.7)
    assert mult.dtype == biasq.dtype == torch.float32
    assert mult.tolist() == [float(np.float32(0.5 * 0.1 / 0.3)), float(np.float32(0.1 / 0.3)), float(np.float32(1.0 / 3 * 0.1 / 0.3))]
    assert biasq.tolist() == [float(np.float32(1.0 / 0.3)), float(np.float32(-0.25 / 0.3)), float(np.float32(np.float64(np.float32(0.1)) / 0.3))]
    assert res_mult == float(np.float32(0.7 / 0.3))
    assert engine_i8.epilogue_constants(0.1, s_w, bias, 0.3)[2] == 0.0
    assert engine_i8.act_scale(0.0) == 1.0 and engine_i8.act_scale(254.0) == 2.0


def _raises(model, pattern):
    with pytest.raises(engine.Unsupported, match=pattern):
        build_int8_engine(model, INT8Calibrator(np.zeros((1, 3, 32, 32), np.float32), '/nonexistent/cache.json'))


def test_unsupported_configurations_are_named():
    _raises(configs.build_sibling_model('FCOS_FPN').eval(), 'LFD models only, not FCOS')
    _raises(configs.build_sibling_model('LFDV2_SFPN').eval(), 'LFD models only, not LFDv2')
    _raises(configs.build_resnet_model('R18_LFD_SIMPLE').eval(), 'LFDResNet backbone only, not ResNet')
    _raises(configs.build_model(configs.PRESETS['fast_fast_fast']).eval(), 'more than 128 channels')
    m = configs.build_model('WIDERFACE_LFD_XS').eval()
    m.precision = 'fp32_storage'
    _raises(m, "precision is 'fp32_storage'")
    m.precision = 'fp16'
    fpn = configs.build_sibling_model('LFDV2_SFPN')
    m2 = configs.build_model('WIDERFACE_LFD_XS').eval()
    m2._neck = fpn._neck
    _raises(m2, 'SimpleNeck only, not SimpleFPN')
    # nothing silent: a supported model on the CPU is an error too, and so is a missing calibrator
    with pytest.raises(RuntimeError, match='must be on the MI355X'):
        build_int8_engine(m, INT8Calibrator(np.zeros((1, 3, 32, 32), np.float32), '/nonexistent/cache.json'))
    with pytest.raises(AssertionError, match='calibrator is not provided'):
        build_int8_engine(m, None)


def test_public_names_and_precisions_unchanged():
    assert LFD.PRECISIONS == ('fp16', 'fp32_storage')
    assert lfd_amd.INT8Calibrator is deployment.INT8Calibrator and lfd_amd.build_int8_engine is deployment.build_int8_engine
    assert lfd_amd.Int8Engine is deployment.Int8Engine
    with pytest.raises(AttributeError):
        lfd_amd.no_such_name
    for name in ('forward', 'forward_resident', 'detect', 'get_results', 'scales', '__call__'):
        assert hasattr(deployment.Int8Engine, name)
