"""Grayscale (input_channels=1) models on the HIP training path -- what holds without a device: the gray twins of the shipped
configurations are covered by train_engine (backbone and whole network), other channel counts and the 48-channel stem are
not, the C ABI declares the gray first-conv training entry points, and the module mirrors reproduce the REAL reference's gray
training iteration (tests/golden/make_golden_train_step_gray.py) on CPU, as test_train_golden.py does for RGB."""
import hashlib
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from lfd_amd import _lib, configs, train, train_engine
import train_step_gray_cases as cases

GRAY_HIP = ['WIDERFACE_LFD_S', 'WIDERFACE_LFD_XS', 'WIDERFACE_LFD_M', 'WIDERFACE_LFD_L', 'TT100K_LFD_S', 'TT100K_LFD_L']


@pytest.mark.parametrize('name', GRAY_HIP)
def test_gray_twins_run_on_the_hip_training_path(name):
    m = configs.build_model(name, input_channels=1).train()
    assert m._backbone._input_channels == 1 and m._backbone._stem[0].in_channels == 1
    assert train_engine.supported(m._backbone)
    assert train_engine.network_supported(m)
    rgb = configs.build_model(name).train()
    assert train_engine.supported(rgb._backbone) and train_engine.network_supported(rgb)


def test_what_stays_on_autograd():
    m = configs.build_model('TL_LFD_S', input_channels=1).train()         # 48-channel stem
    assert not train_engine.supported(m._backbone) and not train_engine.network_supported(m)
    for c in (2, 4):
        m = configs.build_model('WIDERFACE_LFD_S', input_channels=c).train()
        assert not train_engine.supported(m._backbone) and not train_engine.network_supported(m)
    # one input plane is accepted for the first stem conv only
    conv = torch.nn.Conv2d(1, 64, 3, 1, 1)
    assert train_engine._conv_ok(conv, first=True) and not train_engine._conv_ok(conv)


def test_gray_training_input_is_checked():
    m = configs.build_model('WIDERFACE_LFD_XS', input_channels=1).train()
    train_engine.check_train_input(m._backbone, torch.zeros(2, 1, 32, 32))
    with pytest.raises(RuntimeError, match=r'\[N,1,H,W\]'):
        train_engine.check_train_input(m._backbone, torch.zeros(2, 3, 32, 32))
    rgb = configs.build_model('WIDERFACE_LFD_XS').train()
    with pytest.raises(RuntimeError, match=r'\[N,3,H,W\]'):
        train_engine.check_train_input(rgb._backbone, torch.zeros(2, 1, 32, 32))


NEW_SYMBOLS = ['lfd_stem_gray_train_fwd', 'lfd_stem_gray_train_fwd_bn_stats', 'lfd_stem_gray_wgrad', 'lfd_stem_gray_bn_bwd_wgrad_rows']


def test_gray_training_entry_points_are_declared():
    header = open(os.path.join(ROOT, 'include', 'lfd_hip.h')).read()
    for s in NEW_SYMBOLS:
        assert re.search(r'LFD_API int %s\(' % s, header), s
        assert s in _lib.declared_symbols(), s


def _sha(sd):
    h = hashlib.sha256()
    for k in sd:
        h.update(k.encode())
        h.update(sd[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _summary(t):
    f = t.detach().double().reshape(-1).cpu()
    head = torch.zeros(4, dtype=torch.float64)
    head[:min(4, f.numel())] = f[:4]
    return np.concatenate([[float(f.norm()), float(f.mean())], head.numpy()])


def _close_summaries(got, want, names, rtol, what):
    for g, w, k in zip(got, want, names):
        scale = max(abs(w[0]), 1e-12)
        assert abs(g[0] - w[0]) <= rtol * scale, (what, k, 'norm', g[0], w[0])
        np.testing.assert_allclose(g[1:], w[1:], rtol=rtol, atol=rtol * scale, err_msg='%s %s' % (what, k))


@pytest.mark.parametrize('name', list(cases.CASES))
def test_mirror_modules_reproduce_the_reference_gray_training_iteration_on_cpu(name):
    """the gates of test_train_golden's CPU test: outputs, gradients, the hook's gradient norm and the updated state"""
    g = load_golden('ref_train_step_%s.npz' % cases.file_tag(name))
    m = configs.build_model(name, input_channels=1)
    configs.perturb_weights(m, seed=1)
    m.train()
    assert _sha(m.state_dict()) == str(g['sha'])
    assert [k for k, _ in m.named_parameters()] == [str(k) for k in g['param_names']]
    cls, reg = m(cases.images(name))
    assert [tuple(m.head_indexes_to_feature_map_sizes[i]) for i in range(len(g['sizes']))] == [tuple(s) for s in g['sizes'].tolist()]
    np.testing.assert_allclose(cls.detach().numpy(), g['cls'], rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(reg.detach().numpy(), g['reg'], rtol=1e-5, atol=2e-6)
    loss = (cls * torch.from_numpy(g['dcls'])).sum() + (reg * torch.from_numpy(g['dreg'])).sum()
    opt = torch.optim.SGD(m.parameters(), lr=cases.LR, momentum=cases.MOMENTUM, weight_decay=cases.WEIGHT_DECAY)
    hook = train.OptimizerHook(dict(cases.GRAD_CLIP), training_epochs=1000)

    class Executor(object):
        config_dict = dict(model=m, optimizer=opt, loss=loss, epoch=0)
    hook.after_train_iter(Executor)
    norm = float(Executor.config_dict['grad_norm'])
    assert norm == pytest.approx(float(g['grad_norms'][0]), rel=1e-5)
    coef = min(1.0, cases.GRAD_CLIP['max_norm'] / (norm + 1e-6))
    names = [k for k, _ in m.named_parameters()]
    _close_summaries([_summary(p.grad / coef) for _, p in m.named_parameters()], g['grad_summary'], names, 2e-5, 'gradient')
    assert g['grad_summary'][0].shape == (6,) and m._backbone._stem[0].weight.shape[1] == 1
    for k, p in m.named_parameters():
        if p.dim() <= 1:
            w = g['grad/' + k]
            np.testing.assert_allclose((p.grad / coef).numpy(), w, rtol=2e-5, atol=2e-5 * float(np.abs(w).max() + 1e-12), err_msg=k)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g['state_names']]
    _close_summaries([_summary(v) for v in sd.values()], g['state_summary_0'], list(sd.keys()), 1e-6, 'state after the update')
