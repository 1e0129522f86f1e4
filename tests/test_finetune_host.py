"""Fine-tuning on the HIP training path, host side: which models train_engine admits with frozen_stages / norm_eval, the unit
flags of their schedules, and the float64 restatement of the eval-mode BatchNorm backward (tests/golden/norm_eval_cases.py) against
float64 autograd.  No GPU."""
import pytest
import torch
import torch.nn as nn

import norm_cases as NC
import norm_eval_cases as NE
from lfd_amd import configs, train_engine as te

MODELS = [('WIDERFACE_LFD_XS', 3), ('WIDERFACE_LFD_S', 3), ('TT100K_LFD_L', 3), ('WIDERFACE_LFD_XS', 1)]


def _options(name):
    stages = len(configs.ARCHS[name]['body_architecture'])
    last = max(s for s, _ in configs.ARCHS[name]['out_indices']) + 1      # LFDResNet keeps the stages up to its last tap
    out = []
    for k in (1, 2, min(stages, last)):
        out += [dict(frozen_stages=k), dict(frozen_stages=k, norm_eval=True)]
    return out + [dict(norm_eval=True)]


@pytest.mark.parametrize('name,cin', MODELS)
def test_frozen_stages_and_norm_eval_models_are_admitted_with_matching_unit_flags(name, cin):
    for kw in _options(name):
        m = configs.build_model(name, input_channels=cin, **kw).train()
        bb = m._backbone
        assert te.network_supported(m), (name, kw)
        units, outs = te.build_network(m)
        k = kw.get('frozen_stages', -1)
        frozen_convs = {id(c) for fm in te.frozen_modules(bb) for c in fm.modules() if isinstance(c, nn.Conv2d)}
        assert len(te.frozen_modules(bb)) == (1 + k if k > 0 else 0)
        backbone = [u for u in units if u.level is None]
        # the flags are the modules' state
        for u in units:
            assert u.eval_norm == (isinstance(u.norm, nn.BatchNorm2d) and not u.norm.training)
            assert u.frozen == (id(u.conv) in frozen_convs)
            if u.frozen:
                assert u.eval_norm and not any(p.requires_grad for p in (u.conv.weight, u.norm.weight, u.norm.bias))
            else:
                assert all(p.requires_grad for p in (u.conv.weight, u.norm.weight, u.norm.bias))
            if u.level is not None:                  # neck and head: no such option
                assert not u.frozen and not u.eval_norm and u.norm.training
            elif kw.get('norm_eval'):
                assert u.eval_norm
        # frozen units: a contiguous prefix of the backbone chain, downsample convs of the frozen stages included
        flags = [u.frozen for u in backbone]
        nf = sum(flags)
        assert nf == len(frozen_convs) and (nf > 0) == (k > 0) and flags == [True] * nf + [False] * (len(flags) - nf)
        for si in range(k):
            ds = getattr(bb, 'stage%d' % si)[0]._downsample[0]
            assert [u for u in units if u.conv is ds][0].frozen
        ps = te.network_params(units, outs)
        assert len({id(p) for p in ps}) == len(ps)
        assert {id(p) for p in ps} == {id(p) for p in m.parameters() if p.requires_grad}, (name, kw)
        assert {id(p) for p in te.backbone_params(backbone)} == {id(p) for p in bb.parameters() if p.requires_grad}
        for a, b in list(te._stem_pairs(units, outs).items()) + list(te._deferred_units(units, outs).items()):
            assert not (units[a].frozen or units[a].eval_norm or units[b].frozen or units[b].eval_norm)
        dead = te.dead_activations(units)
        assert dead == {0} | {u.dst for u in units if u.frozen}


def test_unfrozen_models_keep_their_schedule_and_other_freezes_stay_on_autograd():
    m = configs.build_model('WIDERFACE_LFD_S').train()
    units, outs = te.build_network(m)
    assert not any(u.frozen or u.eval_norm for u in units)
    assert te._stem_pairs(units, outs) == {0: 1, 2: 3}
    assert [id(p) for p in te.network_params(units, outs)] and {id(p) for p in te.network_params(units, outs)} == {id(p) for p in m.parameters()}
    assert te.dead_activations(units) == {0}
    # state that is not what train() produces from the constructor's options
    f = configs.build_model('WIDERFACE_LFD_XS', frozen_stages=1).train()
    assert te.supported(f._backbone)
    f._backbone.stage0[0]._conv1.weight.requires_grad_(True)               # thawed inside a frozen stage
    assert not te.supported(f._backbone)
    f._backbone.stage0[0]._conv1.weight.requires_grad_(False)
    f._backbone.stage1[0]._conv1.weight.requires_grad_(False)              # frozen outside the frozen stages
    assert not te.supported(f._backbone) and not te.network_supported(f)
    f._backbone.stage1[0]._conv1.weight.requires_grad_(True)
    f._backbone.stage1[0]._norm1.eval()                                    # a norm switched by hand
    assert not te.supported(f._backbone)
    f._backbone.stage1[0]._norm1.train()
    f._backbone._stem[1].train()                                           # a frozen stage's norm back in training mode
    assert not te.supported(f._backbone)
    f.train()
    assert te.network_supported(f)
    f._neck.neck0[1].eval()                                                # the neck has no eval option
    assert not te.network_supported(f) and te.supported(f._backbone)
    f.train()
    f.eval()
    assert not te.supported(f._backbone) and not te.network_supported(f)
    e = configs.build_model('WIDERFACE_LFD_XS', norm_eval=True)
    e.eval()
    assert not te.supported(e._backbone)                                   # (a model in eval() does not train)
    e.train()
    assert te.network_supported(e)
    e._backbone.stage2[0]._norm2.train()
    assert not te.supported(e._backbone)
    # TrafficLight: the backbone node under an autograd neck / head takes the same options
    tl = configs.build_model('TL_LFD_L', frozen_stages=1).train()
    assert te.supported(tl._backbone) and not te.network_supported(tl)
    units, taps = te.build_units(tl._backbone)
    assert {id(p) for p in te.backbone_params(units)} == {id(p) for p in tl._backbone.parameters() if p.requires_grad}
    assert configs.build_model('WIDERFACE_LFD_XS')._backbone._frozen_stages == -1          # defaults unchanged


def test_float64_reference_leaves_almost_no_recomputed_mask_undecided():
    per, und, total = NE.undecided_census()
    print('undecided recomputed masks per case:', per)
    assert und <= NE.UNDECIDED_FRACTION * total
    for name, (u, n) in per.items():
        assert u == 0 or n >= NE.UNDECIDED_FREE_BELOW, name


@pytest.mark.parametrize('name', [c[0] for c in NE.BWD_CASES])
def test_eval_backward_restatement_equals_float64_autograd(name):
    """relu(bn_eval(y) + res) differentiated by torch.autograd in float64 against norm_eval_cases.bn_eval_backward_ref"""
    d = NE.bwd_inputs(name)
    c = d['c']
    flat = lambda t: None if t is None else t.reshape(-1, c)
    stats = NE.stats_row(d['running_mean'], d['running_var'])
    mean, rstd = NC.split_stats(stats)
    y = flat(d['y']).double().requires_grad_(True)
    gamma, beta = d['gamma'].double().requires_grad_(True), d['beta'].double().requires_grad_(True)
    res = None if d['res'] is None else flat(d['res']).double().requires_grad_(True)
    z = (y - mean) * rstd * gamma + beta
    pre = z
    if res is not None:
        z = z + res
    if d['mode'] != 'none':
        z = torch.relu(z)
    dz = flat(d['dz']).double()
    z.backward(dz)
    zref = NE.forward_ref(d, stats)
    torch.testing.assert_close(zref, z.detach(), rtol=1e-12, atol=1e-13)
    mask, und = NE.mask_of(d, stats, z.detach())
    if d['mode'] == 'y':
        assert torch.equal(mask[~und], (pre.detach() > 0)[~und])
    inv = 1.0 / NC.LOSS_SCALE
    r = NE.bn_eval_backward_ref(flat(d['dz']), flat(d['y']), mask, stats, d['gamma'], inv)
    tight = dict(rtol=1e-12, atol=1e-14)
    torch.testing.assert_close(r['dy'], y.grad, **tight)
    torch.testing.assert_close(r['dgamma'], gamma.grad * inv, **tight)
    torch.testing.assert_close(r['dbeta'], beta.grad * inv, **tight)
    if res is not None:
        assert torch.equal(r['g'], res.grad)
    bounds = NE.bn_eval_backward_bounds(r, NE.chain_of(d), inv, NE.PREV_DGAMMA if d['accumulate'] else None,
                                        NE.PREV_DBETA if d['accumulate'] else None)
    assert all(bool((b >= 0).all()) and bool(torch.isfinite(b).all()) for b in bounds)
    assert bounds[0].shape == r['dy'].shape and bounds[1].shape == (c,)


def test_eval_statistics_reference_is_batchnorm_in_eval_mode():
    for name, widths in NE.STATS_TABLES:
        for (rm, rv), c in zip(NE.stats_inputs(name), widths):
            bn = nn.BatchNorm2d(c).double().eval()
            with torch.no_grad():
                bn.running_mean.copy_(rm)
                bn.running_var.copy_(rv)
            x = torch.randn(2, c, 3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(c))
            mean, rstd = NE.eval_stats_ref(rm, rv, bn.eps)
            torch.testing.assert_close(bn(x), (x - mean.view(1, -1, 1, 1)) * rstd.view(1, -1, 1, 1), rtol=1e-12, atol=1e-12)
            assert int(bn.num_batches_tracked) == 0


def test_job_table_mirrors_match_the_header_layout(tmp_path):
    """lfd_bn_eval_job_t / lfd_bn_fold_job_t cross the ABI as device-resident tables: sizeof and every field offset as gcc sees
    them == the ctypes mirrors (the check tests/test_abi.py makes for the older structs)"""
    import ctypes as C
    import os
    import subprocess
    from conftest import ROOT
    from lfd_amd import _lib
    pairs = {'lfd_bn_eval_job_t': _lib.BnEvalJob, 'lfd_bn_fold_job_t': _lib.BnFoldJob}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lfd_hip.h"', 'int main(void) {']
    for cname, mirror in pairs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in mirror._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['return 0; }']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True, capture_output=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, mirror in pairs.items():
        assert int(got[cname]) == C.sizeof(mirror), cname
        for fname, _ in mirror._fields_:
            assert int(got['%s.%s' % (cname, fname)]) == getattr(mirror, fname).offset, (cname, fname)
