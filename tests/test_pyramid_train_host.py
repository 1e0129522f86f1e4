"""Host side of the backbone + pyramid-neck training node (train_engine.pyramid_supported / build_pyramid): which
configurations it admits, what it refuses, and the plan itself -- step order and gradient fan-in -- without a GPU."""
import pytest
import torch.nn as nn

import sibling_cases as SC
from lfd_amd import configs, train_engine as te
from lfd_amd.model import backbone as B, neck as N


def _backbone():
    k = configs.SIBLING_BACKBONE
    return B.LFDResNet(block_mode=k['block_mode'], stem_mode=k['stem_mode'], body_mode=None, input_channels=3,
                       stem_channels=k['stem_channels'], body_architecture=list(k['body_architecture']),
                       body_channels=list(k['body_channels']), out_indices=k['out_indices'], frozen_stages=-1,
                       activation_cfg=dict(type='ReLU', inplace=True), norm_cfg=dict(type='BatchNorm2d'),
                       init_with_weight_file=None, norm_eval=False).train()


def _neck(kind, kw, bb):
    return getattr(N, kind)(num_input_channels_list=list(bb.num_output_channels_list),
                            num_input_strides_list=list(bb.num_output_strides_list), **kw).train()


@pytest.mark.parametrize('case', SC.NECK_CASES, ids=[c[0] for c in SC.NECK_CASES])
def test_every_neck_case_is_admitted(case):
    """all five: plain / GroupNorm + ReLU / BatchNorm laterals, top-down and neighbouring, 'conv' and 'pooling' extras"""
    _, kind, kw = case
    bb = _backbone()
    neck = _neck(kind, kw, bb)
    assert te.pyramid_supported(bb, neck)
    plan = te.build_pyramid(bb, neck)
    assert len(plan.out_ids) == kw['num_outputs'] and len(set(plan.out_ids)) == kw['num_outputs']
    want = {id(p) for p in list(bb.parameters()) + list(neck.parameters())}
    assert {id(p) for p in plan.params} == want and len(plan.params) == len(want)


def test_sibling_models_route():
    """the two pyramid siblings take the node, the SimpleNeck ones keep their routes; network_supported is unchanged"""
    got = {}
    for name in configs.SIBLINGS:
        m = configs.build_sibling_model(name).train()
        got[name] = te.pyramid_supported(m._backbone, m._neck)
        if name != 'LFDV2_SIMPLE' and type(m).__name__ != 'FCOS':
            assert not te.network_supported(m), name
    assert got == dict(FCOS_FPN=True, LFDV2_SFPN=True, LFDV2_SIMPLE=False, LFDV2_HEADV1=False)
    assert te.network_supported(configs.build_sibling_model('LFDV2_SIMPLE').train())
    m = configs.build_sibling_model('LFDV2_SFPN').train()
    assert te.supported(m._backbone)


def test_refusals():
    bb = _backbone()
    kw = dict(SC.NECK_CASES[4][2])                                        # SimpleFPN with BatchNorm laterals
    neck = _neck('SimpleFPN', kw, bb)
    assert te.pyramid_supported(bb, neck)
    neck.lateral1[1].eval()                                               # an eval-mode lateral BatchNorm
    assert not te.pyramid_supported(bb, neck)
    neck.lateral1[1].train()
    assert te.pyramid_supported(bb, neck)
    neck.lateral0[0].weight.requires_grad_(False)                         # a frozen neck parameter
    assert not te.pyramid_supported(bb, neck)
    neck.lateral0[0].weight.requires_grad_(True)
    neck.eval()                                                           # the whole neck in eval mode
    assert not te.pyramid_supported(bb, neck)
    kw96 = dict(SC.NECK_CASES[0][2], num_output_channels=96)              # a width the conv kernels are not instantiated for
    assert not te.pyramid_supported(bb, _neck('FPN', kw96, bb))
    gn = dict(SC.NECK_CASES[1][2], norm_cfg=dict(type='GroupNorm', num_groups=4))     # groups of 16 channels
    assert not te.pyramid_supported(bb, _neck('FPN', gn, bb))
    bb.eval()                                                             # an unsupported backbone
    assert not te.pyramid_supported(bb, _neck('FPN', dict(SC.NECK_CASES[0][2]), bb))
    for name, kind, kw_ in SC.NECK_CASES:                                 # none of these is the all-HIP network
        class _M(object):
            pass
        m = _M()
        bb2 = _backbone()
        m._backbone, m._neck, m._head = bb2, _neck(kind, kw_, bb2), nn.Identity()
        assert not te.network_supported(m), name


def test_gn_lateral_without_relu_is_admitted():
    """the GroupNorm backward takes its ReLU mask from an optional stored output: it has a form without a ReLU"""
    bb = _backbone()
    kw = dict(SC.NECK_CASES[1][2], relu_on_lateral=False)
    neck = _neck('FPN', kw, bb)
    assert te.pyramid_supported(bb, neck)
    plan = te.build_pyramid(bb, neck)
    lat = [plan.units[a[0]] for kind, *a in plan.steps if kind == 'unit']
    assert len(lat) == 3 and not any(u.relu for u in lat)


def _describe(plan):
    """the steps as (kind, sources, result) over activation indices"""
    out = []
    for kind, *a in plan.steps:
        if kind == 'unit':
            u = plan.units[a[0]]
            out.append(('unit', (u.src,), u.dst))
        elif kind == 'conv':
            out.append(('conv', (a[0].src,), a[0].dst))
        elif kind == 'merge':
            out.append(('merge', (a[0], a[1]), a[2]))
        else:
            out.append((kind, (a[0],), a[1]))
    return out


def test_step_order_and_gradient_fan_in_of_a_five_output_fpn():
    """FCOS_FPN's neck (3 inputs, 5 outputs, 'conv' extras behind the in-place ReLU, fed from the previous output): laterals,
    top-down merges from the coarsest level, the three smoothing convs, then ReLU -> conv twice.  Fan-in: a merged level feeds its
    smoothing conv and the merge below it; the ReLU'd output feeds the head and the next extra level."""
    m = configs.build_sibling_model('FCOS_FPN').train()
    plan = te.build_pyramid(m._backbone, m._neck)
    steps = _describe(plan)
    t0, t1, t2 = plan.tap_ids
    assert [s[0] for s in steps] == ['conv'] * 3 + ['merge'] * 2 + ['conv'] * 3 + ['relu', 'conv', 'relu', 'conv']
    l0, l1, l2 = (s[2] for s in steps[:3])
    assert [s[1] for s in steps[:3]] == [(t0,), (t1,), (t2,)]
    assert steps[3][1] == (l1, l2) and steps[4][1] == (l0, steps[3][2])           # level 1 first, its MERGED map into level 0
    m1, m0 = steps[3][2], steps[4][2]
    assert [s[1] for s in steps[5:8]] == [(m0,), (m1,), (l2,)]
    o0, o1, o2 = (s[2] for s in steps[5:8])
    assert steps[8] == ('relu', (o2,), steps[8][2]) and steps[9][1] == (steps[8][2],)
    assert steps[10][1] == (steps[9][2],) and steps[11][1] == (steps[10][2],)
    # the head gets the ReLU'd versions of outputs 2 and 3 (the in-place ReLU rewrites the previous output level)
    assert plan.out_ids == [o0, o1, steps[8][2], steps[10][2], steps[11][2]]
    # every result is produced before it is read (the backward walks the list in reverse)
    seen = set(plan.tap_ids)
    for _, srcs, dst in steps:
        assert all(s in seen for s in srcs) and dst not in seen
        seen.add(dst)
    fan = {}
    for _, srcs, _dst in steps:
        for s in srcs:
            fan[s] = fan.get(s, 0) + 1
    for o in plan.out_ids:
        fan[o] = fan.get(o, 0) + 1
    assert fan[m1] == 2 and fan[m0] == 1 and fan[l2] == 2 and fan[l1] == 1 and fan[l0] == 1
    assert fan[steps[8][2]] == 2 and fan[steps[10][2]] == 2 and fan[plan.out_ids[-1]] == 1
    assert fan[o2] == 1 and fan[t0] == fan[t1] == fan[t2] == 1


def test_neighbouring_mode_merges_the_unmerged_neighbour():
    """SimpleFPN neighbouring_mode: lateral[i] += upsample(lateral[i + 1]) walking up from the finest level, so level 1 goes
    into level 0 BEFORE it is merged itself"""
    bb = _backbone()
    name, kind, kw = SC.NECK_CASES[3]
    plan = te.build_pyramid(bb, _neck(kind, kw, bb))
    steps = _describe(plan)
    l0, l1, l2 = (s[2] for s in steps[:3])
    assert steps[3][:2] == ('merge', (l0, l1)) and steps[4][:2] == ('merge', (l1, l2))
    assert plan.out_ids[:2] == [steps[3][2], steps[4][2]]
    assert steps[5][:2] == ('relu', (l2,)) and plan.out_ids[2] == steps[5][2]


def test_extra_level_on_a_backbone_tap_needs_no_relu_step():
    """extra_on_input + relu_before_extra: the tap left the backbone's ReLU, the in-place ReLU changes neither it nor its gradient"""
    bb = _backbone()
    name, kind, kw = SC.NECK_CASES[0]
    plan = te.build_pyramid(bb, _neck(kind, kw, bb))
    steps = _describe(plan)
    pools = [s for s in steps if s[0] == 'pool']
    relus = [s for s in steps if s[0] == 'relu']
    assert pools[0][1] == (plan.tap_ids[-1],) and len(relus) == 1 and relus[0][1] == (pools[0][2],)
    assert pools[1][1] == (relus[0][2],) and plan.out_ids[3:] == [relus[0][2], pools[1][2]]


def test_the_routing_switch_is_read_at_call_time(monkeypatch):
    monkeypatch.delenv('LFD_HIP_NECK', raising=False)
    assert te.switches().hip_neck is True
    monkeypatch.setenv('LFD_HIP_NECK', '0')
    sw = te.switches()
    assert sw.hip_neck is False and all(v is True for v in sw)           # the schedules' switches do not move
