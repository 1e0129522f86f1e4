"""Host side of the 'fp32_storage' mode of FCOS / LFDv2 / LFD over FPN-family necks (lfd_amd/engine_sibling_p32.py): the plan
builds on CPU tensors, its launch list is what the design says (one merge launch per merged lateral, two with LFD_P32_MERGE=0;
one exp launch per FCOS level), wide backbones are refused by name, and the `precision` setters validate and invalidate."""
import collections

import pytest
import torch

from lfd_amd import configs, engine, engine_p32, engine_sibling_p32 as E
from lfd_amd.model import LFD

CPU = torch.device('cpu')
P = 'lfd_p32_'


def _lfd_over_sfpn():
    v2 = configs.build_sibling_model('LFDV2_SFPN', seed=1).eval()
    spec = configs.SIBLINGS['LFDV2_SFPN']
    return LFD(backbone=v2._backbone, neck=v2._neck, head=v2._head, num_classes=spec['head']['num_classes'],
               regression_ranges=spec['regression_ranges'], range_assign_mode='dist', point_strides=v2._point_strides,
               classification_loss_func=v2._classification_loss_func, regression_loss_func=v2._regression_loss_func,
               distance_to_bbox_mode=spec['distance_to_bbox_mode']).eval()


def _model(name):
    return _lfd_over_sfpn() if name == 'LFD_SFPN' else configs.build_sibling_model(name, seed=1).eval()


def _counts(plan):
    return collections.Counter(plan.launch_names())


@pytest.mark.parametrize('name', sorted(configs.SIBLINGS) + ['LFD_SFPN'])
def test_plan_builds_on_cpu_tensors_with_the_designed_launch_list(name):
    m = _model(name)
    neck, head = m._neck, m._head
    fused, two = E.SiblingPrecisePlan(m, CPU, merge=True), E.SiblingPrecisePlan(m, CPU, merge=False)
    cf, ct = _counts(fused), _counts(two)
    pyramid = type(neck).__name__ != 'SimpleNeck'
    merged = neck._num_inputs - 1 if pyramid else 0
    assert cf[P + 'conv2d_merge_nhwc_f32'] == merged and cf[P + 'upsample_nearest_add_f32'] == 0
    assert ct[P + 'conv2d_merge_nhwc_f32'] == 0 and ct[P + 'upsample_nearest_add_f32'] == merged
    assert len(two.ops) == len(fused.ops) + merged                       # one launch per merged lateral instead of two
    assert ct[P + 'conv2d_nhwc_f32'] == cf[P + 'conv2d_nhwc_f32'] + merged
    levels = head._num_heads
    assert cf[P + 'exp_rows_f32'] == (levels if type(head).__name__ == 'FCOSHead' else 0)
    # the laterals are walked from the coarsest level down: each merge reads an already-merged (or the coarsest) map
    merges = [o for o in fused.ops if o.kind == 'merge']
    written = set()
    for o in fused.ops:
        if o.kind == 'merge':
            assert o.res in written and (o.ks, o.stride) == (1, 1)
        if getattr(o, 'dst', None) is not None:
            written.add(o.dst)
    assert [fused.buf_scale[o.dst] for o in merges] == sorted((fused.buf_scale[o.dst] for o in merges), reverse=True)
    # every output conv writes a level of cls / reg (/ ctr); the head levels' sizes come from the neck's outputs
    outs = collections.Counter(o.out for o in fused.ops if o.kind == 'conv' and o.out is not None)
    assert outs['cls'] == outs['reg'] == levels and outs['ctr'] == (levels if fused.has_ctr else 0)
    assert len(fused.level_bufs()) == levels
    scales = [fused.buf_scale[b] for b in fused.level_bufs()]
    assert scales == [scales[0] << i for i in range(levels)]                # each level halves the one before it


@pytest.mark.parametrize('name,distinct', [('FCOS_FPN', 4 + 3), ('LFDV2_SFPN', 4 + 2)])
def test_modules_shared_between_levels_are_packed_once(name, distinct):
    """FCOSHead's towers and output convs (and an LFDHead with share_head_flag) are the same modules on every level: one
    packed weight / bias pair per module in the plan, whatever the number of levels (Scale stays per level)"""
    plan = E.SiblingPrecisePlan(_model(name), CPU, merge=True)
    nl = len(plan.level_bufs())
    convs = [o for o in plan.ops if o.kind in ('conv', 'merge')]         # backbone and neck convs are all different modules
    assert len({id(o.w) for o in convs}) == len(convs) - (nl - 1) * distinct
    assert len({id(o.b) for o in convs}) == len(convs) - (nl - 1) * distinct
    gns = [o for o in plan.ops if o.kind == 'gn']                        # only the head has GroupNorm in these two models
    assert len({id(o.gamma) for o in gns}) * nl == len(gns)
    scales = [o.scale for o in convs if o.scale is not None]
    assert len(scales) == nl and len({id(s) for s in scales}) == nl


def test_extra_levels_and_neighbouring_mode():
    """the in-place ReLU in front of an extra level is its own launch on the buffer the level READS; neighbouring_mode (bottom-up,
    each level reads its unmerged neighbour) takes the two-launch route whatever the switch says"""
    from lfd_amd.model import neck as N
    m = _model('LFDV2_SFPN')
    plan = E.SiblingPrecisePlan(m, CPU, merge=True)
    relu = [o for o in plan.ops if o.kind == 'relu']
    pool = [o for o in plan.ops if o.kind == 'pool']
    assert len(relu) == 1 and len(pool) == 1 and relu[0].src == pool[0].src == plan.level_bufs()[2]
    assert pool[0].dst == plan.level_bufs()[3]
    bb = m._backbone
    m._neck = N.SimpleFPN(num_input_channels_list=list(bb.num_output_channels_list),
                          num_input_strides_list=list(bb.num_output_strides_list), num_output_channels=64, num_outputs=4,
                          extra_type='conv', norm_on_lateral=True, relu_on_lateral=True, norm_cfg=dict(type='BatchNorm2d'),
                          neighbouring_mode=True).eval()
    plan = E.SiblingPrecisePlan(m, CPU, merge=True)
    c = _counts(plan)
    assert c[P + 'conv2d_merge_nhwc_f32'] == 0 and c[P + 'upsample_nearest_add_f32'] == 2
    adds = [o for o in plan.ops if o.kind == 'upadd']
    assert plan.buf_scale[adds[0].dst] < plan.buf_scale[adds[1].dst]           # finest first


def test_wide_backbone_is_refused_with_require_narrows_message():
    m = configs.build_model(configs.PRESETS['faster_faster_faster'])
    with pytest.raises(engine.Unsupported, match="'fp16' mode"):
        E.SiblingPrecisePlan(m, CPU)


# engine_p32.PrecisePlan(WIDERFACE_LFD_S) as recorded BEFORE its backbone part became a method shared with the sibling plan:
# one line per launch -- source buffer > destination (buffer id, or output tensor + level), channels, kernel, stride, ReLU,
# residual buffer, chained 1x1 (tail), frame gather (patch), Scale
_LFD_S_LAUNCHES = """
conv binput>0 3>64 k3s2 r1 tail patch|conv b0>1 64>64 k3s2 r1 tail|conv b1>2 64>64 k1s2 r0|conv b1>3 64>64 k3s2 r1
conv b3>4 64>64 k3s1 r1 +b2|conv b4>5 64>64 k3s1 r1|conv b5>6 64>64 k3s1 r1 +b4|conv b6>7 64>64 k3s1 r1
conv b7>8 64>64 k3s1 r1 +b6|conv b8>9 64>64 k3s1 r1|conv b9>10 64>64 k3s1 r1 +b8|conv b10>11 64>64 k1s2 r0
conv b10>12 64>64 k3s2 r1|conv b12>13 64>64 k3s1 r1 +b11|conv b13>14 64>64 k3s1 r1|conv b14>15 64>64 k3s1 r1 +b13
conv b15>16 64>64 k1s2 r0|conv b15>17 64>64 k3s2 r1|conv b17>18 64>64 k3s1 r1 +b16|conv b18>19 64>64 k3s1 r1
conv b19>20 64>64 k3s1 r1 +b18|conv b20>21 64>128 k1s2 r0|conv b20>22 64>128 k3s2 r1|conv b22>23 128>128 k3s1 r1 +b21
conv b23>24 128>128 k3s1 r1|conv b24>25 128>128 k3s1 r1 +b23|conv b25>26 128>128 k3s1 r1|conv b26>27 128>128 k3s1 r1 +b25
conv b10>28 64>128 k1s1 r1|conv b28>29 128>128 k1s1 r0|gn b29 g16|conv b29>30 128>128 k1s1 r0|gn b30 g16
conv b30>cls0 128>1 k1s1 r0|conv b30>reg0 128>4 k1s1 r0 scale
conv b15>31 64>128 k1s1 r1|conv b31>32 128>128 k1s1 r0|gn b32 g16|conv b32>33 128>128 k1s1 r0|gn b33 g16
conv b33>cls1 128>1 k1s1 r0|conv b33>reg1 128>4 k1s1 r0 scale
conv b20>34 64>128 k1s1 r1|conv b34>35 128>128 k1s1 r0|gn b35 g16|conv b35>36 128>128 k1s1 r0|gn b36 g16
conv b36>cls2 128>1 k1s1 r0|conv b36>reg2 128>4 k1s1 r0 scale
conv b23>37 128>128 k1s1 r1|conv b37>38 128>128 k1s1 r0|gn b38 g16|conv b38>39 128>128 k1s1 r0|gn b39 g16
conv b39>cls3 128>1 k1s1 r0|conv b39>reg3 128>4 k1s1 r0 scale
conv b27>40 128>128 k1s1 r1|conv b40>41 128>128 k1s1 r0|gn b41 g16|conv b41>42 128>128 k1s1 r0|gn b42 g16
conv b42>cls4 128>1 k1s1 r0|conv b42>reg4 128>4 k1s1 r0 scale
"""


def _launch_lines(plan):
    out = []
    for o in plan.ops:
        if o.kind == 'gn':
            out.append('gn b%d g%d' % (o.src, o.groups))
            continue
        dst = o.dst if o.out is None else '%s%d' % (o.out, o.level)
        out.append('conv b%s>%s %d>%d k%ds%d r%d%s%s%s%s' % (
            o.src, dst, o.cin, o.cout, o.ks, o.stride, o.relu, ' +b%d' % o.res if o.res is not None else '',
            ' tail' if o.tail is not None else '', ' patch' if o.patch else '', ' scale' if o.scale is not None else ''))
    return out


def test_lfd_plan_launches_equal_the_list_recorded_before_the_backbone_builder_was_shared():
    plan = engine_p32.PrecisePlan(configs.build_model('WIDERFACE_LFD_S').eval(), CPU)
    want = [l for line in _LFD_S_LAUNCHES.strip().splitlines() for l in line.split('|')]
    assert len(want) == 63 and _launch_lines(plan) == want
    assert all(o.relu == 1 for o in plan.ops if o.kind == 'gn')          # the head's GroupNorm launches keep their ReLU


@pytest.mark.parametrize('name', ['FCOS_FPN', 'LFDV2_SFPN', 'LFD_SFPN'])
def test_precision_setter_validates_and_drops_cached_plans(name):
    m = _model(name)
    assert type(m).PRECISIONS == ('fp16', 'fp32_storage') and m.precision == 'fp16'
    with pytest.raises(ValueError):
        m.precision = 'fp32'
    assert m.precision == 'fp16'
    m.__dict__['_lfd_sibling_cache'] = {'k': object()}
    m.precision = 'fp16'                                   # no change: caches stay
    assert '_lfd_sibling_cache' in m.__dict__
    m.precision = 'fp32_storage'
    assert m.precision == 'fp32_storage' and '_lfd_sibling_cache' not in m.__dict__
    plan = E.get_plan(m, CPU)
    assert E.get_plan(m, CPU) is plan and '_lfd_sibling_p32_cache' in m.__dict__
    m.precision = 'fp16'
    assert '_lfd_sibling_p32_cache' not in m.__dict__
    assert E.covers(m)


def test_merge_switch_is_read_when_a_plan_is_built(monkeypatch):
    m = _model('FCOS_FPN')
    monkeypatch.setenv('LFD_P32_MERGE', '0')
    two = E.get_plan(m, CPU)
    monkeypatch.setenv('LFD_P32_MERGE', '1')
    fused = E.get_plan(m, CPU)
    assert not two.merge and fused.merge and two is not fused and E.get_plan(m, CPU) is fused
    assert not E.covers(_model('LFDV2_SIMPLE'))            # SimpleNeck + LFDHead keeps engine_p32's route
