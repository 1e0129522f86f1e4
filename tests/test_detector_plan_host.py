"""Host side of what the two builders of the detector training node share (train_engine.build_detector for an FCOSHead,
build_lfd_detector for an LFDHead; one _DetectorPlan, one DetectorTrainFunction): the plan class, the widths of the node's outputs
by kind, the output convs' kernel size, the glue adapter, and the ORDER of the parameters -- it decides what Function.apply
receives.  The orders below were recorded from the builders as they stood when each head had a plan class and a node of its own
-- without a GPU."""
from lfd_amd import configs, train_engine as te
from lfd_head_cases import NODE_CASES

# FCOS_FPN and LFDV2_SFPN have the same backbone: stem pair, then per block (downsample pair,) conv1 / norm1, conv2 / norm2
BACKBONE = """
_backbone._stem.0.weight _backbone._stem.1.weight _backbone._stem.1.bias
_backbone._stem.3.weight _backbone._stem.4.weight _backbone._stem.4.bias
_backbone.stage0.0._downsample.0.weight _backbone.stage0.0._downsample.1.weight _backbone.stage0.0._downsample.1.bias
_backbone.stage0.0._conv1.weight _backbone.stage0.0._norm1.weight _backbone.stage0.0._norm1.bias
_backbone.stage0.0._conv2.weight _backbone.stage0.0._norm2.weight _backbone.stage0.0._norm2.bias
_backbone.stage0.1._conv1.weight _backbone.stage0.1._norm1.weight _backbone.stage0.1._norm1.bias
_backbone.stage0.1._conv2.weight _backbone.stage0.1._norm2.weight _backbone.stage0.1._norm2.bias
_backbone.stage1.0._downsample.0.weight _backbone.stage1.0._downsample.1.weight _backbone.stage1.0._downsample.1.bias
_backbone.stage1.0._conv1.weight _backbone.stage1.0._norm1.weight _backbone.stage1.0._norm1.bias
_backbone.stage1.0._conv2.weight _backbone.stage1.0._norm2.weight _backbone.stage1.0._norm2.bias
_backbone.stage2.0._downsample.0.weight _backbone.stage2.0._downsample.1.weight _backbone.stage2.0._downsample.1.bias
_backbone.stage2.0._conv1.weight _backbone.stage2.0._norm1.weight _backbone.stage2.0._norm1.bias
_backbone.stage2.0._conv2.weight _backbone.stage2.0._norm2.weight _backbone.stage2.0._norm2.bias
""".split()

# the FPN's conv + bias steps, the two towers' units, (cls, ctr) then reg output convs of level 0 with its Scale, the other Scales
FCOS_FPN = BACKBONE + """
_neck.lateral0.0.weight _neck.lateral0.0.bias _neck.lateral1.0.weight _neck.lateral1.0.bias
_neck.lateral2.0.weight _neck.lateral2.0.bias
_neck.fpn_out0.0.weight _neck.fpn_out0.0.bias _neck.fpn_out1.0.weight _neck.fpn_out1.0.bias
_neck.fpn_out2.0.weight _neck.fpn_out2.0.bias _neck.fpn_out3.1.weight _neck.fpn_out3.1.bias
_neck.fpn_out4.1.weight _neck.fpn_out4.1.bias
_head._classification_path.0.weight _head._classification_path.1.weight _head._classification_path.1.bias
_head._classification_path.3.weight _head._classification_path.4.weight _head._classification_path.4.bias
_head._regression_path.0.weight _head._regression_path.1.weight _head._regression_path.1.bias
_head._regression_path.3.weight _head._regression_path.4.weight _head._regression_path.4.bias
_head._classification.weight _head._classification.bias _head._centerness.weight _head._centerness.bias
_head._regression.weight _head._regression.bias
_head._scales.0._scale _head._scales.1._scale _head._scales.2._scale _head._scales.3._scale _head._scales.4._scale
""".split()

SFPN_NECK = """
_neck.lateral0.0.weight _neck.lateral0.1.weight _neck.lateral0.1.bias
_neck.lateral1.0.weight _neck.lateral1.1.weight _neck.lateral1.1.bias
_neck.lateral2.0.weight _neck.lateral2.1.weight _neck.lateral2.1.bias
""".split()

# separate towers: the classification conv, the level's Scale, then the regression conv (two records per level)
LFDV2_SFPN = BACKBONE + SFPN_NECK + """
_head.head0_classification_path.0.weight _head.head0_classification_path.1.weight _head.head0_classification_path.1.bias
_head.head0_classification_path.3.weight _head.head0_classification_path.4.weight _head.head0_classification_path.4.bias
_head.head0_regression_path.0.weight _head.head0_regression_path.1.weight _head.head0_regression_path.1.bias
_head.head0_regression_path.3.weight _head.head0_regression_path.4.weight _head.head0_regression_path.4.bias
_head.head0_classification_path.6.weight _head.head0_classification_path.6.bias _head._scales.0._scale
_head.head0_regression_path.6.weight _head.head0_regression_path.6.bias
_head._scales.1._scale _head._scales.2._scale _head._scales.3._scale
""".split()

# its twin with a merged 1x1 path: one record per level with both convs
MERGED_1X1 = BACKBONE + SFPN_NECK + """
_head.head0_merge_path.0.weight _head.head0_merge_path.1.weight _head.head0_merge_path.1.bias
_head.head0_merge_path.3.weight _head.head0_merge_path.4.weight _head.head0_merge_path.4.bias
_head.head0_classification_path.0.weight _head.head0_classification_path.0.bias
_head.head0_regression_path.0.weight _head.head0_regression_path.0.bias
_head._scales.0._scale _head._scales.1._scale _head._scales.2._scale _head._scales.3._scale
""".split()


def _plan(spec, build):
    m = configs.build_sibling_model(spec).train()
    return m, build(m._backbone, m._neck, m._head)


def _param_names(m, plan):
    name_of = {id(p): n for n, p in m.named_parameters()}
    return [name_of[id(p)] for p in plan.params]


def test_both_builders_return_the_one_plan_class():
    m, fcos = _plan('FCOS_FPN', te.build_detector)
    assert type(fcos) is te._DetectorPlan and fcos.head is m._head
    assert list(fcos.widths.items()) == [('cls', m._head._num_classes), ('reg', 4), ('ctr', 1)]       # the order the node returns
    assert fcos.ks == 3 and fcos.rows == te.FCOS_OUT_ROWS and fcos.glue is te._FCOSGlue and fcos.glue.reads == ('reg',)
    m, lfd = _plan(configs.SIBLINGS['LFDV2_SFPN'], te.build_lfd_detector)
    assert type(lfd) is te._DetectorPlan and lfd.head is m._head
    assert list(lfd.widths.items()) == [('cls', m._head.num_cls_channels), ('reg', 4)]
    assert lfd.ks == 1 and lfd.rows == 64 and lfd.glue is te._LFDGlue and lfd.glue.reads == ()
    m, ce = _plan(NODE_CASES['fpn128-ce'], te.build_lfd_detector)                                    # C + 1 class channels
    assert ce.widths == dict(cls=m._head._num_classes + 1, reg=4)
    assert te.lfd_detector_train_forward is te.detector_train_forward                                 # one entry point


def test_parameter_order_is_the_one_the_separate_builders_produced():
    for spec, build, want in (('FCOS_FPN', te.build_detector, FCOS_FPN),
                              (configs.SIBLINGS['LFDV2_SFPN'], te.build_lfd_detector, LFDV2_SFPN),
                              (NODE_CASES['merged1x1'], te.build_lfd_detector, MERGED_1X1)):
        m, plan = _plan(spec, build)
        assert _param_names(m, plan) == want
        assert len(want) == len(list(m.parameters()))                                                 # every parameter exactly once
