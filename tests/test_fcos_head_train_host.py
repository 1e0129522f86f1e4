"""Host side of the detector training node (train_engine.fcos_head_supported / build_detector): which FCOS heads it admits,
what it refuses, and the plan -- tower units over shared modules, padded output convs with their row ranges, parameters --
without a GPU."""
import torch.nn as nn

from lfd_amd import configs, train_engine as te


def _variant(head=None, neck=None):
    """FCOS_FPN with head / neck keywords replaced"""
    spec = dict(configs.SIBLINGS['FCOS_FPN'])
    spec['head'] = dict(spec['head'], **(head or {}))
    spec['neck'] = dict(spec['neck'], **(neck or {}))
    return configs.build_sibling_model(spec).train()


def _narrow():
    return _variant(dict(num_head_channels=64, norm_cfg=dict(type='GroupNorm', num_groups=8)), dict(num_output_channels=64))


def _ok(m):
    return te.fcos_head_supported(m._backbone, m._neck, m._head)


def test_admits_fcos_fpn_and_its_64_channel_variant():
    assert _ok(configs.build_sibling_model('FCOS_FPN').train())
    m = _narrow()
    assert m._head._num_input_channels == 64 and m._head._num_head_channels == 64 and _ok(m)
    assert _ok(_variant(dict(num_classes=te.FCOS_OUT_ROWS - 1)))          # classes + centerness fill the padded conv exactly


def test_refusals():
    assert not _ok(_variant(dict(norm_cfg=None)))                                          # norm-free towers
    assert not _ok(_variant(dict(norm_cfg=dict(type='BatchNorm2d'))))                      # BatchNorm towers
    assert not _ok(_variant(dict(norm_cfg=dict(type='GroupNorm', num_groups=32))))         # groups of 4 channels
    assert not _ok(_variant(dict(num_layers=0)))
    assert not _ok(_variant(dict(num_classes=te.FCOS_OUT_ROWS)))                           # no row left for the centerness
    m = configs.build_sibling_model('FCOS_FPN').train()
    m._head._centerness.bias.requires_grad_(False)                                         # one frozen head parameter
    assert not _ok(m)
    m._head._centerness.bias.requires_grad_(True)
    assert _ok(m)
    m._head.eval()
    assert not _ok(m)
    m._head.train()
    m._neck.eval()                                                                         # the pyramid node refuses
    assert not _ok(m)
    v2 = configs.build_sibling_model('LFDV2_SFPN').train()                                 # an LFDHead behind a SimpleFPN
    assert te.pyramid_supported(v2._backbone, v2._neck) and not _ok(v2)


def test_the_head_switch_is_read_at_call_time(monkeypatch):
    monkeypatch.delenv('LFD_HIP_HEAD', raising=False)
    monkeypatch.delenv('LFD_HIP_NECK', raising=False)
    assert te.switches().hip_head is True
    monkeypatch.setenv('LFD_HIP_HEAD', '0')
    sw = te.switches()
    assert sw.hip_head is False and sw.hip_neck is True and all(v is True for v in sw)


def test_plan_of_fcos_fpn():
    m = configs.build_sibling_model('FCOS_FPN').train()
    head = m._head
    plan = te.build_detector(m._backbone, m._neck, head)
    L, C, nlev = head._num_layers, head._num_classes, m._neck._num_outputs
    assert nlev == 5 and plan.pyramid is m._neck.__dict__['_lfd_pyramid_plan'] and plan.rows == te.FCOS_OUT_ROWS
    # 5 levels x 2 towers x num_layers units over 2 x num_layers distinct conv (and norm) modules
    assert len(plan.units) == nlev * 2 * L
    assert len({id(u.conv) for u in plan.units}) == 2 * L == len({id(u.norm) for u in plan.units})
    assert all(isinstance(u.norm, nn.GroupNorm) and u.relu and u.res is None and not u.first and not u.frozen for u in plan.units)
    cls_convs = [mod for mod in head._classification_path if isinstance(mod, nn.Conv2d)]
    reg_convs = [mod for mod in head._regression_path if isinstance(mod, nn.Conv2d)]
    for i in range(nlev):
        lv = plan.units[i * 2 * L:(i + 1) * 2 * L]
        assert all(u.level == i for u in lv)
        assert [u.conv for u in lv] == cls_convs + reg_convs                 # FCOSHead.forward's order within a level
        assert lv[0].src == lv[L].src == plan.pyramid.out_ids[i]             # both towers read the level's neck output
        for a, b in zip(lv[:L - 1], lv[1:L]):
            assert b.src == a.dst
        for a, b in zip(lv[L:2 * L - 1], lv[L + 1:]):
            assert b.src == a.dst
        assert all(u.dst >= plan.pyramid.n_act for u in lv)                  # activation numbering goes on from the pyramid's
        o_cls, o_reg = plan.outs[2 * i], plan.outs[2 * i + 1]
        assert o_cls.level == o_reg.level == i and o_cls.src == lv[L - 1].dst and o_reg.src == lv[-1].dst
        assert te.out_row_ranges(o_cls) == [(head._classification, 0, C), (head._centerness, C, C + 1)]
        assert te.out_row_ranges(o_reg) == [(head._regression, 0, 4)]
        assert o_cls.scale is None and o_reg.scale is head._scales[i]
    assert len(plan.outs) == 2 * nlev
    assert len({u.dst for u in plan.units}) == len(plan.units)
    want = {id(p) for p in m.parameters()}
    assert {id(p) for p in plan.params} == want and len(plan.params) == len(want)
