"""Host side of the LFDHead detector training node (train_engine.lfd_head_supported / build_lfd_detector): which LFD heads
behind an FPN / SimpleFPN it admits, what it refuses, the plan, and the layout of the glue's descriptor structs -- without a GPU."""
import ctypes as C
import os
import subprocess

import torch.nn as nn

from conftest import ROOT
from lfd_amd import _lib, configs, train_engine as te
from lfd_head_cases import NODE_CASES, V1_SPEC, variant

def _build(spec):
    return configs.build_sibling_model(spec).train()


def _ok(m):
    return te.lfd_head_supported(m._backbone, m._neck, m._head)


def test_admits_lfdv2_sfpn_and_the_variants():
    for name, spec in NODE_CASES.items():
        m = _build(spec)
        assert te.pyramid_supported(m._backbone, m._neck) and _ok(m), name
        assert not te.network_supported(m), name
    m = _build(NODE_CASES['wide-merged3x3'])
    assert (m._head._num_input_channels, m._head._num_head_channels, m._head._conv_kernel_size, m._head._merge_path_flag) == (64, 128, 3, True)
    m = _build(NODE_CASES['fpn128-ce'])
    assert m._head.num_cls_channels == m._head._num_classes + 1 and m._head._num_input_channels == 128 and m._neck._num_outputs == 5
    assert not hasattr(_build(NODE_CASES['no-scale'])._head, '_scales')
    # the padded conv's rows: merged, classes + 4 regression rows up to 128; separate towers, classes up to 128
    assert _ok(_build(variant(dict(conv_kernel_size=1, merge_path_flag=True, num_classes=124))))
    assert not _ok(_build(variant(dict(conv_kernel_size=1, merge_path_flag=True, num_classes=125))))
    assert _ok(_build(variant(dict(num_classes=128)))) and not _ok(_build(variant(dict(num_classes=129))))
    assert not _ok(_build(variant(dict(num_conv_layers=0, num_classes=125))))            # no tower layers: one conv too


def test_refusals():
    v1 = _build(V1_SPEC)
    assert type(v1._head).__name__ == 'LFDHeadV1' and te.pyramid_supported(v1._backbone, v1._neck) and not _ok(v1)
    assert not _ok(_build(variant(dict(norm_cfg=dict(type='BatchNorm2d')))))             # BatchNorm towers
    assert not _ok(_build(variant(dict(norm_cfg=None))))
    assert not _ok(_build(variant(dict(norm_cfg=dict(type='GroupNorm', num_groups=16)))))    # 64 channels in 16 groups
    m = _build(configs.SIBLINGS['LFDV2_SFPN'])
    p = m._head.head0_regression_path[-1].bias
    p.requires_grad_(False)                                                              # one frozen head parameter
    assert not _ok(m)
    p.requires_grad_(True)
    assert _ok(m)
    m._head.eval()
    assert not _ok(m)
    m._head.train()
    m._neck.eval()                                                                       # the pyramid node refuses
    assert not _ok(m)
    simple = _build(configs.SIBLINGS['LFDV2_SIMPLE'])                                    # a SimpleNeck: the whole-network node's
    assert te.network_supported(simple) and not _ok(simple)
    fcos = _build(configs.SIBLINGS['FCOS_FPN'])
    assert not _ok(fcos) and te.fcos_head_supported(fcos._backbone, fcos._neck, fcos._head)


def test_plan_of_lfdv2_sfpn_and_of_its_merged_twin():
    m = _build(configs.SIBLINGS['LFDV2_SFPN'])
    head = m._head
    plan = te.build_lfd_detector(m._backbone, m._neck, head)
    L, nlev = head._num_conv_layers, m._neck._num_outputs
    assert nlev == 4 and plan.pyramid is m._neck.__dict__['_lfd_pyramid_plan'] and plan.rows == 64 and plan.widths['cls'] == 4
    assert len(plan.units) == nlev * 2 * L and len({id(u.conv) for u in plan.units}) == 2 * L       # shared: packed once
    assert all(isinstance(u.norm, nn.GroupNorm) and u.relu and u.res is None and not u.first and not u.frozen for u in plan.units)
    assert all(u.conv.kernel_size == (3, 3) for u in plan.units)
    for i in range(nlev):
        lv = plan.units[i * 2 * L:(i + 1) * 2 * L]
        assert all(u.level == i for u in lv) and lv[0].src == lv[L].src == plan.pyramid.out_ids[i]
        assert all(u.dst >= plan.pyramid.n_act for u in lv)
        o_cls, o_reg = plan.outs[2 * i], plan.outs[2 * i + 1]
        assert o_cls.src == lv[L - 1].dst and o_reg.src == lv[-1].dst and o_cls.scale is o_reg.scale is head._scales[i]
        assert te.out_row_ranges(o_cls) == [(head.head0_classification_path[-1], 0, 4)]
        assert te.out_row_ranges(o_reg) == [(head.head0_regression_path[-1], 0, 4)]
    assert len({u.dst for u in plan.units}) == len(plan.units)
    want = {id(p) for p in m.parameters()}
    assert {id(p) for p in plan.params} == want and len(plan.params) == len(want)

    m = _build(NODE_CASES['merged1x1'])
    plan = te.build_lfd_detector(m._backbone, m._neck, m._head)
    assert len(plan.units) == nlev * L and len(plan.outs) == nlev
    o = plan.outs[1]
    assert te.out_row_ranges(o) == [(m._head.head0_classification_path[-1], 0, 4), (m._head.head0_regression_path[-1], 4, 8)]
    m = _build(NODE_CASES['no-layers'])
    plan = te.build_lfd_detector(m._backbone, m._neck, m._head)
    assert plan.units == [] and [o.src for o in plan.outs] == list(plan.pyramid.out_ids)
    m = _build(NODE_CASES['unshared'])
    plan = te.build_lfd_detector(m._backbone, m._neck, m._head)
    assert len({id(u.conv) for u in plan.units}) == len(plan.units) == nlev * 2 * L
    assert {id(p) for p in plan.params} == {id(p) for p in m.parameters()}
    m = _build(variant(dict(num_classes=100)))                                           # separate towers, 100 classes: both convs 128 rows
    assert te.build_lfd_detector(m._backbone, m._neck, m._head).rows == 128


def test_glue_struct_mirrors_match_the_header_layout(tmp_path):
    """sizeof and the offset of every field of the lfd_lfdhead_out_* structs as gcc sees them == the ctypes mirrors"""
    pairs = {'lfd_lfdhead_out_seg_t': _lib.LfdHeadOutSeg, 'lfd_lfdhead_out_conv_t': _lib.LfdHeadOutConv,
             'lfd_lfdhead_out_level_t': _lib.LfdHeadOutLevel}
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


def test_workspace_query_and_host_refusals():
    """pure host functions: the workspace query, and every refusal answers before anything touches a device"""
    l = _lib.lib()
    assert l.lfd_lfdhead_out_grad_workspace_bytes(1, 64) == 1024 * 2 * 2 * 64 * 4
    assert l.lfd_lfdhead_out_grad_workspace_bytes(8, 128) == 8 * 1024 * 2 * 2 * 128 * 4 <= l.lfd_train_workspace_bytes()
    assert l.lfd_lfdhead_out_grad_workspace_bytes(1, 32) == 0 and l.lfd_lfdhead_out_grad_workspace_bytes(9, 64) == 0
    assert l.lfd_lfdhead_out_pack_levels_f32(None, 1, 1, 64, 4, 16, None, None, None) == -1
    assert l.lfd_lfdhead_out_grad_levels_f32(None, 1, 1, 64, 4, 16, None, None, 1.0, None, 0, None) == -1
