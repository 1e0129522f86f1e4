"""Host side of the fused get_loss for every loss pair (csrc/getloss_ex.hip): the descriptor's ctypes mirror against the
header as gcc lays it out, the bindings, the host validation of the four entry points (status codes, no launch: this runs
without a GPU) and the admission table LFD / LFDv2 derive from their two loss modules."""
import ctypes as C
import itertools
import os
import re
import subprocess

import pytest

from conftest import ROOT
from lfd_amd import _lib, ops
from lfd_amd.model import losses as L
from lfd_amd.model.lfd import fused_loss_route

EXPORTS = ['lfd_get_loss_ex_workspace_bytes', 'lfd_get_loss_ex_sums_f32', 'lfd_get_loss_ex_finalize_f32',
           'lfd_get_loss_ex_bwd_f32']
OK, INVALID, WS_SMALL, UNSUPPORTED = 0, -1, -2, -4


def test_descriptor_mirror_matches_the_header_layout(tmp_path):
    mirror, cname = _lib.LossDescEx, 'lfd_loss_ex_desc_t'
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lfd_hip.h"', 'int main(void) {',
             'printf("size %%zu\\n", sizeof(%s));' % cname]
    for fname, _ in mirror._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(%s, %s));' % (fname, cname, fname))
    lines.append('return 0; }')
    src, exe = tmp_path / 'layout.c', tmp_path / 'layout'
    src.write_text('\n'.join(lines))
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True, capture_output=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got['size']) == C.sizeof(mirror)
    for fname, _ in mirror._fields_:
        assert int(got[fname]) == getattr(mirror, fname).offset, fname
    # the fields the issue names, and the geometry of lfd_loss_desc_t in the same order
    names = [f for f, _ in mirror._fields_]
    geometry = ['n', 'num_levels', 'level_h', 'level_w', 'stride', 'range_max', 'total_points', 'num_classes']
    assert names[:len(geometry)] == geometry == [f for f, _ in _lib.LossDesc._fields_][:len(geometry)]
    assert set(names[len(geometry):]) == {'cls_loss', 'reg_loss', 'decode_mode', 'gamma', 'alpha', 'qfl_beta', 'smooth_l1_beta',
                                          'box_eps', 'cls_loss_weight', 'reg_loss_weight', 'cls_weighted', 'reg_weighted'}


def test_exports_are_bound_additively_and_the_abi_version_stays():
    header = open(os.path.join(ROOT, 'include', 'lfd_hip.h')).read()
    lib = C.CDLL(_lib.LIB_PATH)
    for s in EXPORTS:
        assert re.search(r'LFD_API\s+[\w\s\*]+?\b%s\s*\(' % s, header), s
        assert hasattr(lib, s), s
        assert s in _lib.declared_symbols(), s
    assert _lib.lib().lfd_hip_abi_version() == _lib.ABI_VERSION == 3
    for s in ('lfd_get_loss_workspace_bytes', 'lfd_get_loss_sums_f32', 'lfd_get_loss_finalize_f32', 'lfd_get_loss_bwd_f32'):
        assert hasattr(lib, s), s                         # the existing trio is untouched
    assert C.sizeof(_lib.LossDesc) == 8 + 16 * _lib.MAX_LEVELS + 8 + 8 + 12 + 8 + 8


def _desc(**kw):
    args = dict(n=2, sizes=[(3, 5), (2, 2)], strides=[8, 16], reg_ranges=[(0, 64), (64, 128)], num_classes=3,
                cls_loss='QualityFocalLoss', reg_loss='GIoULoss', decode_mode='exp')
    args.update(kw)
    return ops.make_loss_desc_ex(**args)


def test_workspace_query_is_a_pure_host_function():
    l = _lib.lib()
    assert l.lfd_get_loss_ex_workspace_bytes() == 8 * 8 * 1024     # 8 doubles per block partial, at most 1024 blocks
    assert l.lfd_get_loss_ex_workspace_bytes() == l.lfd_get_loss_workspace_bytes()


def test_descriptor_builder_fills_kinds_and_total_points():
    d = _desc(qfl_beta=1.5, smooth_l1_beta=0.25, box_eps=1e-7, gamma=1.0, alpha=0.5, cls_loss_weight=2.0, reg_loss_weight=3.0,
              cls_weighted=True, reg_weighted=True)
    assert (d.n, d.num_levels, d.total_points, d.num_classes) == (2, 2, 19, 3)
    assert (d.cls_loss, d.reg_loss, d.decode_mode) == (2, 1, 1)
    assert (d.qfl_beta, d.smooth_l1_beta, d.gamma, d.alpha) == (1.5, 0.25, 1.0, 0.5)
    assert d.box_eps == pytest.approx(1e-7) and (d.cls_loss_weight, d.reg_loss_weight) == (2.0, 3.0)
    assert (d.cls_weighted, d.reg_weighted) == (1, 1) and list(d.range_max)[:2] == [64.0, 128.0]
    assert ops.CLS_LOSSES == {'FocalLoss': 0, 'CrossEntropyLoss': 1, 'QualityFocalLoss': 2, 'BCEWithLogitsLoss': 3}
    assert ops.REG_LOSSES == {'IoULoss': 0, 'GIoULoss': 1, 'DIoULoss': 2, 'CIoULoss': 3, 'SmoothL1Loss': 4, 'MSELoss': 5}
    assert _desc(cls_loss=3, reg_loss=5, decode_mode='sigmoid').decode_mode == 0


def _calls(l, d, p, ws_bytes=None):
    """the three launching entry points with the host pointer `p` in every pointer slot (never dereferenced on the host)"""
    ws = l.lfd_get_loss_ex_workspace_bytes() if ws_bytes is None else ws_bytes
    ref = C.byref(d) if d is not None else None
    return (l.lfd_get_loss_ex_sums_f32(ref, p, p, p, p, p, ws, p, None),
            l.lfd_get_loss_ex_finalize_f32(ref, p, p, 1.0, p, None),
            l.lfd_get_loss_ex_bwd_f32(ref, p, p, p, p, p, p, p, p, None))


def test_invalid_arguments_are_status_codes_without_a_launch():
    l = _lib.lib()
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    # null descriptor / null tensors
    assert _calls(l, None, p) == (INVALID, INVALID, INVALID)
    assert _calls(l, _desc(), None) == (INVALID, INVALID, INVALID)
    d = _desc()
    ws = l.lfd_get_loss_ex_workspace_bytes()
    assert l.lfd_get_loss_ex_sums_f32(C.byref(d), p, p, p, p, None, ws, p, None) == INVALID      # no workspace
    assert l.lfd_get_loss_ex_sums_f32(C.byref(d), p, p, p, p, p, ws, None, None) == INVALID      # no sums
    assert l.lfd_get_loss_ex_finalize_f32(C.byref(d), p, None, 1.0, p, None) == INVALID
    assert l.lfd_get_loss_ex_bwd_f32(C.byref(d), p, p, p, p, p, p, p, None, None) == INVALID     # no grad_reg
    # kinds out of range
    for field, bad in (('cls_loss', -1), ('cls_loss', 4), ('reg_loss', -1), ('reg_loss', 6), ('decode_mode', 2)):
        d = _desc()
        setattr(d, field, bad)
        assert _calls(l, d, p) == (INVALID, INVALID, INVALID), (field, bad)
    # total_points is not the sum of the levels
    d = _desc()
    d.total_points += 1
    assert _calls(l, d, p) == (INVALID, INVALID, INVALID)
    d = _desc(reg_loss='SmoothL1Loss', smooth_l1_beta=0.0)
    assert _calls(l, d, p) == (INVALID, INVALID, INVALID)
    # an independent regression loss cannot be row-weighted
    for reg in ('SmoothL1Loss', 'MSELoss'):
        assert _calls(l, _desc(reg_loss=reg, reg_weighted=True), p) == (UNSUPPORTED, UNSUPPORTED, UNSUPPORTED)
    # workspace too small
    d = _desc()
    assert l.lfd_get_loss_ex_sums_f32(C.byref(d), p, p, p, p, p, ws - 1, p, None) == WS_SMALL
    assert l.lfd_get_loss_ex_sums_f32(C.byref(d), p, p, p, p, p, 0, p, None) == WS_SMALL
    # an empty batch has nothing to launch in the backward
    assert l.lfd_get_loss_ex_bwd_f32(C.byref(_desc(n=0)), None, None, None, None, None, None, None, None, None) == OK


CLS = {'FocalLoss': lambda **k: L.FocalLoss(**k), 'CrossEntropyLoss': lambda **k: L.CrossEntropyLoss(**k),
       'QualityFocalLoss': lambda **k: L.QualityFocalLoss(**k), 'BCEWithLogitsLoss': lambda **k: L.BCEWithLogitsLoss(**k)}
REG = {'IoULoss': lambda **k: L.IoULoss(**k), 'GIoULoss': lambda **k: L.GIoULoss(**k), 'DIoULoss': lambda **k: L.DIoULoss(**k),
       'CIoULoss': lambda **k: L.CIoULoss(**k), 'SmoothL1Loss': lambda **k: L.SmoothL1Loss(**k),
       'MSELoss': lambda **k: L.MSELoss(**k)}


def test_admission_table_over_all_pairs_and_the_refusals():
    assert len(CLS) * len(REG) == 24
    for (cn, cf), (rn, rf) in itertools.product(CLS.items(), REG.items()):
        want = 'base' if cn in ('FocalLoss', 'CrossEntropyLoss') and rn == 'IoULoss' else 'ex'
        for cw in (False, True):
            assert fused_loss_route(cf(), rf(), cw, False) == want, (cn, rn, cw)
        independent = rn in ('SmoothL1Loss', 'MSELoss')
        assert fused_loss_route(cf(), rf(), False, True) == (None if independent else want), (cn, rn)
        # a reduction other than 'mean' on either module
        assert fused_loss_route(cf(reduction='sum'), rf(), False, False) is None, (cn, rn)
        assert fused_loss_route(cf(), rf(reduction='sum'), False, False) is None, (cn, rn)
    softmax_focal = L.FocalLoss()
    softmax_focal.use_sigmoid = False          # (the constructor refuses it; the admission reads the attribute)
    for rn, rf in REG.items():
        assert fused_loss_route(softmax_focal, rf(), False, False) is None, rn
    assert fused_loss_route(None, L.IoULoss()) is None and fused_loss_route(L.FocalLoss(), L.L1Loss()) is None


def test_switches_select_the_route_of_a_model(monkeypatch):
    """LFD_FUSED_LOSS=0: op by op for every pair; LFD_FUSED_LOSS_EX=0: the admission before the widening -- 'base' pairs only;
    =1: every admitted pair; unset: of the 'ex' pairs those on IoULoss (the TrafficLight family)"""
    from lfd_amd.model.lfd import LFD
    from lfd_amd.model.lfdv2 import LFDv2
    kw = dict(regression_ranges=((0, 64), (64, 128)), point_strides=(8, 16), num_classes=3)
    base = LFD(classification_loss_func=L.FocalLoss(), regression_loss_func=L.IoULoss(), **kw)
    ex = LFD(classification_loss_func=L.QualityFocalLoss(), regression_loss_func=L.IoULoss(), **kw)
    v2 = LFDv2(classification_loss_func=L.FocalLoss(), regression_loss_func=L.GIoULoss(), **kw)
    sl1 = LFD(classification_loss_func=L.BCEWithLogitsLoss(), regression_loss_func=L.SmoothL1Loss(), **kw)
    routes = lambda: tuple(m._fused_loss_route() for m in (base, ex, v2, sl1))      # noqa: E731
    monkeypatch.delenv('LFD_FUSED_LOSS', raising=False)
    monkeypatch.delenv('LFD_FUSED_LOSS_EX', raising=False)
    assert routes() == ('base', 'ex', None, None)
    monkeypatch.setenv('LFD_FUSED_LOSS_EX', '1')
    assert routes() == ('base', 'ex', 'ex', 'ex')
    monkeypatch.setenv('LFD_FUSED_LOSS_EX', '0')
    assert routes() == ('base', None, None, None)
    monkeypatch.setenv('LFD_FUSED_LOSS_EX', '1')
    monkeypatch.setenv('LFD_FUSED_LOSS', '0')
    assert routes() == (None, None, None, None)
    monkeypatch.delenv('LFD_FUSED_LOSS')
    for i, s in enumerate([(3, 5), (2, 2)]):
        ex._head_indexes_to_feature_map_sizes[i] = base._head_indexes_to_feature_map_sizes[i] = s
    assert isinstance(ex._loss_desc(2), _lib.LossDescEx) and ex._loss_desc(2).cls_loss == 2
    assert isinstance(base._loss_desc(2), _lib.LossDesc)
    v2.device_targets = False
    import torch
    assert not v2._fused_loss_supported(torch.zeros(1))         # a CPU prediction never takes the device route
