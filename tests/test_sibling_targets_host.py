"""CPU suite, sibling target assignment: the host mirrors (FCOS / FCOSv1 / LFDv2 .annotation_to_target) reproduce
ref_sibling_targets.npz -- the edge cases of tests/golden/sibling_target_cases.py as the REAL reference assigns them
(make_golden_sibling_targets.py) -- so the fixture the device kernels are compared with is pinned here as well; the per-point
rule the kernels implement (one pass over the boxes, ties to the lowest box index; csrc/assign_sibling.hip), restated in
numpy, equals the reference's sort / scatter / first-max on every committed fixture; and the new descriptors' ctypes
mirrors have the header's layout."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, load_golden
from lfd_amd import _lib, configs
from lfd_amd.model import FCOS, FCOSv1, LFDv2, losses as L
import sibling_cases as SC
import sibling_target_cases as TC

F = np.float32


def _host_targets(model, ann):
    for i, hw in enumerate(TC.SIZES):
        model._head_indexes_to_feature_map_sizes[i] = hw
    pts = model.generate_point_coordinates(model._head_indexes_to_feature_map_sizes)
    a, b = model.annotation_to_target(pts, [torch.from_numpy(x) for x, _ in ann], [torch.from_numpy(l) for _, l in ann])
    return a.numpy(), b.numpy()


def v2_model(mode, loss):
    return LFDv2(num_classes=TC.NUM_CLASSES, regression_ranges=TC.V2_RANGES, gray_range_factors=TC.GRAY_FACTORS,
                 range_assign_mode=mode, point_strides=TC.STRIDES, classification_loss_func=L.FocalLoss(),
                 regression_loss_func=getattr(L, loss)(), distance_to_bbox_mode='exp')


def test_fixture_holds_the_edge_cases_it_is_meant_to():
    g = load_golden('ref_sibling_targets.npz')
    ann = TC.annotations()
    assert [len(l) for _, l in ann] == [0, 8, 70]
    P = TC.total_points()
    pts = TC.points()
    fl, fr = g['fcos_labels'], g['fcos_reg']
    assert fl.shape == (3, P) and (fl[0] == TC.NUM_CLASSES).all() and not fr[0].any()       # image without boxes
    at = {(int(x), int(y)): i for i, (x, y) in enumerate(pts[:192])}                         # level 0
    # the right edge of box 0 lies on x = 48: FCOS's strict test leaves (48, 16) to the background
    assert fl[1, at[(48, 16)]] == TC.NUM_CLASSES
    # (104, 72) lies on the top edge of box 7 (class 1) and in its core zone: LFDv2's `>= 0` hit test scores it 1
    assert g['v2_0_cls'][1, at[(104, 72)], 1] == 1.0 and fl[1, at[(104, 72)]] == TC.NUM_CLASSES
    # equal areas: the lower box index (class 0) wins
    assert fl[1, at[(56, 56)]] == 0
    # largest distance == 32: valid on level 0 (upper bound) and on level 1 (lower bound), same coordinates
    p1 = 192 + (16 // 16) * 8 + 64 // 16
    assert tuple(pts[p1]) == (64, 16) and fl[1, at[(64, 16)]] == 2 and fl[1, p1] == 2
    assert fr[1, p1].max() == 32.0
    # nested boxes of two classes: FCOSv1 marks both, FCOS the inner one
    p = at[(40, 32)]
    assert fl[2, p] == 0 and g['fcosv1_labels'][1, p, 0] == 0 and g['fcosv1_labels'][1, p, 2] == 0
    # two core zones at (48, 48): score 1, regression target of the lower index (box 4: distances 4, 4, 4, 4)
    p = at[(48, 48)]
    assert g['v2_0_cls'][1, p, 2] == 1.0 and g['v2_0_reg'][1, p].tolist() == [4.0, 4.0, 4.0, 4.0]
    # relaxation: every LFDv2 case has scores strictly between 0 and 1
    for i in range(len(TC.V2_CASES)):
        c = g['v2_%d_cls' % i]
        assert ((c > 0) & (c < 1)).any() and c.max() == 1.0


def test_host_mirrors_reproduce_the_reference_edge_case_targets(ieee_sqrt):
    g = load_golden('ref_sibling_targets.npz')
    ann = TC.annotations()
    lab, reg = _host_targets(FCOS(num_classes=TC.NUM_CLASSES, regress_ranges=TC.FCOS_RANGES, point_strides=TC.STRIDES), ann)
    np.testing.assert_array_equal(lab, g['fcos_labels'])
    np.testing.assert_array_equal(reg, g['fcos_reg'])
    lab, reg = _host_targets(FCOSv1(num_classes=TC.NUM_CLASSES, regress_ranges=TC.FCOS_RANGES, point_strides=TC.STRIDES), ann)
    np.testing.assert_array_equal(lab[1:], g['fcosv1_labels'])
    np.testing.assert_array_equal(reg[1:], g['fcosv1_reg'])
    assert (lab[0] == 1).all() and not reg[0].any()
    for i, (mode, loss) in enumerate(TC.V2_CASES):
        ct, rt = _host_targets(v2_model(mode, loss), ann)
        np.testing.assert_array_equal(ct, g['v2_%d_cls' % i], err_msg=mode)
        np.testing.assert_array_equal(rt[:2], g['v2_%d_reg' % i][:2], err_msg=mode)
        # 70 boxes: rows whose best score is shared follow torch's unstable sort (see v2_rule), on any host's torch
        ok = v2_rule(TC.points(), _levels(TC.SIZES), TC.STRIDES, TC.V2_RANGES, [(3, 35), (28, 70), (57, 140)], ann[2][0],
                     ann[2][1], TC.NUM_CLASSES, mode, loss == 'SmoothL1Loss')[2]
        np.testing.assert_array_equal(rt[2][ok], g['v2_%d_reg' % i][2][ok], err_msg=mode)


# ---------------------------------------------------------------------------------------------- the kernels' per-point rule
def _dists(pts, b):
    px, py = pts[:, 0].astype(F), pts[:, 1].astype(F)
    return np.stack([px - b[0], py - b[1], (b[0] + b[2] - F(1)) - px, (b[1] + b[3] - F(1)) - py], -1)


def fcos_rule(pts, lvl, ranges, boxes, labels, C, multi_label):
    """csrc/assign_sibling.hip k_assign_fcos in numpy: one pass over the boxes, strict `<` keeps the first minimum"""
    P = len(pts)
    lo = np.array([ranges[l][0] for l in lvl], F)
    hi = np.array([ranges[l][1] for l in lvl], F)
    best_a = np.zeros(P, F)
    best_lab = np.full(P, C, np.int64)
    reg = np.zeros((P, 4), F)
    multi = np.ones((P, C), np.int64)
    for g, (b, c) in enumerate(zip(boxes.astype(F), labels)):
        d = _dists(pts, b)
        ok = (d.min(-1) > 0) & (d.max(-1) >= lo) & (d.max(-1) <= hi)
        area = np.where(ok, b[2] * b[3], F(1e8)).astype(F)
        multi[ok, c] = 0
        take = (area < best_a) if g else np.ones(P, bool)
        best_a = np.where(take, area, best_a)
        best_lab = np.where(take, np.where(area != F(1e8), c, C), best_lab)
        reg[take] = d[take]
    return (multi if multi_label else best_lab), reg


def v2_rule(pts, lvl, strides, rr, gr, boxes, labels, C, mode, independent):
    """k_assign_v2 in numpy (fp32, the reference's expression order); IEEE sqrt through fp64.
    -> (cls [P,C], reg [P,4], decided [P]: the largest score of the row is attained by ONE box, or G <= 16).
    The reference takes the first maximum of `score.sort(dim=1)`; torch's default CPU sort is stable for rows of up to 16
    elements only, so on longer rows WHICH of several equal scores (in practice: which box of an all-zero row) it selects
    is an artefact of that sort, not of the reference's algebra.  The kernel's rule is the stable one (lowest index)."""
    P = len(pts)
    px, py = pts[:, 0].astype(F), pts[:, 1].astype(F)
    half = np.array([strides[l] for l in lvl], F) / F(2)
    rlo, rhi = (np.array([rr[l][k] for l in lvl], F) for k in (0, 1))
    glo, ghi = (np.array([gr[l][k] for l in lvl], F) for k in (0, 1))
    lden, rden = np.maximum(rlo - glo, F(0.01)), np.maximum(ghi - rhi, F(0.01))
    cls = np.zeros((P, C), F)
    reg = np.zeros((P, 4), F)
    best = np.zeros(P, F)
    ntie = np.zeros(P, np.int64)
    sq = lambda v: np.sqrt(v.astype(np.float64)).astype(F)
    for g, (b, c) in enumerate(zip(boxes.astype(F), labels)):
        d = _dists(pts, b)
        hit = d.min(-1) >= 0
        lr = np.maximum(np.minimum(d[:, 0], d[:, 2]), F(0)) / np.maximum(np.maximum(d[:, 0], d[:, 2]), F(0.01))
        tb = np.maximum(np.minimum(d[:, 1], d[:, 3]), F(0)) / np.maximum(np.maximum(d[:, 1], d[:, 3]), F(0.01))
        score = np.where(hit, sq(lr * tb), F(0))
        cx, cy = b[0] + b[2] / F(2), b[1] + b[3] / F(2)
        core = (px >= cx - half) & (px <= cx + half) & (py >= cy - half) & (py <= cy + half) & hit
        score = np.where(core, F(1), score)
        measure = {'longer': np.full(P, max(b[2], b[3]), F), 'shorter': np.full(P, min(b[2], b[3]), F),
                   'sqrt': np.full(P, sq(np.array(b[2] * b[3], F)), F), 'dist': d.max(-1)}[mode]
        if independent:
            d = d / rhi[:, None]
        left = (measure - glo) / lden
        right = (ghi - measure) / rden
        relax = left * ((glo <= measure) & (measure < rlo)).astype(F) + ((rlo <= measure) & (measure <= rhi)).astype(F) \
            + right * ((rhi < measure) & (measure <= ghi)).astype(F)
        score = (score * relax).astype(F)
        cls[:, c] = np.where(score > 0, np.maximum(cls[:, c], score), cls[:, c])
        take = (score > best) if g else np.ones(P, bool)
        ntie = np.where(take, 1, ntie + (score == best))
        best = np.where(take, score, best)
        reg[take] = d[take]
    return cls, reg, (ntie <= 1) | (len(boxes) <= 16)


def _levels(sizes):
    return np.concatenate([np.full(h * w, i) for i, (h, w) in enumerate(sizes)])


def _points(sizes, strides):
    out = []
    for (h, w), s in zip(sizes, strides):
        ys, xs = np.meshgrid(np.arange(h) * s, np.arange(w) * s, indexing='ij')
        out.append(np.stack([xs.reshape(-1), ys.reshape(-1)], -1))
    return np.concatenate(out)


def test_per_point_rule_equals_the_reference_on_the_edge_cases():
    g = load_golden('ref_sibling_targets.npz')
    pts, lvl = TC.points(), _levels(TC.SIZES)
    gray = [(int(lo * 0.9), int(hi * 1.1)) for lo, hi in TC.V2_RANGES]
    for n, (b, l) in enumerate(TC.annotations()):
        lab, reg = fcos_rule(pts, lvl, TC.FCOS_RANGES, b, l, TC.NUM_CLASSES, False)
        np.testing.assert_array_equal(lab, g['fcos_labels'][n])
        np.testing.assert_array_equal(reg, g['fcos_reg'][n])
        if n:
            lab, reg = fcos_rule(pts, lvl, TC.FCOS_RANGES, b, l, TC.NUM_CLASSES, True)
            np.testing.assert_array_equal(lab, g['fcosv1_labels'][n - 1])
            np.testing.assert_array_equal(reg, g['fcosv1_reg'][n - 1])
        for i, (mode, loss) in enumerate(TC.V2_CASES):
            ct, rt, ok = v2_rule(pts, lvl, TC.STRIDES, TC.V2_RANGES, gray, b, l, TC.NUM_CLASSES, mode, loss == 'SmoothL1Loss')
            np.testing.assert_array_equal(ct, g['v2_%d_cls' % i][n], err_msg='%s image %d' % (mode, n))
            np.testing.assert_array_equal(rt[ok], g['v2_%d_reg' % i][n][ok], err_msg='%s image %d' % (mode, n))
            # nearly every positive row of the 70-box image has ONE best box (the rest: several core zones, score 1)
            assert (n == 2 or ok.all()) and (n == 0 or ok[ct.max(-1) > 0].mean() > 0.9)


@pytest.mark.parametrize('name', sorted(k for k, v in configs.SIBLINGS.items() if v['meta'] == 'LFDv2'))
def test_per_point_rule_equals_the_reference_on_the_model_fixtures(name):
    """the tie rule of the regression target (largest score, lowest index; box 0 on an all-zero row) against the reg_target
    arrays of the ref_sibling_LFDV2_* fixtures, which are mostly all-zero rows"""
    g = load_golden('ref_sibling_%s.npz' % name)
    spec = configs.SIBLINGS[name]
    n, H, W = [int(v) for v in g['shape']]
    sizes = [tuple(s) for s in g['sizes'].tolist()]
    model = configs.build_sibling_model(name, seed=1)
    C_ = spec['head']['num_classes']
    ann = SC.synth_annotations(5, n, H, W, C_)
    pts, lvl = _points(sizes, model._point_strides), _levels(sizes)
    assert (g['cls_target'].max(-1) == 0).mean() > 0.5
    for i, (b, l) in enumerate(ann):
        ct, rt, ok = v2_rule(pts, lvl, model._point_strides, model._regression_ranges, model._gray_ranges, b, l, C_,
                             spec['range_assign_mode'], model._regression_loss_type == 'independent')
        assert ok.all()
        np.testing.assert_array_equal(ct, g['cls_target'][i])
        np.testing.assert_array_equal(rt, g['reg_target'][i])


def test_new_descriptor_mirrors_match_the_header_layout(tmp_path):
    pairs = {'lfd_assign_fcos_desc_t': _lib.AssignFcosDesc, 'lfd_fcos_loss_desc_t': _lib.FcosLossDesc}
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


def test_device_routing_rules_without_a_device():
    """what get_loss routes to the fused kernels is decided from the loss modules; CPU predictions never are"""
    m = configs.build_sibling_model('FCOS_FPN')
    cpu = torch.zeros(1, 4, 3)
    assert m.device_targets and not m._fused_loss_supported(cpu)
    assert FCOSv1._multi_label and not FCOS._multi_label
    for name, want in (('LFDV2_SIMPLE', True), ('LFDV2_HEADV1', True), ('LFDV2_SFPN', False)):
        v2 = configs.build_sibling_model(name)
        cf, rf = v2._classification_loss_func, v2._regression_loss_func
        covered = type(cf).__name__ in ('FocalLoss', 'CrossEntropyLoss') and type(rf).__name__ == 'IoULoss'
        assert covered == want and not v2._fused_loss_supported(cpu)
