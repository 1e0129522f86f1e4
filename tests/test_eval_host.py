"""Evaluation, host side (no GPU): the numpy oracle of the definition (tests/golden/coco_eval_oracle.py, DESIGN.md
"Evaluation") pinned to answers derivable by hand, one case per rule; and the parts of lfd_amd/evaluation.py that run on the
host -- the JSON reader, the label -> category map, the summary, the display string, the empty case, argument errors, the
ctypes mirrors of the new structs."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import coco_eval_oracle as oracle
from conftest import ROOT
from lfd_amd import _lib, evaluation


def gt(image_id, bbox, category_id=1, iscrowd=0, area=None):
    return dict(image_id=image_id, category_id=category_id, bbox=list(bbox), iscrowd=iscrowd,
                area=bbox[2] * bbox[3] if area is None else area)


def dt(image_id, bbox, score, category_id=1):
    return dict(image_id=image_id, category_id=category_id, bbox=list(bbox), score=score)


ONE = 1.0 / (1.0 + np.spacing(1))     # one hit, no miss: tp / (fp + tp + spacing(1)) is the float64 just below 1
A_BOX, B_BOX, NOWHERE = [10, 10, 50, 50], [200, 10, 50, 50], [400, 400, 50, 50]    # 2500 px: "medium"


def base_case():
    gts = [gt(1, A_BOX), gt(1, B_BOX)]
    dts = [dt(1, A_BOX, 0.9), dt(1, NOWHERE, 0.8), dt(1, B_BOX, 0.7)]
    return gts, dts


def test_three_detections_two_boxes_is_253_over_303():
    gts, dts = base_case()
    r = oracle.evaluate(gts, dts, [1], [1])
    want = 253.0 / 303.0
    p = r['precision']
    assert p.shape == (10, 101, 1, 4, 3) and r['recall'].shape == (10, 1, 4, 3)
    for a in (0, 2):
        for m in range(3):
            for t in range(10):
                col = p[t, :, 0, a, m]
                assert (col[:51] == ONE).all() and (col[51:] == 2.0 / 3.0).all()
                assert r['recall'][t, 0, a, m] == 1.0
    assert (p[:, :, :, 1, :] == -1).all() and (p[:, :, :, 3, :] == -1).all()
    s = r['stats']
    for i in (0, 1, 2, 4):
        assert abs(s[i] - want) < 1e-15, (i, s[i])
    assert s[3] == -1 and s[5] == -1 and s[8] == 1.0 and s[6] == 1.0 and s[10] == 1.0 and s[9] == -1 and s[11] == -1
    m = r['matches'][(1, 1)]
    assert m['index'] == [0, 1, 2]
    assert m['matched'][:, 0, :].tolist() == [[True, False, True]] * 10
    assert not m['ignored'][:, 0, :].any() and not m['ignored'][:, 2, :].any()
    assert m['ignored'][:, 1, :].all() and m['ignored'][:, 3, :].all()      # everything is "medium"


def test_image_without_detections_counts_only_when_it_is_evaluated():
    gts, dts = base_case()
    gts.append(gt(2, [5, 5, 60, 60]))
    quirk = oracle.evaluate(gts, dts, [1], [1])                 # the reference records only images that produced a detection
    assert abs(quirk['stats'][0] - 253.0 / 303.0) < 1e-15 and quirk['stats'][8] == 1.0
    full = oracle.evaluate(gts, dts, [1, 2], [1])
    col = full['precision'][0, :, 0, 0, 2]
    assert (col[:34] == ONE).all() and (col[34:67] == 2.0 / 3.0).all() and (col[67:] == 0.0).all()
    assert abs(full['stats'][0] - 56.0 / 101.0) < 1e-15 and abs(full['stats'][1] - 56.0 / 101.0) < 1e-15
    assert abs(full['stats'][8] - 2.0 / 3.0) < 1e-15


def test_a_crowd_box_takes_any_number_of_detections_and_none_is_a_false_positive():
    gts = [gt(1, [0, 0, 200, 200], iscrowd=1), gt(1, [300, 300, 50, 50])]
    dts = [dt(1, [10, 10, 40, 40], 0.9), dt(1, [100, 100, 40, 40], 0.8), dt(1, [300, 300, 50, 50], 0.7)]
    r = oracle.evaluate(gts, dts, [1], [1])
    m = r['matches'][(1, 1)]
    assert m['matched'][:, 0, :].all()                      # IoU with a crowd = intersection / detection area = 1
    assert m['ignored'][:, 0, :].tolist() == [[True, True, False]] * 10
    assert abs(r['stats'][0] - 1.0) < 1e-15 and r['stats'][8] == 1.0
    assert m['npig'].tolist() == [1, 0, 1, 0]


def test_a_non_ignored_match_wins_over_a_better_overlapping_ignored_one():
    # G1: IoU 0.6 with the detection, area "medium".  G2: the detection's own box (IoU 1) but an annotated area of 100 ("small")
    gts = [gt(1, [0, 0, 50, 30]), gt(1, [0, 0, 50, 50], area=100)]
    dts = [dt(1, [0, 0, 50, 50], 0.9)]
    assert oracle.iou([0, 0, 50, 50], [0, 0, 50, 30], False) == 0.6
    m = oracle.evaluate(gts, dts, [1], [1])['matches'][(1, 1)]
    # medium: G1 is not ignored, G2 is.  Up to 0.60 the walk stops at G1; above, G1 fails and the ignored G2 takes it
    assert m['matched'][:, 2, 0].all()
    assert m['ignored'][:, 2, 0].tolist() == [False] * 3 + [True] * 7
    # small: G2 is the non-ignored one and matches at every threshold; all: both count, the better overlap wins
    assert m['matched'][:, 1, 0].all() and not m['ignored'][:, 1, 0].any()
    assert m['matched'][:, 0, 0].all() and not m['ignored'][:, 0, 0].any()


def test_equal_scores_keep_insertion_order():
    gts = [gt(1, A_BOX)]
    miss_first = oracle.evaluate(gts, [dt(1, NOWHERE, 0.5), dt(1, A_BOX, 0.5)], [1], [1])
    hit_first = oracle.evaluate(gts, [dt(1, A_BOX, 0.5), dt(1, NOWHERE, 0.5)], [1], [1])
    assert miss_first['matches'][(1, 1)]['index'] == [0, 1] and hit_first['matches'][(1, 1)]['index'] == [0, 1]
    assert miss_first['stats'][0] == 0.5 and abs(hit_first['stats'][0] - 1.0) < 1e-15


def test_an_area_of_exactly_1024_is_small_and_medium():
    box = [0, 0, 32, 32]
    s = oracle.evaluate([gt(1, box)], [dt(1, box, 0.9)], [1], [1])['stats']
    assert abs(s[3] - 1.0) < 1e-15 and abs(s[4] - 1.0) < 1e-15 and s[5] == -1 and abs(s[0] - 1.0) < 1e-15


def test_more_than_100_detections_in_an_image():
    gts = [gt(1, A_BOX)]
    dts = [dt(1, [500 + 60 * i, 500, 50, 50], 0.99 - 0.001 * i) for i in range(120)] + [dt(1, A_BOX, 0.5)]
    dts += [dt(1, [500 + 60 * i, 900, 50, 50], 0.4 - 0.001 * i) for i in range(29)]
    s = oracle.evaluate(gts, dts, [1], [1])['stats']
    assert s[0] == 0.0                       # at 100 detections the hit is cut away
    assert abs(s[1] - 1.0 / 121.0) < 1e-15   # at 1000 it is the 121st
    assert s[6] == 0.0 and s[7] == 1.0 and s[8] == 1.0


def test_more_than_1000_detections_are_cut_before_matching():
    gts = [gt(1, A_BOX)]
    dts = [dt(1, [500, 500, 50, 50], 0.9)] * 1000 + [dt(1, A_BOX, 0.5)]
    r = oracle.evaluate(gts, dts, [1], [1])
    assert len(r['matches'][(1, 1)]['index']) == 1000 and r['stats'][8] == 0.0


def test_an_iou_equal_to_the_threshold_matches():
    gts = [gt(1, [0, 0, 50, 25], area=2000)]
    dts = [dt(1, [0, 0, 50, 50], 0.9)]
    assert oracle.iou([0, 0, 50, 50], [0, 0, 50, 25], False) == 0.5 == oracle.IOU_THRS[0]
    m = oracle.evaluate(gts, dts, [1], [1])['matches'][(1, 1)]
    assert m['matched'][:, 0, 0].tolist() == [True] + [False] * 9


def test_iou_has_no_plus_one_and_crowd_union_is_the_detection():
    assert oracle.iou([0, 0, 10, 10], [10, 0, 10, 10], False) == 0.0         # touching: width 0
    assert oracle.iou([0, 0, 10, 10], [5, 0, 10, 10], False) == 50.0 / 150.0
    assert oracle.iou([0, 0, 10, 10], [5, 0, 100, 100], True) == 0.5


# ---------------------------------------------------------------------------------------------------- lfd_amd/evaluation.py
def coco_dict():
    gts, _ = base_case()
    gts.append(gt(7, [5, 5, 60, 60], category_id=3, iscrowd=1))
    for i, g in enumerate(gts):
        g['id'] = i + 1
    del gts[1]['area']
    return dict(images=[dict(id=7), dict(id=1), dict(id=4)], categories=[dict(id=3), dict(id=1), dict(id=9)], annotations=gts)


def test_parameters_and_summary_agree_with_the_oracle():
    iou_thrs, rec_thrs, area_rng = evaluation.coco_params()
    assert iou_thrs.dtype == rec_thrs.dtype == area_rng.dtype == np.float64
    assert np.array_equal(iou_thrs, oracle.IOU_THRS) and np.array_equal(rec_thrs, oracle.REC_THRS)
    assert area_rng.tolist() == [[float(v) for v in r] for r in oracle.AREA_RNG]
    assert list(evaluation.MAX_DETS) == oracle.MAX_DETS
    gts, dts = base_case()
    r = oracle.evaluate(gts + [gt(2, [5, 5, 60, 60])], dts, [1, 2], [1])
    assert np.array_equal(evaluation.summarize(r['precision'], r['recall']), r['stats'])
    empty = evaluation.summarize(-np.ones((10, 101, 1, 4, 3)), -np.ones((10, 1, 4, 3)))
    assert (empty == -1).all() and empty.shape == (12,)


def test_json_reader_sorts_images_and_categories_and_groups_the_ground_truth(tmp_path):
    path = tmp_path / 'instances_val.json'
    path.write_text(json.dumps(coco_dict()))
    for ev in (evaluation.COCOEvaluator(str(path), {0: 1, 1: 3}), evaluation.COCOEvaluator(None, {0: 1, 1: 3}, annotations=coco_dict())):
        assert isinstance(ev, evaluation.Evaluator)
        assert ev.image_ids == [1, 4, 7] and ev.category_ids == [1, 3, 9]
        assert ev._label_map.tolist() == [0, 1]
        assert ev.gt_pair.tolist() == [0, 0, 2 * 3 + 1]
        assert ev.gt_box.dtype == np.float64 and ev.gt_box.tolist() == [A_BOX, B_BOX, [5, 5, 60, 60]]
        assert ev.gt_area.tolist() == [2500.0, 2500.0, 3600.0]          # the second has no 'area': w * h
        assert ev.gt_crowd.tolist() == [0, 0, 1]
        start = ev.gt_pair_start
        assert start.shape == (3 * 3 + 1,) and start[0] == 0 and start[1] == 2 and start[7] == 2 and start[8] == 3 and start[9] == 3


def test_ground_truth_values_stay_float64():
    v = 123.456789012345678            # not representable in fp32
    ev = evaluation.COCOEvaluator(None, {0: 1}, annotations=dict(annotations=[gt(1, [v, 0.1, 10.3, 20.7])]))
    assert ev.gt_box[0, 0] == v and float(np.float32(v)) != v


def test_display_string_and_the_empty_case():
    stats = np.array([0.123456, 0.5, 0.25, -1.0, 1.0, 0.0] + [0.0] * 6)
    assert evaluation.format_display(stats) == ('\nmAP       :0.12346\nmAP_50    :0.50000\nmAP_75    :0.25000\n'
                                                'mAP_s     :-1.00000\nmAP_m     :1.00000\nmAP_l     :0.00000\n')
    ev = evaluation.COCOEvaluator(None, {0: 1}, annotations=coco_dict())
    assert ev.get_eval_display_str() == ''
    ev.evaluate()
    assert ev.get_eval_display_str() == '\nNo bboxes detected! Evaluation abort!\n'
    assert ev.stats is None


def test_argument_errors(tmp_path):
    with pytest.raises(ValueError):
        evaluation.COCOEvaluator(None, {0: 1})
    with pytest.raises(ValueError):
        evaluation.COCOEvaluator('x.json', {0: 1}, annotations=coco_dict())
    with pytest.raises(FileNotFoundError):
        evaluation.COCOEvaluator(str(tmp_path / 'missing.json'), {0: 1})
    with pytest.raises(TypeError):
        evaluation.COCOEvaluator(None, [1], annotations=coco_dict())
    with pytest.raises(ValueError):
        evaluation.COCOEvaluator(None, {0: 2}, annotations=coco_dict())          # category 2 does not exist
    with pytest.raises(ValueError):
        evaluation.COCOEvaluator(None, {0: 1}, annotations=dict(images=[]))
    ev = evaluation.COCOEvaluator(None, {0: 1}, annotations=coco_dict())
    with pytest.raises(TypeError):
        ev.update([[], []])
    with pytest.raises(ValueError):
        ev.update(([[]], [dict(image_id=1), dict(image_id=4)]))
    with pytest.raises(ValueError):
        ev.update(([[]], [dict(image_id=12345)]))
    with pytest.raises(KeyError):
        ev.update(([[[5, 0.9, 1.0, 1.0, 2.0, 2.0]]], [dict(image_id=1)]))       # label 5 has no category, as the reference
    with pytest.raises(NotImplementedError):
        evaluation.Evaluator().update(None)


def test_entry_points_refuse_bad_arguments_with_status_codes():
    l = _lib.lib()
    assert l.lfd_eval_match_workspace_bytes(None) == 0
    d = _lib.EvalDesc()
    d.num_images, d.num_categories, d.num_gt, d.det_capacity = 4, 3, 5, 100
    d.num_iou_thrs, d.num_area_rngs, d.num_rec_thrs, d.num_max_dets = 10, 4, 101, 3
    d.max_dets[0], d.max_dets[1], d.max_dets[2] = 100, 300, 1000
    assert l.lfd_eval_match_workspace_bytes(C.byref(d)) >= (3 * 4 * 3 + 100) * 4 + 5 * 64
    assert l.lfd_eval_accumulate_workspace_bytes(C.byref(d)) >= 2 * 100 * 4 + 256 * 4
    b = _lib.EvalBufs()
    assert l.lfd_eval_match(C.byref(d), C.byref(b), None, 0, None) == -1
    assert l.lfd_eval_accumulate(C.byref(d), C.byref(b), None, 0, None) == -1
    assert l.lfd_eval_append_rows_f64(C.byref(d), C.byref(b), None, 1, None, 0, None) == -1
    assert l.lfd_eval_append_dets_f32(C.byref(d), C.byref(b), None, None, None, 1, 8, None, 1, None, 0, None) == -1
    d.num_iou_thrs = 17                                                          # 17 * 4 matchings do not fit a wave
    assert l.lfd_eval_match_workspace_bytes(C.byref(d)) == 0
    d.num_iou_thrs, d.max_dets[1] = 10, 50                                       # not ascending
    assert l.lfd_eval_match_workspace_bytes(C.byref(d)) == 0


def test_ctypes_mirrors_of_the_evaluation_structs_match_the_header(tmp_path):
    pairs = {'lfd_eval_desc_t': _lib.EvalDesc, 'lfd_eval_bufs_t': _lib.EvalBufs}
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
