"""The TT100K protocol, host side (no GPU): the numpy restatement of DESIGN.md 9b (tests/golden/tt100k_eval_oracle.py) equals
every number the reference's own official_eval.eval_annos produced for tests/golden/ref_tt100k_eval.npz -- counts, outcome
codes, the float64 bits of accuracy / recall, the report strings; and the parts of lfd_amd/evaluation.py TT100KEvaluator that
run on the host: annotation parsing, the id-as-string lookup, argument errors, the display string, the results dictionary, the
new C-ABI symbols.  tt100k_fixture.py (tests/golden) turns the fixture into the evaluator's and the oracle's inputs."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import tt100k_eval_oracle as oracle
import tt100k_fixture as fx
from conftest import ROOT
from lfd_amd import _lib, evaluation


@pytest.fixture(scope='module')
def fix():
    return fx.load()


def test_the_oracle_equals_the_reference_on_every_fixture_group(fix):
    assert fix.num_groups >= 10 and len(fix.images) > 40
    cells = 0
    for g in range(fix.num_groups):
        p, want = fix.params(g), fix.expected(g)
        r = oracle.evaluate(fix.oracle_images(), p['ious'], p['minscores'], p['size_ranges'], fix.in_types(p['types']),
                            p['check_type'], p['match_same'], num_categories=len(fix.cat_names))
        for k in ('right', 'num_detections', 'num_ground_truth'):
            assert r[k].dtype == np.int64 and np.array_equal(r[k], want[k]), (g, k)
        for k in ('accuracy', 'recall'):
            assert r[k].tobytes() == want[k].tobytes(), (g, k)                    # the same float64 bits
        T, M, S = want['right'].shape
        for t in range(T):
            for m in range(M):
                for s in range(S):
                    det = np.concatenate([c[t][m][s] for c in r['det_code']])
                    gt = np.concatenate([c[t][m][s] for c in r['gt_code']])
                    assert np.array_equal(det, want['det_code'][t, m, s]), (g, t, m, s)
                    assert np.array_equal(gt == oracle.GT_MISSED, want['gt_missed'][t, m, s]), (g, t, m, s)
                    lo, hi = p['size_ranges'][s]
                    line = oracle.report(p['ious'][t], lo, hi, p['types'], p['check_type'], r['right'][t, m, s],
                                         r['num_detections'][t, m, s], r['num_ground_truth'][t, m, s])
                    assert line == str(want['report'][t, m, s]), (g, t, m, s)
                    cells += 1
    assert cells >= 40


def test_per_category_counts_are_the_reference_runs_with_one_type(fix):
    """types=[name, '<no such type>'] keeps one category: its totals are that category's slice of the all-types run"""
    base = fix.params(3)
    assert base['types'] is None and base['match_same'] and base['ious'] == [0.5] and base['minscores'][0] == 50
    r = oracle.evaluate(fix.oracle_images(), [0.5], [50], [[0, 400], [32, 96]], None, True, True, num_categories=len(fix.cat_names))
    seen = 0
    for g in range(fix.num_groups):
        p = fix.params(g)
        if p['types'] is None or len(p['types']) != 2:
            continue
        k = fix.cat_names.index(p['types'][0])
        want = fix.expected(g)
        got = r['per_category'][0, 0, :, k, :]
        assert np.array_equal(got[:, 0], want['right'][0, 0]) and np.array_equal(got[:, 1], want['num_detections'][0, 0])
        assert np.array_equal(got[:, 2], want['num_ground_truth'][0, 0])
        assert got[0].min() > 0
        seen += 1
    assert seen >= 4


def test_fixture_holds_the_cases_that_tell_a_wrong_matcher_apart(fix):
    n_gt = [len(im[1]) for im in fix.oracle_images()]
    n_dt = [len(im[3]) for im in fix.oracle_images()]
    assert max(n_gt) > 64 and max(n_dt) > 1024 and 0 in n_gt and 0 in n_dt
    box, score = oracle.detections_from_f32(fix.det)
    assert (score == 50.0).any() and (score == 75.0).any()
    assert ((box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1]) == 0).any()
    for v in (32.0, 96.0, 400.0):
        assert (oracle.long_side(fix.gt_box) == v).any() and (oracle.long_side(box) == v).any()
    # a score-ordered matcher (the COCO evaluator's order) gets a different answer on the "steal" image
    gb, gc, db, dc, sc = fix.oracle_images()[1]
    t = oracle.iou_matrix(gb, db)
    taken, by_score = set(), 0
    for j in np.argsort(-sc, kind='stable'):
        cand = [(t[i, j], i) for i in range(len(gc)) if i not in taken and t[i, j] > 0.5]
        if cand:
            taken.add(max(cand)[1])
            by_score += 1
    assert by_score == 1 and fix.expected(0)['det_code'][0, 0, 0][fix.det_img == 1].tolist() == [1, 1]


def test_type45_and_the_results_dictionary(fix):
    assert len(evaluation.TYPE45) == 45 == len(set(evaluation.TYPE45)) and evaluation.TYPE45 == fix.type45
    rows, meta = fix.rows(), fix.meta()
    got = evaluation.tt100k_results(rows[:2], meta[:2], fix.names)
    assert got == json.loads(fix.results_json)
    assert json.dumps(got) == fix.results_json                                   # key order and float repr too
    as_dict = evaluation.tt100k_results(rows[:2], meta[:2], dict(enumerate(fix.names)))
    assert as_dict == got
    with pytest.raises(KeyError):
        evaluation.tt100k_results([[[99, 0.5, 1.0, 1.0, 2.0, 2.0]]], meta[:1], fix.names)


def small_annotations():
    return {'imgs': {'7': {'objects': [{'bbox': {'xmin': 1, 'ymin': 2, 'xmax': 30.5, 'ymax': 40}, 'category': 'pn'},
                                       {'bbox': {'xmin': 5, 'ymin': 5, 'xmax': 9, 'ymax': 9}, 'category': 'not_a_label'}]},
                     '12': {'objects': []}, 'a3': {'objects': [{'bbox': {'xmin': 0, 'ymin': 0, 'xmax': 8, 'ymax': 8}, 'category': 'i2'}]}},
            'types': ['pn', 'i2']}


def test_annotations_are_parsed_in_annotation_order_and_ids_are_strings(tmp_path):
    ann = small_annotations()
    ev = evaluation.TT100KEvaluator(annotations=ann, label_indexes_to_category_names=['i2', 'pn'])
    assert ev.image_ids == ['7', '12', 'a3'] and ev.gt_start.tolist() == [0, 2, 2, 3]
    assert ev.gt_box.dtype == np.float64 and ev.gt_box.tolist() == [[1, 2, 30.5, 40], [5, 5, 9, 9], [0, 0, 8, 8]]
    assert [ev.category_names[c] for c in ev.gt_cat] == ['pn', 'not_a_label', 'i2']
    assert ev.category_names[:2] == ['i2', 'pn'] and set(evaluation.TYPE45) < set(ev.category_names)
    assert ev._label_map.tolist() == [0, 1]
    assert ev._in_types[ev._cat_idx['pn']] == 1 and ev._in_types[ev._cat_idx['not_a_label']] == 0
    assert ev._ordinals([dict(image_id=12), dict(image_id='a3')]) == [1, 2]          # looked up as str(...)
    path = tmp_path / 'annotations.json'
    path.write_text(json.dumps(ann))
    from_file = evaluation.TT100KEvaluator(annotation_path=str(path), label_indexes_to_category_names={0: 'i2', 1: 'pn'}, types=None)
    assert from_file.image_ids == ev.image_ids and np.array_equal(from_file.gt_box, ev.gt_box)
    assert from_file._in_types.tolist() == [1] * len(from_file.category_names) and from_file.types is None


def test_argument_errors():
    ann = small_annotations()
    names = ['i2', 'pn']
    with pytest.raises(ValueError):
        evaluation.TT100KEvaluator(label_indexes_to_category_names=names)
    with pytest.raises(ValueError):
        evaluation.TT100KEvaluator(annotation_path='x.json', annotations=ann, label_indexes_to_category_names=names)
    with pytest.raises(FileNotFoundError):
        evaluation.TT100KEvaluator(annotation_path='/nonexistent/annotations.json', label_indexes_to_category_names=names)
    with pytest.raises(ValueError):
        evaluation.TT100KEvaluator(annotations={'annotations': []}, label_indexes_to_category_names=names)
    with pytest.raises(TypeError):
        evaluation.TT100KEvaluator(annotations=ann, label_indexes_to_category_names=None)
    with pytest.raises(ValueError):
        evaluation.TT100KEvaluator(annotations=ann, label_indexes_to_category_names=names, size_ranges=())
    ev = evaluation.TT100KEvaluator(annotations=ann, label_indexes_to_category_names=names)
    with pytest.raises(TypeError):
        ev.update([[], []])
    with pytest.raises(ValueError, match='not in the annotations'):
        ev.update(([[]], [dict(image_id=8)]))
    with pytest.raises(ValueError, match='twice'):
        ev.update(([[], []], [dict(image_id=7), dict(image_id='7')]))
    with pytest.raises(ValueError, match='no category name'):
        ev.update(([[[5, 0.9, 1.0, 1.0, 5.0, 5.0]]], [dict(image_id=7)]))
    with pytest.raises(ValueError):
        ev.update(([[]], [dict(image_id=7), dict(image_id=12)]))
    with pytest.raises(RuntimeError):
        ev.match_table()


def test_scalar_or_sequence_arguments_and_the_display_string_of_an_empty_run():
    ann = small_annotations()
    ev = evaluation.TT100KEvaluator(annotations=ann, label_indexes_to_category_names=['i2', 'pn'])
    assert (ev.ious, ev.minscores, ev.size_ranges, ev.check_type, ev.match_same) == ([0.5], [90], [(0, 400)], True, True)
    assert ev.types == evaluation.TYPE45 and ev.types is not evaluation.TYPE45
    ev.evaluate()                                                   # nothing accumulated: no device is needed
    assert ev.right.shape == (1, 1, 1) and ev.right.dtype == np.int64 and ev.accuracy.dtype == np.float64
    assert ev.accuracy[0, 0, 0] == 1.0 and ev.recall[0, 0, 0] == 1.0 and ev.num_ground_truth_per_category.shape == (1, 1, 1, len(ev.category_names))
    assert ev.get_eval_display_str() == 'iou:0.5, size:[0,400), types:[i2, ...total 45...], accuracy:1, recall:1'
    sweep = evaluation.TT100KEvaluator(annotations=ann, label_indexes_to_category_names=['i2', 'pn'], types=None, iou=(0.5, 0.75),
                                       minscore=[10, 50, 90], size_ranges=((0, 32), (32, 96), (96.0, 400)), match_same=False)
    sweep.evaluate()
    assert sweep.right.shape == (2, 3, 3) and sweep.right_per_category is None
    lines = sweep.get_eval_display_str().split('\n')
    assert len(lines) == 18 and lines[0] == 'iou:0.5, size:[0,32), types:all, accuracy:1, recall:1'
    assert lines[-1] == 'iou:0.75, size:[96.0,400), types:all, accuracy:1, recall:1'
    one = evaluation.TT100KEvaluator(annotations=ann, label_indexes_to_category_names=['i2', 'pn'], types=['pn'])
    one.evaluate()
    assert one.report() == 'iou:0.5, size:[0,400), types:pn, accuracy:1, recall:1'        # the reference raises here
    none = evaluation.TT100KEvaluator(annotations=ann, label_indexes_to_category_names=['i2', 'pn'], check_type=False, match_same=False)
    none.evaluate()
    assert none.report() == 'iou:0.5, size:[0,400), types:none, accuracy:1, recall:1'


def test_without_a_gpu_update_raises():
    import torch
    ev = evaluation.TT100KEvaluator(annotations=small_annotations(), label_indexes_to_category_names=['i2', 'pn'])
    batch = ([[[0, 0.9, 1.0, 1.0, 5.0, 5.0]]], [dict(image_id=7)])
    if torch.cuda.is_available():
        ev.update(batch)                                            # where a GPU is visible the kernels run instead
        return
    with pytest.raises(RuntimeError, match='no CPU implementation'):
        ev.update(batch)


def test_new_symbols_are_exported_bound_and_refuse_null_arguments():
    new = ['lfd_eval_tt100k_append_dets_f32', 'lfd_eval_tt100k_append_rows_f64', 'lfd_eval_tt100k_match',
           'lfd_eval_tt100k_workspace_bytes']
    assert [s for s in _lib.declared_symbols() if s.startswith('lfd_eval_tt100k_')] == new
    header = open(os.path.join(ROOT, 'include', 'lfd_hip.h')).read()
    raw = C.CDLL(_lib.LIB_PATH)
    for s in new:
        assert s in header and hasattr(raw, s)
    l = _lib.lib()
    assert l.lfd_hip_abi_version() == 3
    assert l.lfd_eval_tt100k_append_dets_f32(None, None, None, None, None, 1, 1, None, 1, None, None) == -1
    assert l.lfd_eval_tt100k_append_rows_f64(None, None, None, 0, None, 0, None) == -1
    assert l.lfd_eval_tt100k_match(None, None, None, 0, None) == -1
    assert l.lfd_eval_tt100k_workspace_bytes(None) == 0
    desc = _lib.TT100KEvalDesc(4, 3, 5, 1024, 2, 3, 4, 1, 1)
    wb = l.lfd_eval_tt100k_workspace_bytes(C.byref(desc))
    assert wb >= 1024 * (4 + 4 * 8 + 8 + 4) + 2 * 4 * 4 and wb % 256 == 0
    bufs = _lib.TT100KEvalBufs()
    assert l.lfd_eval_tt100k_match(C.byref(desc), C.byref(bufs), None, 0, None) == -1          # no store, no workspace
    assert l.lfd_eval_tt100k_append_rows_f64(C.byref(desc), C.byref(bufs), None, 1, None, 0, None) == -1
    desc.num_ious = 0
    assert l.lfd_eval_tt100k_workspace_bytes(C.byref(desc)) == 0
    for name, code in (('DET_EXCLUDED', 0), ('DET_RIGHT', 1), ('DET_WRONG', 2), ('DET_UNMATCHED', 3), ('GT_EXCLUDED', 0),
                       ('GT_MISSED', 1), ('GT_MATCHED', 2)):
        assert '#define LFD_TT100K_%s %d' % (name, code) in header and getattr(evaluation, name) == code == getattr(oracle, name)


def test_ctypes_mirrors_of_the_new_structs_match_the_header(tmp_path):
    pairs = {'lfd_eval_tt100k_desc_t': _lib.TT100KEvalDesc, 'lfd_eval_tt100k_bufs_t': _lib.TT100KEvalBufs}
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
