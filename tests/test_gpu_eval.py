"""Evaluation on the device (csrc/evaluate.hip through lfd_amd/evaluation.py) against the numpy oracle of the definition
(tests/golden/coco_eval_oracle.py) on seeded synthetic sets: the per-detection matched / ignored flags of all 40
(threshold, area range) matchings bit for bit, precision / recall / stats to 1e-12 with every -1 cell in place; the
device-resident append against the list path on real DetectOutputs; no synchronisation in update_resident; split batches;
refills."""
import numpy as np
import pytest
import torch

import coco_eval_oracle as oracle
from lfd_amd import configs, evaluation, ops

pytestmark = pytest.mark.gpu

CAT_IDS = [1, 2, 4, 7, 9]                 # 7: no ground truth, 9: no detections
LABEL_TO_CAT = {0: 1, 1: 2, 2: 4, 3: 7, 4: 9}
CAT_TO_LABEL = dict((v, k) for k, v in LABEL_TO_CAT.items())


def synthetic_set(seed, n_images=64):
    """-> (coco dict, per-image lists of [label, score, x, y, w, h] rows, image ids).  Ground truth: 0-40 boxes per image
    (one image: 150 in one category, more than one tile of 64), 5-10 % crowds, sides log-uniform in [5, 320] so that the
    areas cover all three ranges, an annotated area below w * h, float64 coordinates that fp32 cannot hold.  Detections:
    jittered copies of the ground truth + random false positives, scores rounded to two digits (many ties), up to 300 per
    image, one image with 1300 (1150 of them in one category: more than maxDets[-1] in one pair), images with nothing."""
    rng = np.random.RandomState(seed)
    image_ids = [1000 + 7 * i for i in range(n_images)]
    anns, rows = [], []

    def box():
        w, h = np.exp(rng.uniform(np.log(5), np.log(320), 2))
        return [float(rng.uniform(0, 1200)), float(rng.uniform(0, 800)), float(w), float(h)]
    for n, iid in enumerate(image_ids):
        kind = n % 16
        n_gt = 0 if kind in (3, 5) else int(rng.randint(0, 41))
        gts = []
        for _ in range(n_gt):
            b = box()
            gts.append(dict(image_id=iid, category_id=int(rng.choice([1, 2, 4, 9], p=[.4, .3, .2, .1])), bbox=b,
                            area=b[2] * b[3] * float(rng.uniform(0.5, 1.0)), iscrowd=int(rng.rand() < 0.075)))
        if n == 9:
            for _ in range(150):
                b = box()
                gts.append(dict(image_id=iid, category_id=2, bbox=b, area=b[2] * b[3], iscrowd=int(rng.rand() < 0.05)))
        anns += gts
        dets = []
        if kind not in (5, 7):                                   # 5: nothing at all, 7: ground truth without detections
            for g in gts:
                if g['category_id'] == 9:
                    continue
                for _ in range(int(rng.randint(0, 4))):
                    j = rng.normal(0, 0.08, 4) * [g['bbox'][2], g['bbox'][3], g['bbox'][2], g['bbox'][3]]
                    b = [g['bbox'][0] + j[0], g['bbox'][1] + j[1], max(1.0, g['bbox'][2] + j[2]), max(1.0, g['bbox'][3] + j[3])]
                    dets.append([CAT_TO_LABEL[g['category_id']], round(float(rng.uniform(0.3, 1.0)), 2)] + [float(v) for v in b])
            for _ in range(int(rng.randint(0, 60))):
                dets.append([int(rng.choice([0, 1, 2, 3])), round(float(rng.uniform(0.0, 0.6)), 2)] + box())
            if n == 9:
                for g in gts[-150:]:
                    dets.append([1, round(float(rng.uniform(0.3, 1.0)), 2)] + [float(v) for v in g['bbox']])
            if n == 20:
                for _ in range(1150):
                    dets.append([0, round(float(rng.uniform(0.0, 1.0)), 3)] + box())
                for _ in range(150):
                    dets.append([2, round(float(rng.uniform(0.0, 1.0)), 2)] + box())
            order = rng.permutation(len(dets))
            dets = [dets[i] for i in order][:1300 if n == 20 else 300]
        rows.append(dets)
    for i, a in enumerate(anns):
        a['id'] = i + 1
    coco = dict(images=[dict(id=i) for i in image_ids], categories=[dict(id=c) for c in CAT_IDS], annotations=anns)
    return coco, rows, image_ids


def oracle_inputs(coco, rows, image_ids, all_images):
    dts = [dict(image_id=iid, category_id=LABEL_TO_CAT[r[0]], score=r[1], bbox=r[2:]) for iid, dets in zip(image_ids, rows) for r in dets]
    evaluated = [iid for iid, dets in zip(image_ids, rows) if dets or all_images]
    return coco['annotations'], dts, evaluated


def feed(ev, rows, image_ids, batch=8):
    for i in range(0, len(image_ids), batch):
        ev.update((rows[i:i + batch], [dict(image_id=v) for v in image_ids[i:i + batch]]))


def compare_results(ev, ref):
    assert ev.precision.shape == ref['precision'].shape and ev.recall.shape == ref['recall'].shape
    for name, got, want in (('precision', ev.precision, ref['precision']), ('recall', ev.recall, ref['recall']),
                            ('stats', ev.stats, ref['stats'])):
        assert np.array_equal(got == -1, want == -1), name
        diff = float(np.abs(got - want).max())
        print('%s: max |device - oracle| = %.3e over %d cells (%d of them -1)' % (name, diff, want.size, int((want == -1).sum())))
        assert diff <= 1e-12, (name, diff)


@pytest.mark.parametrize('all_images', [False, True])
def test_flags_precision_recall_and_stats_equal_the_oracle(all_images):
    coco, rows, image_ids = synthetic_set(20261016)
    gts, dts, evaluated = oracle_inputs(coco, rows, image_ids, all_images)
    assert max(len(r) for r in rows) > 1000 and any(not r for r in rows)
    assert len(set(d['score'] for d in dts)) < len(dts) // 4                        # duplicated scores
    assert any(float(np.float32(g['bbox'][0])) != g['bbox'][0] for g in gts)
    ref = oracle.evaluate(gts, dts, evaluated, CAT_IDS)
    ev = evaluation.COCOEvaluator(None, LABEL_TO_CAT, annotations=coco, all_images=all_images)
    feed(ev, rows, image_ids)
    ev.evaluate(keep_matches=True)
    # stage 1: every detection that takes part, all 40 matchings, no tolerance
    tab = ev.match_table()
    want = {}
    for (iid, cid), m in ref['matches'].items():
        for pos, idx in enumerate(m['index']):
            want[idx] = (pos, m['matched'][:, :, pos], m['ignored'][:, :, pos])
    kept = tab['rank'] < 1000
    assert int((~kept).sum()) == len(dts) - len(want) > 0 and sorted(tab['index'][kept].tolist()) == sorted(want)
    assert len(set(tab['index'].tolist())) == len(tab['index']) == len(dts)
    wrong = 0
    for idx, rank, mt, ig in zip(tab['index'][kept], tab['rank'][kept], tab['matched'][kept], tab['ignored'][kept]):
        pos, wm, wi = want[int(idx)]
        wrong += int(pos != rank) + int((mt != wm).sum()) + int((ig != wi).sum())
    print('%d detections x 40 matchings: %d flags or ranks differ' % (int(kept.sum()), wrong))
    assert wrong == 0
    npig = np.zeros((len(CAT_IDS), 4), np.int64)
    for (iid, cid), m in ref['matches'].items():
        npig[CAT_IDS.index(cid)] += m['npig']
    assert np.array_equal(tab['npig'], npig)
    assert (ref['precision'][:, :, 3] == -1).all() and (ref['precision'][:, :, 4, 0] == 0).all()
    # stage 2
    compare_results(ev, ref)
    assert ev.get_eval_display_str() == evaluation.format_display(ref['stats'])
    assert ev.stats[0] != ev.stats[1] and 0.05 < ev.stats[1] < 0.95


def test_refill_gives_the_same_numbers_and_the_accumulators_are_cleared():
    coco, rows, image_ids = synthetic_set(7, n_images=24)
    ev = evaluation.COCOEvaluator(None, LABEL_TO_CAT, annotations=coco)
    feed(ev, rows, image_ids)
    ev.evaluate()
    first = (ev.stats.copy(), ev.precision.copy(), ev.recall.copy())
    ev.evaluate()                                                                   # nothing accumulated any more
    assert ev.stats is None and ev.get_eval_display_str() == '\nNo bboxes detected! Evaluation abort!\n'
    feed(ev, rows[:12], image_ids[:12])
    ev.evaluate()
    assert not np.array_equal(ev.precision, first[1])
    feed(ev, rows, image_ids, batch=5)
    ev.evaluate()
    assert np.array_equal(ev.stats, first[0]) and np.array_equal(ev.precision, first[1]) and np.array_equal(ev.recall, first[2])


def test_hand_cases_on_the_device():
    """the cases tests/test_eval_host.py derives by hand, through the kernels, with the reference's quirk and without"""
    gts = [dict(image_id=1, category_id=1, bbox=[10, 10, 50, 50], area=2500, iscrowd=0),
           dict(image_id=1, category_id=1, bbox=[200, 10, 50, 50], area=2500, iscrowd=0),
           dict(image_id=2, category_id=1, bbox=[5, 5, 60, 60], area=3600, iscrowd=0)]
    rows = [[[0, 0.9, 10, 10, 50, 50], [0, 0.8, 400, 400, 50, 50], [0, 0.7, 200, 10, 50, 50]], []]
    meta = [dict(image_id=1), dict(image_id=2)]
    ev = evaluation.COCOEvaluator(None, {0: 1}, annotations=dict(annotations=gts))
    ev.update((rows, meta))
    ev.evaluate()
    assert abs(ev.stats[0] - 253.0 / 303.0) < 1e-15 and ev.stats[3] == -1 and ev.stats[5] == -1 and ev.stats[8] == 1.0
    assert ev.get_eval_display_str().startswith('\nmAP       :0.83498\nmAP_50    :0.83498\n')
    ev = evaluation.COCOEvaluator(None, {0: 1}, annotations=dict(annotations=gts), all_images=True)
    ev.update((rows, meta))
    ev.evaluate()
    assert abs(ev.stats[0] - 56.0 / 101.0) < 1e-15 and abs(ev.stats[8] - 2.0 / 3.0) < 1e-15


def _model_batch(name, n=4, h=256, w=320):
    m = configs.build_model(name)
    configs.perturb_weights(m)
    m.eval().cuda()
    x = (torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(11)) * 2 - 1).cuda()
    meta = torch.tensor([[float(w), float(h), 1.0]] * n).cuda()
    iou, agn = m._nms_cfg.get('iou_thr', 0.5), m._nms_cfg.get('class_agnostic', False)
    with torch.no_grad():
        cls, reg = m(x)
        for thr in (0.6, 0.5, 0.4, 0.3, 0.2, 0.1, 0.05, 0.02, 0.01, 0.003, 0.001):
            out, counts = m._detect_with_retry(cls, reg, meta, thr, iou, agn)
            if int(counts[:, 1].min()) >= 8:
                break
    assert int(counts[:, 1].min()) >= 8 and int(counts[:, 2].max()) == 0, counts
    m._classification_threshold = thr
    meta_batch = [dict(image_id=50 + 3 * i, resized_height=h, resized_width=w, resize_scale=1.0) for i in range(n)]
    lists = m.get_results((cls, reg), meta_batch)
    assert [len(r) for r in lists] == counts[:, 1].tolist()
    # synthetic ground truth: some of the detections themselves (shifted a little), some random boxes, a crowd
    rng = np.random.RandomState(3)
    anns = []
    for mb, dets in zip(meta_batch, lists):
        for r in dets[::3]:
            anns.append(dict(image_id=mb['image_id'], category_id=r[0] + 1, bbox=[r[2] + 0.7, r[3] - 0.4, r[4] * 1.05, r[5] * 0.97],
                             area=r[4] * r[5], iscrowd=0))
        for _ in range(5):
            b = [float(v) for v in rng.uniform(0, 200, 4)]
            anns.append(dict(image_id=mb['image_id'], category_id=int(rng.randint(1, m._num_classes + 1)), bbox=b, area=b[2] * b[3],
                             iscrowd=int(rng.rand() < 0.2)))
    coco = dict(images=[dict(id=mb['image_id']) for mb in meta_batch], categories=[dict(id=c + 1) for c in range(m._num_classes)],
                annotations=anns)
    label_map = dict((c, c + 1) for c in range(m._num_classes))
    return m, out, lists, meta_batch, coco, label_map


@pytest.mark.parametrize('name,classes', [('TT100K_LFD_L', 45), ('WIDERFACE_LFD_S', 1)])
def test_update_resident_equals_update_on_the_lists(name, classes):
    m, out, lists, meta_batch, coco, label_map = _model_batch(name)
    assert m._num_classes == classes
    a = evaluation.COCOEvaluator(None, label_map, annotations=coco)
    a.update((lists, meta_batch))
    a.evaluate(keep_matches=True)
    b = evaluation.COCOEvaluator(None, label_map, annotations=coco)
    b.update_resident(out, meta_batch)
    b.evaluate(keep_matches=True)
    ta, tb = a.match_table(), b.match_table()
    for k in ta:
        assert np.array_equal(ta[k], tb[k]), k
    assert len(ta['index']) == sum(len(r) for r in lists)
    assert np.array_equal(a.stats, b.stats) and np.array_equal(a.precision, b.precision) and np.array_equal(a.recall, b.recall)
    assert a.stats[1] > 0.0, a.stats
    # and the list path is the oracle's
    dts = [dict(image_id=mb['image_id'], category_id=label_map[r[0]], score=r[1], bbox=r[2:]) for mb, dets in zip(meta_batch, lists)
           for r in dets]
    ref = oracle.evaluate(coco['annotations'], dts, [mb['image_id'] for mb in meta_batch], sorted(label_map.values()))
    compare_results(b, ref)


def _slice_outputs(out, lo, hi):
    s = ops.DetectOutputs()
    s.dets, s.labels, s.counts = out.dets[lo:hi], out.labels[lo:hi], out.counts[lo:hi]
    s.cand = s.point = s.ws = None
    return s


def test_update_resident_does_not_synchronise_and_split_batches_add_up():
    m, out, lists, meta_batch, coco, label_map = _model_batch('WIDERFACE_LFD_S')
    whole = evaluation.COCOEvaluator(None, label_map, annotations=coco)
    whole.update_resident(out, meta_batch)
    whole.evaluate()
    halves = evaluation.COCOEvaluator(None, label_map, annotations=coco)
    halves.update_resident(_slice_outputs(out, 0, 1), meta_batch[:1])         # first use: buffers are sized here
    halves.evaluate()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        halves.update_resident(_slice_outputs(out, 0, 2), meta_batch[:2])
        halves.update_resident(_slice_outputs(out, 2, 4), meta_batch[2:])
    finally:
        torch.cuda.set_sync_debug_mode('default')
    halves.evaluate()
    assert np.array_equal(whole.stats, halves.stats) and np.array_equal(whole.precision, halves.precision)
    assert np.array_equal(whole.recall, halves.recall)


def test_a_label_without_a_category_is_an_error_not_a_silent_drop():
    m, out, lists, meta_batch, coco, label_map = _model_batch('TT100K_LFD_L')
    used = sorted(set(r[0] for dets in lists for r in dets))
    partial = dict((c, c + 1) for c in range(m._num_classes) if c != used[0])
    ev = evaluation.COCOEvaluator(None, partial, annotations=coco)
    ev.update_resident(out, meta_batch)
    with pytest.raises(RuntimeError, match='label'):
        ev.evaluate()
