"""The TT100K protocol on the device (csrc/evaluate_tt100k.hip through lfd_amd.evaluation.TT100KEvaluator).  Everything is
compared with `==`: the integers, the outcome codes, the float64 bits of accuracy / recall and the report strings against
what the reference's own eval_annos recorded in tests/golden/ref_tt100k_eval.npz, through `update` and through
`update_resident`; seeded random sets (one image with 120 ground-truth boxes and 2600 detections) against the numpy
restatement tests/golden/tt100k_eval_oracle.py, which test_tt100k_eval_host.py pins to the same fixture; sweeps against
single-combination runs; the device-resident append against the list path on real TT100K_LFD_L outputs at 720p; split
batches, refills, and no synchronisation in update_resident."""
import numpy as np
import pytest
import torch

import tt100k_eval_oracle as oracle
import tt100k_fixture as fx
from lfd_amd import configs, evaluation, ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fix():
    return fx.load()


def make_outputs(dets_list, labels_list):
    """ops.DetectOutputs of a batch from per-image fp32 [k, 5] detections and labels (padded with garbage beyond the count)"""
    n, cap = len(dets_list), max([len(l) for l in labels_list] + [1])
    dets = np.full((n, cap, 5), 12345.0, np.float32)
    labels = np.full((n, cap), 10 ** 6, np.int32)
    counts = np.zeros((n, 4), np.int32)
    for i, (d, l) in enumerate(zip(dets_list, labels_list)):
        dets[i, :len(l)], labels[i, :len(l)], counts[i, 1] = np.asarray(d, np.float32).reshape(-1, 5), l, len(l)
    o = ops.DetectOutputs()
    o.dets, o.labels, o.counts = torch.from_numpy(dets).cuda(), torch.from_numpy(labels).cuda(), torch.from_numpy(counts).cuda()
    o.cand = o.point = o.ws = None
    return o


def feed_rows(ev, rows, meta, batch=8):
    for i in range(0, len(meta), batch):
        ev.update((rows[i:i + batch], meta[i:i + batch]))


def feed_resident(ev, det, det_label, det_img, meta, batch=8):
    for i in range(0, len(meta), batch):
        idx = range(i, min(i + batch, len(meta)))
        ev.update_resident(make_outputs([det[det_img == k] for k in idx], [det_label[det_img == k] for k in idx]), meta[i:i + batch])


def snapshot(ev):
    return dict((k, getattr(ev, k).copy()) for k in ('right', 'num_detections', 'num_ground_truth', 'accuracy', 'recall'))


def same_snapshot(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in a)


def check_against_oracle(ev, images, names_of_oracle_cats, in_types, label=''):
    """ev was evaluated with keep_matches=True on `images` (in the evaluator's image order): counts, per-category counts, every
    outcome code and every matched ground-truth index equal the oracle's"""
    T, M, S = len(ev.ious), len(ev.minscores), len(ev.size_ranges)
    r = oracle.evaluate(images, [float(v) for v in ev.ious], [float(v) for v in ev.minscores],
                        [[float(a), float(b)] for a, b in ev.size_ranges], in_types, ev.check_type, ev.match_same,
                        num_categories=len(names_of_oracle_cats))
    for k in ('right', 'num_detections', 'num_ground_truth'):
        assert getattr(ev, k).dtype == np.int64 and np.array_equal(getattr(ev, k), r[k]), (label, k, getattr(ev, k), r[k])
    assert ev.accuracy.tobytes() == r['accuracy'].tobytes() and ev.recall.tobytes() == r['recall'].tobytes(), label
    if ev.match_same:
        perm = [ev.category_names.index(n) for n in names_of_oracle_cats]
        rest = np.setdiff1d(np.arange(len(ev.category_names)), perm)
        for i, k in enumerate(('right_per_category', 'num_detections_per_category', 'num_ground_truth_per_category')):
            got = getattr(ev, k)
            assert np.array_equal(got[..., perm], r['per_category'][..., i]) and not got[..., rest].any(), (label, k)
    wrong = cells = 0
    for t in range(T):
        for m in range(M):
            for s in range(S):
                tab = ev.match_table(t, m, s)
                det = np.concatenate([c[t][m][s] for c in r['det_code']])
                gt = np.concatenate([c[t][m][s] for c in r['gt_code']])
                dgt = np.concatenate([c[t][m] for c in r['det_gt']])
                assert tab['det_code'].shape == det.shape and tab['gt_code'].shape == gt.shape
                wrong += int((tab['det_code'] != det).sum()) + int((tab['gt_code'] != gt).sum()) + int((tab['det_gt'] != dgt).sum())
                cells += 1
    print('%s: %d combinations x (%d detections + %d ground truth): %d codes or partners differ from the oracle' % (
        label, cells, len(det), len(gt), wrong))
    assert wrong == 0
    return r


@pytest.mark.parametrize('path', ['update', 'update_resident'])
def test_every_fixture_group_equals_the_reference(fix, path):
    ann, meta = fix.annotations(), fix.meta()
    rows = fix.rows()
    for g in range(fix.num_groups):
        p, want = fix.params(g), fix.expected(g)
        ev = evaluation.TT100KEvaluator(annotations=ann, label_indexes_to_category_names=fix.names, types=p['types'], iou=p['ious'],
                                        minscore=p['minscores'], size_ranges=p['size_ranges'], check_type=p['check_type'],
                                        match_same=p['match_same'])
        if path == 'update':
            feed_rows(ev, rows, meta)
        else:
            feed_resident(ev, fix.det, fix.det_label, fix.det_img, meta)
        ev.evaluate(keep_matches=True)
        for k in ('right', 'num_detections', 'num_ground_truth'):
            assert np.array_equal(getattr(ev, k), want[k]), (g, k, getattr(ev, k), want[k])
        assert ev.accuracy.tobytes() == want['accuracy'].tobytes() and ev.recall.tobytes() == want['recall'].tobytes(), g
        T, M, S = want['right'].shape
        assert ev.get_eval_display_str().split('\n') == [str(want['report'][t, m, s]) for t in range(T) for m in range(M) for s in range(S)]
        for t in range(T):
            for m in range(M):
                for s in range(S):
                    tab = ev.match_table(t, m, s)
                    assert np.array_equal(tab['index'], np.arange(len(fix.det_label))) and np.array_equal(tab['image'], fix.det_img)
                    assert np.array_equal(tab['det_code'], want['det_code'][t, m, s]), (g, t, m, s)
                    assert np.array_equal(tab['gt_code'] == evaluation.GT_MISSED, want['gt_missed'][t, m, s]), (g, t, m, s)
        check_against_oracle(ev, fix.oracle_images(), fix.cat_names, fix.in_types(p['types']), 'group %d via %s' % (g, path))


def test_default_arguments_print_the_reference_report_line(fix):
    p, want = fix.params(0), fix.expected(0)
    assert (p['types'], p['check_type'], p['match_same']) == (evaluation.TYPE45, True, True)
    t, m, s = p['ious'].index(0.5), p['minscores'].index(90), p['size_ranges'].index([0, 400])
    ev = evaluation.TT100KEvaluator(annotations=fix.annotations(), label_indexes_to_category_names=fix.names)
    feed_rows(ev, fix.rows(), fix.meta(), batch=16)
    ev.evaluate()
    assert ev.get_eval_display_str() == str(want['report'][t, m, s])
    assert ev.accuracy.tobytes() == want['accuracy'][t, m, s].tobytes() and ev.recall.tobytes() == want['recall'][t, m, s].tobytes()
    assert 0.0 < ev.accuracy[0, 0, 0] < 1.0 and 0.0 < ev.recall[0, 0, 0] < 1.0
    with pytest.raises(RuntimeError):
        ev.match_table()                                        # keep_matches was off


NAMES = ['i2', 'pl40', 'pn', 'w57', 'zz_a', 'zz_b']             # two names outside type45


def random_set(seed, n_images=30, big=True):
    """-> (annotations, per-image fp32 detections, labels, oracle images).  Integer-valued coordinates on a coarse grid give
    many exact IoU ties and sizes exactly on the band limits; scores on a grid of 1/64 hit the minscores exactly."""
    rng = np.random.RandomState(seed)
    imgs, dets, labels, images = dict(), [], [], []
    for n in range(n_images):
        large = big and n == 11
        n_gt = 120 if large else (0 if n % 7 == 3 else int(rng.randint(0, 12)))
        gb = np.zeros((n_gt, 4))
        gb[:, :2] = rng.randint(0, 60, (n_gt, 2)) * 16.0
        gb[:, 2:] = gb[:, :2] + rng.choice([16.0, 32.0, 48.0, 96.0, 200.0, 400.0, 33.5], (n_gt, 2))
        gc = rng.randint(0, len(NAMES), n_gt)
        d = []
        if n % 7 != 5:
            for b, c in zip(gb, gc):
                for _ in range(int(rng.randint(0, 4)) + (8 if large else 0)):
                    j = rng.randint(-1, 2, 4) * 4.0
                    d.append([b[0] + j[0], b[1] + j[1], b[2] - 1 + j[2], b[3] - 1 + j[3], rng.randint(16, 65) / 64.0,
                              c if rng.rand() < 0.8 else rng.randint(0, len(NAMES))])
            for _ in range(1400 if large else int(rng.randint(0, 20))):
                x, y = rng.randint(0, 60, 2) * 16.0
                w, h = rng.choice([16.0, 32.0, 48.0, 96.0, 200.0, 400.0], 2)
                d.append([x, y, x + w - 1, y + h - 1, rng.randint(16, 65) / 64.0, rng.randint(0, len(NAMES))])
        d = np.array(d, np.float64).reshape(-1, 6)[rng.permutation(len(d))]
        det, lab = d[:, :5].astype(np.float32), d[:, 5].astype(np.int32)
        iid = str(500 + 3 * n)
        imgs[iid] = dict(objects=[dict(bbox=dict(xmin=b[0], ymin=b[1], xmax=b[2], ymax=b[3]), category=NAMES[c]) for b, c in zip(gb.tolist(), gc)])
        box, score = oracle.detections_from_f32(det)
        dets.append(det)
        labels.append(lab)
        images.append((gb, gc, box, lab, score))
    return dict(imgs=imgs), dets, labels, images


def rows_of(det, lab):
    from lfd_amd.model.lfd import LFD
    return LFD._pack(torch.from_numpy(det), torch.from_numpy(lab)) if len(lab) else []


@pytest.mark.parametrize('types,check_type,match_same', [(['i2', 'pl40', 'pn', 'zz_a'], True, True), (None, True, False),
                                                           (['pn', 'w57', 'zz_b', 'i2'], False, False)])
def test_random_sets_with_a_large_image_equal_the_oracle(types, check_type, match_same):
    ann, dets, labels, images = random_set(20261016)
    assert max(len(l) for l in labels) > 1024 and max(len(im[0]) for im in images) > 64
    meta = [dict(image_id=k) for k in ann['imgs']]
    ev = evaluation.TT100KEvaluator(annotations=ann, label_indexes_to_category_names=NAMES, types=types, iou=[0.5, 0.3, 0.75],
                                    minscore=[25, 50, 90.625], size_ranges=[(0, 32), (32, 96), (96, 400), (0, 400)],
                                    check_type=check_type, match_same=match_same)
    for i in range(0, len(meta), 4):
        ev.update_resident(make_outputs(dets[i:i + 4], labels[i:i + 4]), meta[i:i + 4])
    ev.evaluate(keep_matches=True)
    in_types = None if types is None else np.array([n in types for n in NAMES])
    r = check_against_oracle(ev, images, NAMES, in_types, 'random set, types %s' % (types,))
    assert len(set(r['right'].ravel().tolist())) > 10 and r['right'].max() > 50 and r['right'][:2].min() > 0
    assert r['num_detections'].max() > r['right'].max() and r['num_ground_truth'].max() > r['right'].max()


def test_all_combinations_of_one_evaluate_equal_single_combination_runs():
    ann, dets, labels, images = random_set(5, n_images=16, big=False)
    meta = [dict(image_id=int(k)) for k in ann['imgs']]
    rows = [rows_of(d, l) for d, l in zip(dets, labels)]
    ious, minscores, bands = [0.5, 0.75], [25, 50, 75], [(0, 32), (32, 96), (96, 400)]
    sweep = evaluation.TT100KEvaluator(annotations=ann, label_indexes_to_category_names=NAMES, types=None, iou=ious, minscore=minscores,
                                       size_ranges=bands)
    feed_rows(sweep, rows, meta)
    sweep.evaluate(keep_matches=True)
    assert sweep.right.shape == (2, 3, 3) and len(set(sweep.right.ravel().tolist())) >= 6 and sweep.right.min() > 0
    for t, iou in enumerate(ious):
        for m, ms in enumerate(minscores):
            for s, band in enumerate(bands):
                one = evaluation.TT100KEvaluator(annotations=ann, label_indexes_to_category_names=NAMES, types=None, iou=iou, minscore=ms,
                                                 size_ranges=(band,))
                feed_rows(one, rows, meta, batch=5)
                one.evaluate(keep_matches=True)
                for k in ('right', 'num_detections', 'num_ground_truth', 'accuracy', 'recall'):
                    assert getattr(one, k)[0, 0, 0].tobytes() == getattr(sweep, k)[t, m, s].tobytes(), (k, t, m, s)
                assert np.array_equal(one.right_per_category[0, 0, 0], sweep.right_per_category[t, m, s])
                a, b = one.match_table(), sweep.match_table(t, m, s)
                for k in a:
                    assert np.array_equal(a[k], b[k]), (k, t, m, s)
                assert one.get_eval_display_str() == sweep.report(t, m, s)


def test_split_batches_add_up_and_a_refill_gives_the_same_numbers():
    ann, dets, labels, images = random_set(9, n_images=20, big=False)
    meta = [dict(image_id=k) for k in ann['imgs']]
    kw = dict(annotations=ann, label_indexes_to_category_names=NAMES, types=None, iou=[0.5, 0.75], minscore=[25, 75],
              size_ranges=[(0, 400), (32, 96)])
    ev = evaluation.TT100KEvaluator(**kw)
    ev.update_resident(make_outputs(dets, labels), meta)
    ev.evaluate()
    first = snapshot(ev)
    assert first['right'].min() > 0
    ev.evaluate()                                               # nothing accumulated any more
    assert not ev.right.any() and not ev.num_ground_truth.any() and (ev.accuracy == 1.0).all()
    ev.update_resident(make_outputs(dets[:7], labels[:7]), meta[:7])
    ev.evaluate()
    assert not same_snapshot(snapshot(ev), first)
    for cut in ((0, 1, 4, 20), (0, 13, 20)):                    # different splits, rows and resident mixed, images out of order
        for lo, hi in reversed(list(zip(cut[:-1], cut[1:]))):
            if lo % 2:
                ev.update(([rows_of(d, l) for d, l in zip(dets[lo:hi], labels[lo:hi])], meta[lo:hi]))
            else:
                ev.update_resident(make_outputs(dets[lo:hi], labels[lo:hi]), meta[lo:hi])
        with pytest.raises(ValueError, match='twice'):
            ev.update_resident(make_outputs(dets[:1], labels[:1]), meta[:1])
        ev.evaluate()
        assert same_snapshot(snapshot(ev), first), cut


def test_update_resident_enqueues_without_synchronising():
    ann, dets, labels, images = random_set(3, n_images=12, big=False)
    meta = [dict(image_id=k) for k in ann['imgs']]
    kw = dict(annotations=ann, label_indexes_to_category_names=NAMES, types=None, minscore=50)
    whole = evaluation.TT100KEvaluator(**kw)
    whole.update_resident(make_outputs(dets, labels), meta)
    whole.evaluate()
    halves = evaluation.TT100KEvaluator(**kw)
    a, b = make_outputs(dets[:6], labels[:6]), make_outputs(dets[6:], labels[6:])
    halves.update_resident(a, meta[:6])                          # first use: buffers are sized here
    halves.evaluate()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        halves.update_resident(a, meta[:6])
        halves.update_resident(b, meta[6:])
    finally:
        torch.cuda.set_sync_debug_mode('default')
    halves.evaluate()
    assert same_snapshot(snapshot(whole), snapshot(halves)) and whole.right[0, 0, 0] > 0


def test_a_label_without_a_name_is_an_error_not_a_silent_drop():
    ann, dets, labels, images = random_set(3, n_images=4, big=False)
    meta = [dict(image_id=k) for k in ann['imgs']]
    ev = evaluation.TT100KEvaluator(annotations=ann, label_indexes_to_category_names=NAMES[:3], types=None)
    assert max(int(l.max()) for l in labels if len(l)) >= 3
    ev.update_resident(make_outputs(dets, labels), meta)
    with pytest.raises(RuntimeError, match='label'):
        ev.evaluate()
    ev.evaluate()                                               # the error bits were cleared with the accumulation
    assert not ev.num_detections.any()


def test_update_resident_equals_update_on_real_tt100k_lfd_l_outputs():
    n, h, w = 2, 720, 1280
    m = configs.build_model('TT100K_LFD_L')
    configs.perturb_weights(m)
    m.eval().cuda()
    assert m._num_classes == 45
    x = (torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(11)) * 2 - 1).cuda()
    meta_t = torch.tensor([[float(w), float(h), 1.0]] * n).cuda()
    meta = [dict(image_id=9000 + 5 * i, resized_height=h, resized_width=w, resize_scale=1.0) for i in range(n)]
    chosen = None
    with torch.no_grad():
        for thr in (0.5, 0.3, 0.2, 0.1, 0.05, 0.02, 0.01, 0.005, 0.002, 0.001):
            counts = m.detect_resident(x, meta_t, score_thr=thr).counts.cpu()
            if int(counts[:, 2].max()) != 0:
                break                                           # candidate capacity exceeded: keep the previous threshold
            chosen = (thr, counts[:, 1].tolist())
            if int(counts[:, 1].min()) >= 200:
                break
        assert chosen is not None
        thr = chosen[0]
        res = m.detect_resident(x, meta_t, score_thr=thr)
        out = ops.DetectOutputs()
        out.dets, out.labels, out.counts = res.dets.clone(), res.labels.clone(), res.counts.clone()
        out.cand = out.point = out.ws = None
        m._classification_threshold = thr
        lists = m.get_results(m.forward_resident(x), meta)
    kept = out.counts[:, 1].tolist()
    print('TT100K_LFD_L 720p, score threshold %g: %s boxes kept' % (thr, kept))
    assert [len(r) for r in lists] == kept and min(kept) >= 100, (thr, kept)
    # synthetic ground truth cut from every third detection (shifted and rescaled a little), plus boxes that match nothing
    rng = np.random.RandomState(3)
    imgs = dict()
    for mb, rows in zip(meta, lists):
        objs = [dict(bbox=dict(xmin=r[2] + 0.7, ymin=r[3] - 0.4, xmax=r[2] + 0.7 + r[4] * 1.05, ymax=r[3] - 0.4 + r[5] * 0.97),
                     category=evaluation.TYPE45[r[0]]) for r in rows[::3]]
        for _ in range(5):
            b = rng.uniform(0, 600, 4)
            objs.append(dict(bbox=dict(xmin=b[0], ymin=b[1], xmax=b[0] + b[2] + 1, ymax=b[1] + b[3] + 1), category='pn'))
        imgs[str(mb['image_id'])] = dict(objects=objs)
    # minscore cuts taken from the scores themselves (seeded weights put them in a narrow range above the threshold): the
    # median and the upper decile of score * 100
    scaled = np.sort(np.array([r[1] * 100 for rows in lists for r in rows], np.float64))
    cuts = [0, float(scaled[len(scaled) // 2]), float(scaled[(9 * len(scaled)) // 10])]
    assert cuts[0] < scaled[0] and cuts[1] < cuts[2]
    kw = dict(annotations=dict(imgs=imgs), label_indexes_to_category_names=evaluation.TYPE45, iou=[0.5, 0.75],
              minscore=cuts, size_ranges=[(0, 400), (0, 32), (32, 96), (96, 400)])
    a = evaluation.TT100KEvaluator(**kw)
    a.update((lists, meta))
    a.evaluate(keep_matches=True)
    b = evaluation.TT100KEvaluator(**kw)
    b.update_resident(out, meta)
    b.evaluate(keep_matches=True)
    assert same_snapshot(snapshot(a), snapshot(b)) and a.get_eval_display_str() == b.get_eval_display_str()
    for k in ('right_per_category', 'num_detections_per_category', 'num_ground_truth_per_category'):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    for t in range(2):
        for ms in range(3):
            for s in range(4):
                ta, tb = a.match_table(t, ms, s), b.match_table(t, ms, s)
                for k in ta:
                    assert np.array_equal(ta[k], tb[k]), (k, t, ms, s)
    assert len(a.match_table()['index']) == sum(kept)
    print('right', a.right.tolist(), 'detections', a.num_detections.tolist(), 'ground truth', a.num_ground_truth.tolist())
    assert a.right[0, 0, 0] > a.right[0, 1, 0] > a.right[0, 2, 0] > 0, a.right
    assert a.num_detections[0, 0, 0] == sum(kept) > a.num_detections[0, 1, 0] > a.num_detections[0, 2, 0] > 0
    # and both are the oracle's numbers on the lists
    images = []
    for mb, rows in zip(meta, lists):
        lab, box, score = oracle.detections_from_rows(rows)
        objs = imgs[str(mb['image_id'])]['objects']
        gb = np.array([[o['bbox'][k] for k in ('xmin', 'ymin', 'xmax', 'ymax')] for o in objs], np.float64)
        images.append((gb, np.array([evaluation.TYPE45.index(o['category']) for o in objs]), box, lab, score))
    check_against_oracle(b, images, evaluation.TYPE45, np.ones(45, bool), 'TT100K_LFD_L 720p')
