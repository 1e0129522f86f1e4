"""The WIDERFACE protocol on the host: tests/golden/widerface_eval_oracle.py (the yardstick of the kernels) pinned to answers
worked out by hand and written here as literals, the step-6 function and the text-file writer / reader of
lfd_amd.evaluation, and the .mat loader.  No GPU."""
import numpy as np
import pytest

import widerface_eval_oracle as oracle
from lfd_amd import evaluation

E, M, H = 0, 1, 2


def keep(easy, medium, hard):
    return dict(easy=list(easy), medium=list(medium), hard=list(hard))


def three_images():
    a = (np.array([[0, 0, 9, 9], [100, 100, 9, 9]], np.float64), keep([0], [0, 1], [0, 1]),
         np.array([[0, 0, 9, 9, 0.9], [100, 100, 9, 9, 0.7], [50, 50, 9, 9, 0.5]], np.float64))
    b = (np.array([[0, 0, 9, 9]], np.float64), keep([0], [0], [0]), None)
    c = (np.zeros((0, 4)), keep([], [], []), np.array([[0, 0, 5, 5, 1.0], [3, 3, 5, 5, 0.1]], np.float64))
    return [a, b, c]


def segments(*parts):
    """[(first t, last t, proposals, recalled)] -> [1000, 2]"""
    out = np.full((1000, 2), -1, np.int64)
    for t0, t1, p, r in parts:
        out[t0:t1 + 1] = (p, r)
    assert (out >= 0).all()
    return out


def test_three_images_by_hand():
    """Image A: boxes g0 = (0, 0, 9, 9) and g1 = (100, 100, 9, 9); easy keeps [0], medium and hard [0, 1].  Its detections are
    g0 itself at 0.9, g1 itself at 0.7 (IoU 1 each) and a box that overlaps nothing at 0.5.  Image B: one box in all three
    lists and no detections: it only adds to faces.  Image C: no ground truth, detections at 1.0 and 0.1: they only take part
    in the normalisation, lo = 0.1, hi = 1.0, diff = 0.9.

    A's normalised scores are 0.8 / 0.9 = 0.888.., 0.6 / 0.9 = 0.666.., 0.4 / 0.9 = 0.444..; thr[t] = 1 - (t + 1) / 1000 is at
    most 0.888.. from t = 111 (0.888), at most 0.666.. from t = 333, at most 0.444.. from t = 555: n = 0, 1, 2, 3 on
    [0, 110], [111, 332], [333, 554], [555, 999].
    easy: the second detection's best box g1 is not kept: proposal 0.  proposal = 1 0 1, running 1 1 2; recalled 1 1 1.
    medium, hard: proposal 1 1 1, running 1 2 3; recalled 1 2 2.
    faces: easy 1 + 1 = 2, medium and hard 2 + 1 = 3.
    AP easy: recall 0 then 1 / 2 from t = 111, precision there 1 (then 1 / 2 from 555): (0.5 - 0) * 1 + (1 - 0.5) * 0.
    AP medium: recall 1 / 3 from 111 and 2 / 3 from 333, both at enveloped precision 1: 1 / 3 + (2 / 3 - 1 / 3)."""
    r = oracle.evaluate(three_images())
    assert (r['lo'], r['hi']) == (0.1, 1.0)
    assert r['faces'].tolist() == [2, 3, 3]
    assert np.array_equal(r['curve'][E], segments((0, 110, 0, 0), (111, 332, 1, 1), (333, 554, 1, 1), (555, 999, 2, 1)))
    for d in (M, H):
        assert np.array_equal(r['curve'][d], segments((0, 110, 0, 0), (111, 332, 1, 1), (333, 554, 2, 2), (555, 999, 3, 2)))
    assert r['ap'].tolist() == [0.5, 1 / 3 + (2 / 3 - 1 / 3), 1 / 3 + (2 / 3 - 1 / 3)]
    a, b, c = r['images']
    assert b is None and c is None
    assert a['order'].tolist() == [0, 1, 2] and a['m'].tolist() == [0, 1, 0] and a['over'].tolist() == [True, True, False]
    assert a['proposal'].tolist() == [[1, 0, 1], [1, 1, 1], [1, 1, 1]] and a['rec'].tolist() == [[1, 1, 1], [1, 2, 2], [1, 2, 2]]
    assert a['score'].tolist() == [(0.9 - 0.1) / (1.0 - 0.1), (0.7 - 0.1) / (1.0 - 0.1), (0.5 - 0.1) / (1.0 - 0.1)]
    # step 6 of the package is the same function of the integers
    p, rc, ap = evaluation.widerface_ap(r['curve'], r['faces'])
    assert p.tobytes() == r['precision'].tobytes() and rc.tobytes() == r['recall'].tobytes() and ap.tobytes() == r['ap'].tobytes()
    assert p[E, 110] == 0.0 and p[E, 111] == 1.0 and p[E, 555] == 0.5 and rc[M, 333] == 2 / 3


def test_an_iou_of_exactly_one_half_matches_and_a_single_score_normalises_to_zero():
    """ground truth (0, 0, 1, 2), detection (0, 0, 2, 1): iw = min(2, 1) - 0 + 1 = 2, ih = min(1, 2) - 0 + 1 = 2, intersection 4,
    union 3 * 2 + 2 * 3 - 4 = 8.  One score only: diff == 0 becomes 1, s' = 0, and only thr[999] = 0 counts it."""
    assert oracle.iou([0, 0, 2, 1], [0, 0, 1, 2]) == 0.5
    img = (np.array([[0, 0, 1, 2]], np.float64), keep([0], [0], []), np.array([[0, 0, 2, 1, 0.37]]))
    r = oracle.evaluate([img])
    assert r['lo'] == r['hi'] == 0.37 and r['images'][0]['score'].tolist() == [0.0] and r['images'][0]['over'].tolist() == [True]
    assert oracle.thresholds()[999] == 0.0
    assert not r['curve'][:, :999].any()
    assert r['curve'][:, 999].tolist() == [[1, 1], [1, 1], [0, 0]]          # hard does not keep the box: no proposal
    assert r['ap'].tolist() == [1.0, 1.0, 0.0] and r['faces'].tolist() == [1, 1, 0]
    r = oracle.evaluate([img], iou_thresh=0.5000001)
    assert r['images'][0]['over'].tolist() == [False] and r['curve'][:, 999].tolist() == [[1, 0], [1, 0], [1, 0]]


def test_of_two_identical_boxes_the_first_is_matched():
    img = (np.array([[50, 50, 9, 9], [10, 10, 20, 20], [10, 10, 20, 20]], np.float64), keep([2], [1], [1, 2]),
           np.array([[11, 10, 20, 20, 0.8], [10, 10, 20, 20, 0.6]]))
    r = oracle.evaluate([img])
    im = r['images'][0]
    assert im['m'].tolist() == [1, 1] and im['over'].tolist() == [True, True]
    assert im['proposal'].tolist() == [[0, 0], [1, 1], [1, 1]] and im['rec'].tolist() == [[0, 0], [1, 1], [1, 1]]


def test_a_best_box_outside_the_keep_list_takes_the_proposal_away_and_stays_minus_one():
    """box 0 is kept by hard only.  easy: both detections on box 0 are no proposals (hit[0] = -1 and stays), the third one
    recalls box 1.  hard: the first detection recalls box 0, the second is a proposal that recalls nothing new."""
    img = (np.array([[0, 0, 19, 19], [100, 0, 19, 19]], np.float64), keep([1], [1], [0, 1]),
           np.array([[0, 0, 19, 19, 0.9], [1, 0, 19, 19, 0.8], [100, 0, 19, 19, 0.7], [300, 300, 5, 5, 0.1]]))
    im = oracle.evaluate([img])['images'][0]
    assert im['m'].tolist() == [0, 0, 1, 0] and im['over'].tolist() == [True, True, True, False]
    assert im['proposal'].tolist() == [[0, 0, 1, 1], [0, 0, 1, 1], [1, 1, 1, 1]]
    assert im['rec'].tolist() == [[0, 0, 1, 1], [0, 0, 1, 1], [1, 1, 2, 2]]


def test_equal_scores_keep_insertion_order():
    img = (np.array([[0, 0, 9, 9]], np.float64), keep([0], [0], [0]),
           np.array([[40, 40, 9, 9, 0.5], [0, 0, 9, 9, 0.9], [0, 1, 9, 9, 0.5], [80, 80, 3, 3, 0.9], [1, 0, 9, 9, 0.5]]))
    im = oracle.evaluate([img])['images'][0]
    assert im['order'].tolist() == [1, 3, 0, 2, 4]
    assert im['score'].tolist() == [1.0, 1.0, 0.0, 0.0, 0.0]
    assert im['rec'][E].tolist() == [1, 1, 1, 1, 1] and np.cumsum(im['proposal'][E]).tolist() == [1, 2, 3, 4, 5]


def test_as_written_quantises_like_the_text_file():
    """'%.03f' rounds the exact binary value half to even: 0.0625 -> 0.062, 0.1875 -> 0.188; a score above 1 is written as 1"""
    rows = oracle.as_written_rows([[3.7, 4.2, 10.1, 12.0, 0.0625], [-0.5, 7.0, 3.0, 2.5, 0.1875], [1, 2, 3, 4, 1.7]])
    assert rows == [[0.0, 0.0, 0.0, 0.0, 0.001], [3.0, 4.0, 11.0, 12.0, 0.062], [-1.0, 7.0, 3.0, 3.0, 0.188], [1.0, 2.0, 3.0, 4.0, 1.0]]
    assert evaluation._quantise_as_written([0, 0.0625, 3.7, 4.2, 10.1, 12.0]) == (0.062, 3.0, 4.0, 11.0, 12.0)
    assert evaluation._quantise_as_written([0, 1.7, -0.5, 7.0, 3.0, 2.5]) == (1.0, -1.0, 7.0, 3.0, 3.0)
    # the dummy row is a detection: it joins the normalisation (lo = 0.001) and the matching
    img = (np.array([[0, 0, 9, 9]], np.float64), keep([0], [0], [0]), np.array([[0.4, 0.2, 8.6, 8.8, 0.5]]))
    r = oracle.evaluate([img, (np.zeros((0, 4)), keep([], [], []), None)], as_written=True)
    assert (r['lo'], r['hi']) == (0.001, 0.5)
    im = r['images'][0]
    assert im['order'].tolist() == [1, 0] and im['over'].tolist() == [True, False] and im['score'].tolist() == [1.0, 0.0]
    assert r['curve'][E, 0].tolist() == [1, 1] and r['curve'][E, 998].tolist() == [1, 1] and r['curve'][E, 999].tolist() == [2, 1]


def test_voc_ap_on_a_known_curve():
    """mrec = 0 .25 .5 .5 1 1, mpre = 0 1 .5 .8 .4 0 -> enveloped 1 1 .8 .8 .4 0; recall changes at i = 0, 1, 3"""
    want = 0.25 * 1.0 + 0.25 * 0.8 + 0.5 * 0.4
    for f in (oracle.voc_ap, evaluation.voc_ap):
        assert f([0.25, 0.5, 0.5, 1.0], [1.0, 0.5, 0.8, 0.4]) == want
        assert f([0.0, 0.0], [0.0, 0.0]) == 0.0
        assert f([1.0], [1.0]) == 1.0


def annotations_of(images):
    return [dict(id='img%d' % i, event='%d--Event' % (i % 2), stem='%d_Event_%d' % (i % 2, i), boxes=b, keep=k)
            for i, (b, k, _) in enumerate(images)]


def random_images(seed, n=6):
    rng = np.random.RandomState(seed)
    images = []
    for i in range(n):
        g = int(rng.randint(1, 6))
        boxes = np.concatenate([rng.uniform(0, 200, (g, 2)), rng.uniform(8, 60, (g, 2))], 1)
        k = keep(*[np.nonzero(rng.rand(g) < p)[0].tolist() for p in (0.4, 0.7, 1.0)])
        d = np.concatenate([boxes[rng.randint(0, g, 12)] + rng.uniform(-3, 3, (12, 4)), rng.uniform(0.01, 1.2, (12, 1))], 1)
        images.append((boxes, k, d if i != 2 else np.zeros((0, 5))))
    return images


def test_the_written_directory_reads_back_to_the_as_written_curve(tmp_path):
    images = random_images(7)
    ann = annotations_of(images)
    rows = [[[0, r[4], r[0], r[1], r[2], r[3]] for r in d.tolist()] for _, _, d in images]
    meta = [dict(image_id=a['id']) for a in ann]
    evaluation.write_widerface_results(rows[:4], meta[:4], ann, str(tmp_path))
    evaluation.write_widerface_results(rows[4:5], meta[4:5], ann, str(tmp_path))          # the last image is never written
    text = (tmp_path / ann[2]['event'] / (ann[2]['stem'] + '.txt')).read_text()
    assert text == ann[2]['stem'] + '\n1\n0 0 0 0 0.001\n'
    first = (tmp_path / ann[0]['event'] / (ann[0]['stem'] + '.txt')).read_text().splitlines()
    assert first[:3] == [ann[0]['stem'], '13', '0 0 0 0 0.001'] and len(first) == 15
    back, back_meta = evaluation.read_widerface_results(str(tmp_path), ann)
    assert [m['image_id'] for m in back_meta] == [a['id'] for a in ann[:5]]
    as_read = [(b, k, np.array([[r[2], r[3], r[4], r[5], r[1]] for r in rows_i], np.float64).reshape(-1, 5))
               for (b, k, _), rows_i in zip(images[:5], back)] + [(images[5][0], images[5][1], None)]
    original = images[:5] + [(images[5][0], images[5][1], None)]
    a, b = oracle.evaluate(as_read, as_written=False), oracle.evaluate(original, as_written=True)
    assert np.array_equal(a['curve'], b['curve']) and np.array_equal(a['faces'], b['faces']) and a['ap'].tobytes() == b['ap'].tobytes()
    assert (a['curve'][:, -1, 1] > 0).all()
    for x, y in zip(a['images'], b['images']):
        assert (x is None) == (y is None)
        if x is not None:
            assert all(np.array_equal(x[k], y[k]) for k in x)


def test_the_evaluator_parses_on_the_host_and_an_empty_evaluate_counts_every_annotated_face():
    images = three_images()
    ann = annotations_of(images)
    ev = evaluation.WIDERFACEEvaluator(annotations=ann)
    assert ev.gt_start.tolist() == [0, 2, 3, 3] and ev.gt_kept.tolist() == [7, 6, 7] and ev.keep_len.tolist() == [[1, 2, 2], [1, 1, 1], [0, 0, 0]]
    assert ev.thr.tobytes() == oracle.thresholds().tobytes() and ev.thr[0] == 0.999 and ev.thr[999] == 0.0
    got = ev.evaluate()
    assert got == dict(easy=0.0, medium=0.0, hard=0.0) and ev.faces.tolist() == [2, 3, 3] and not ev.curve.any()
    assert 'easy AP' in ev.get_eval_display_str()
    with pytest.raises(ValueError, match='not in the annotations'):
        ev.update(([[]], [dict(image_id='nope')]))
    with pytest.raises(ValueError, match='outside'):
        evaluation.WIDERFACEEvaluator(annotations=[dict(id=0, event='e', stem='s', boxes=np.zeros((1, 4)), keep=keep([1], [], []))])
    with pytest.raises(ValueError, match='twice'):
        evaluation.WIDERFACEEvaluator(annotations=ann + ann[:1])


def test_the_mat_loader_reads_what_the_dataset_ships(tmp_path):
    sio = pytest.importorskip('scipy.io')
    def obj(items):                                              # an [n, 1] cell array
        a = np.empty((len(items), 1), object)
        for i, it in enumerate(items):
            a[i, 0] = it
        return a
    events = ['0--Parade', '1--Handshaking']
    stems = [['0_Parade_a_1', '0_Parade_b_2'], ['1_Handshaking_c_3']]
    boxes = [[np.array([[1, 2, 3, 4], [5, 6, 7, 8], [9, 10, 11, 12]], np.float64), np.zeros((0, 4))], [np.array([[20, 21, 22, 23]], np.float64)]]
    lists = dict(easy=[[[1], []], [[1]]], medium=[[[1, 3], []], [[1]]], hard=[[[1, 2, 3], []], [[]]])
    cell = lambda per_event, conv: obj([obj([conv(v) for v in ev]) for ev in per_event])   # noqa: E731
    sio.savemat(str(tmp_path / 'wider_face_val.mat'),
                dict(event_list=obj([np.array([e]) for e in events]), file_list=cell(stems, lambda s: np.array([s])),
                     face_bbx_list=cell(boxes, lambda b: b)))
    for d in ('easy', 'medium', 'hard'):
        sio.savemat(str(tmp_path / ('wider_%s_val.mat' % d)),
                    dict(gt_list=cell(lists[d], lambda v: np.array(v, np.float64).reshape(-1, 1))))
    ann = evaluation.load_widerface_mat(str(tmp_path))
    assert [(a['id'], a['event'], a['stem']) for a in ann] == [(s, e, s) for e, ss in zip(events, stems) for s in ss]
    assert ann[0]['boxes'].tolist() == boxes[0][0].tolist() and ann[1]['boxes'].shape == (0, 4) and ann[2]['boxes'].tolist() == [[20, 21, 22, 23]]
    assert ann[0]['keep'] == dict(easy=[0], medium=[0, 2], hard=[0, 1, 2])                  # 1-based in the file
    assert ann[1]['keep'] == dict(easy=[], medium=[], hard=[]) and ann[2]['keep'] == dict(easy=[0], medium=[0], hard=[])
    ev = evaluation.WIDERFACEEvaluator(annotations=ann)
    ev.evaluate()
    assert ev.faces.tolist() == [2, 3, 3]
