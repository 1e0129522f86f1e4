"""The WIDERFACE protocol on the device (csrc/evaluate_widerface.hip through lfd_amd.evaluation.WIDERFACEEvaluator) against
the numpy restatement tests/golden/widerface_eval_oracle.py, which test_widerface_eval_host.py pins to answers worked out by
hand.  Everything is compared with `==`: the int64 curve and faces, the float64 bits of ap / precision / recall and every
column of match_table; through `update` and `update_resident`, in both modes (as_written off and on), with batches split
differently, after a refill, on real WIDERFACE_LFD_S outputs; the as_written score rounding of the append kernel on 4096
fp32 scores; a capacity overflow; no synchronisation in update_resident."""
import ctypes as C

import numpy as np
import pytest
import torch

import widerface_eval_oracle as oracle
from lfd_amd import configs, evaluation, ops

pytestmark = pytest.mark.gpu


def make_outputs(dets_list, labels_list=None):
    """ops.DetectOutputs of a batch from per-image fp32 [k, 5] detections and labels (padded with garbage beyond the count)"""
    if labels_list is None:
        labels_list = [np.zeros(len(d), np.int32) for d in dets_list]
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


def rows_of(det, lab=None):
    from lfd_amd.model.lfd import LFD
    lab = np.zeros(len(det), np.int32) if lab is None else lab
    return LFD._pack(torch.from_numpy(det), torch.from_numpy(lab)) if len(det) else []


def xywhs(rows):
    """LFD.get_results rows [label, score, x, y, w, h] -> the oracle's [n, 5] x y w h score"""
    return np.array([[r[2], r[3], r[4], r[5], r[1]] for r in rows], np.float64).reshape(-1, 5)


# (ground-truth boxes, detections): the tile edges 63 / 64 / 65, more boxes than the LDS hit state holds (256), the
# workgroup-size edges 255 / 256 / 257 and an image with many detection tiles
SPECS = [(1, 1), (63, 255), (64, 256), (300, 257), (65, 120), (5, 2600), (10, 0), (0, 30)]


def synthetic_set(seed=20261017, n_images=24):
    """-> (annotations, per-image fp32 detections [k, 5] x1 y1 x2 y2 score).  Ground truth on an integer grid with duplicated
    boxes and every kind of keep-list membership; detections are jittered copies of ground-truth boxes (half of them by whole
    pixels, so that IoUs tie exactly, half by fractions) plus boxes that hit nothing; scores on a grid of 1 / 64 repeat."""
    rng = np.random.RandomState(seed)
    ann, dets = [], []
    for n in range(n_images):
        G, nd = SPECS[n] if n < len(SPECS) else (int(rng.randint(1, 20)), int(rng.randint(5, 80)))
        gb = np.zeros((G, 4))
        gb[:, :2] = rng.randint(0, 200, (G, 2)) * 8.0
        gb[:, 2:] = rng.choice([7.0, 15.0, 23.0, 39.0, 63.0], (G, 2))
        for k in range(G // 6):                                  # duplicated boxes: the first index has to win
            gb[rng.randint(0, G)] = gb[rng.randint(0, G)]
        kind = rng.randint(0, 5, G)                              # none, hard, medium + hard, all three, easy only
        keep = dict(easy=np.nonzero((kind == 3) | (kind == 4))[0].tolist(), medium=np.nonzero((kind == 2) | (kind == 3))[0].tolist(),
                    hard=np.nonzero((kind >= 1) & (kind <= 3))[0].tolist())
        d = np.zeros((nd, 5))
        for j in range(nd):
            if G and rng.rand() < 0.8:
                b = gb[rng.randint(0, G)]
                jit = rng.randint(-2, 3, 4) * 1.0 if rng.rand() < 0.5 else rng.uniform(-2.5, 2.5, 4)
                d[j, :4] = [b[0] + jit[0], b[1] + jit[1], b[0] + b[2] + jit[2], b[1] + b[3] + jit[3]]
            else:
                x, y = rng.randint(0, 1700, 2)
                d[j, :4] = [x, y, x + rng.randint(4, 60), y + rng.randint(4, 60)]
            d[j, 4] = rng.randint(1, 65) / 64.0
        if n == 8:                                               # IoU exactly 0.5: intersection 4, union 8 (as xywh (.., 1, 2) and (.., 2, 1))
            gb = np.concatenate([gb, [[5000.0, 5000.0, 1.0, 2.0]]])
            keep['easy'].append(len(gb) - 1)
            keep['hard'].append(len(gb) - 1)
            d = np.concatenate([d, [[5000.0, 5000.0, 5000.0 + 2 - 1, 5000.0 + 1 - 1, 0.75]]])
        ann.append(dict(id=700 + 3 * n, event='%d--Event' % (n % 3), stem='%d_Event_%d' % (n % 3, n), boxes=gb, keep=keep))
        dets.append(d.astype(np.float32))
    return ann, dets


class Case(object):
    """the seeded set with its list rows and, per mode, the oracle's answer (computed once)"""

    def __init__(self):
        self.ann, self.dets = synthetic_set()
        self.meta = [dict(image_id=a['id']) for a in self.ann]
        self.rows = [rows_of(d) for d in self.dets]
        self._oracle = dict()

    def oracle(self, as_written):
        if as_written not in self._oracle:
            images = [(a['boxes'], a['keep'], xywhs(r)) for a, r in zip(self.ann, self.rows)]
            self._oracle[as_written] = oracle.evaluate(images, as_written=as_written)
        return self._oracle[as_written]


@pytest.fixture(scope='module')
def case():
    return Case()


def snapshot(ev):
    return dict((k, getattr(ev, k).copy()) for k in ('curve', 'faces', 'ap', 'precision', 'recall'))


def same_snapshot(a, b):
    return all(a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes() for k in a)


def check_against_oracle(ev, r, stored_per_image, label=''):
    """ev was evaluated with keep_matches=True on images fed in annotation order, stored_per_image[i] rows each (the dummy row
    included): curve, faces, the float64 bits of ap / precision / recall and every match_table column equal the oracle's.
    -> (cells compared, cells that differ)"""
    assert ev.curve.dtype == np.int64 and ev.faces.dtype == np.int64 and ev.ap.dtype == np.float64
    cells = ev.curve.size + ev.faces.size + ev.ap.size + ev.precision.size + ev.recall.size
    wrong = int((ev.curve != r['curve']).sum()) + int((ev.faces != r['faces']).sum())
    for k in ('ap', 'precision', 'recall'):
        wrong += int((getattr(ev, k).view(np.int64) != r[k].view(np.int64)).sum())
    base = np.concatenate([[0], np.cumsum(stored_per_image)])
    ranked = [(i, im) for i, im in enumerate(r['images']) if im is not None]
    want = dict(image=np.concatenate([np.full(len(im['m']), i) for i, im in ranked]),
                index=np.concatenate([base[i] + im['order'] for i, im in ranked]),
                rank=np.concatenate([np.arange(len(im['m'])) for i, im in ranked]),
                m=np.concatenate([im['m'] for i, im in ranked]), over=np.concatenate([im['over'] for i, im in ranked]))
    for d in range(3):
        tab = ev.match_table(d)
        want['proposal'] = np.concatenate([im['proposal'][d] for i, im in ranked]).astype(bool)
        want['rec'] = np.concatenate([im['rec'][d] for i, im in ranked])
        for k in ('image', 'index', 'rank', 'm', 'over', 'proposal', 'rec'):
            assert tab[k].shape == want[k].shape, (label, k, tab[k].shape, want[k].shape)
            wrong += int((tab[k] != want[k]).sum())
            cells += want[k].size
    print('%s: %d cells compared with the oracle (integers, float64 bits, match table), %d differ' % (label, cells, wrong))
    assert wrong == 0, label
    return cells, wrong


@pytest.mark.parametrize('path', ['update', 'update_resident'])
@pytest.mark.parametrize('as_written', [False, True])
def test_the_seeded_set_equals_the_oracle(case, as_written, path):
    assert sorted(set(len(a['boxes']) for a in case.ann) & {0, 1, 63, 64, 65, 300}) == [0, 1, 63, 64, 65, 300]
    assert sorted(set(len(d) for d in case.dets) & {0, 1, 255, 256, 257, 2600}) == [0, 1, 255, 256, 257, 2600]
    ev = evaluation.WIDERFACEEvaluator(annotations=case.ann, as_written=as_written)
    for i in range(0, len(case.meta), 8):
        if path == 'update':
            ev.update((case.rows[i:i + 8], case.meta[i:i + 8]))
        else:
            ev.update_resident(make_outputs(case.dets[i:i + 8]), case.meta[i:i + 8])
    got = ev.evaluate(keep_matches=True)
    r = case.oracle(as_written)
    assert all(r['curve'][d, -1, 1] > 0 for d in range(3)) and (r['curve'][:, 500, 1] > 0).all() and len(set(r['ap'].tolist())) == 3
    assert 0 < r['ap'].min() and r['ap'].max() < 1
    check_against_oracle(ev, r, [len(d) + int(as_written) for d in case.dets], 'seeded set, as_written %s, %s' % (as_written, path))
    assert got == dict(easy=r['ap'][0], medium=r['ap'][1], hard=r['ap'][2])
    assert ev.get_eval_display_str() == '\n' + ''.join('{:<10}:{:.5f}\n'.format(n + ' AP', r['ap'][i]) for i, n in enumerate(oracle.DIFFICULTIES))


@pytest.mark.parametrize('as_written', [False, True])
def test_split_batches_mixed_paths_and_a_refill_give_the_same_numbers(case, as_written):
    r = case.oracle(as_written)
    ev = evaluation.WIDERFACEEvaluator(annotations=case.ann, as_written=as_written)
    ev.update_resident(make_outputs(case.dets), case.meta)
    ev.evaluate()
    first = snapshot(ev)
    assert np.array_equal(first['curve'], r['curve']) and first['ap'].tobytes() == r['ap'].tobytes()
    ev.evaluate()                                               # nothing accumulated any more
    assert not ev.curve.any() and not ev.ap.any() and np.array_equal(ev.faces, r['faces'])
    ev.update_resident(make_outputs(case.dets[:7]), case.meta[:7])
    ev.evaluate()
    assert not same_snapshot(snapshot(ev), first)
    n = len(case.meta)
    for cut in ((0, 1, 4, 9, n), (0, 13, n)):                   # different splits, rows and resident mixed, images out of order
        for lo, hi in reversed(list(zip(cut[:-1], cut[1:]))):
            if lo % 2:
                ev.update((case.rows[lo:hi], case.meta[lo:hi]))
            else:
                ev.update_resident(make_outputs(case.dets[lo:hi]), case.meta[lo:hi])
        with pytest.raises(ValueError, match='twice'):
            ev.update_resident(make_outputs(case.dets[:1]), case.meta[:1])
        ev.evaluate()
        assert same_snapshot(snapshot(ev), first), cut


def test_label_index_drops_the_other_labels_on_both_paths(case):
    rng = np.random.RandomState(5)
    sel = list(range(8, 20))
    ann, meta = [case.ann[i] for i in sel], [case.meta[i] for i in sel]
    dets = [case.dets[i] for i in sel]
    labels = [rng.randint(0, 3, len(d)).astype(np.int32) for d in dets]
    r = oracle.evaluate([(a['boxes'], a['keep'], xywhs(rows_of(d[l == 1]))) for a, d, l in zip(ann, dets, labels)])
    assert (r['curve'][:, -1, 1] > 0).all()
    a = evaluation.WIDERFACEEvaluator(annotations=ann, label_index=1)
    a.update(([rows_of(d, l) for d, l in zip(dets, labels)], meta))
    a.evaluate(keep_matches=True)
    b = evaluation.WIDERFACEEvaluator(annotations=ann, label_index=1)
    b.update_resident(make_outputs(dets, labels), meta)
    b.evaluate(keep_matches=True)
    assert same_snapshot(snapshot(a), snapshot(b))
    # the store index counts the dropped rows on the resident path only (they keep their slot there); all else is equal
    kept_at = np.concatenate([np.nonzero(l == 1)[0] + o for l, o in zip(labels, np.cumsum([0] + [len(l) for l in labels[:-1]]))])
    for d in range(3):
        ta, tb = a.match_table(d), b.match_table(d)
        assert all(np.array_equal(ta[k], tb[k]) for k in ta if k != 'index'), d
        assert np.array_equal(kept_at[ta['index']], tb['index'])
    assert np.array_equal(a.curve, r['curve']) and a.ap.tobytes() == r['ap'].tobytes()


def test_a_written_directory_read_back_gives_the_as_written_curve_on_the_device(case, tmp_path):
    sel = list(range(8, 24))
    ann, meta = [case.ann[i] for i in sel], [case.meta[i] for i in sel]
    rows = [case.rows[i] for i in sel]
    evaluation.write_widerface_results(rows[:9], meta[:9], ann, str(tmp_path))
    evaluation.write_widerface_results(rows[9:-1], meta[9:-1], ann, str(tmp_path))       # the last image is never passed
    back, back_meta = evaluation.read_widerface_results(str(tmp_path), ann)
    assert [m['image_id'] for m in back_meta] == [m['image_id'] for m in meta[:-1]]
    assert [len(b) for b in back] == [len(r) + 1 for r in rows[:-1]]
    a = evaluation.WIDERFACEEvaluator(annotations=ann, as_written=False)
    a.update((back, back_meta))
    a.evaluate(keep_matches=True)
    b = evaluation.WIDERFACEEvaluator(annotations=ann, as_written=True)
    b.update((rows[:-1], meta[:-1]))
    b.evaluate(keep_matches=True)
    assert same_snapshot(snapshot(a), snapshot(b)) and (a.curve[:, -1, 1] > 0).all()
    for d in range(3):
        ta, tb = a.match_table(d), b.match_table(d)
        assert all(np.array_equal(ta[k], tb[k]) for k in ta), d
    r = oracle.evaluate([(an['boxes'], an['keep'], xywhs(rw) if i < len(sel) - 1 else None) for i, (an, rw) in enumerate(zip(ann, rows))],
                        as_written=True)
    assert np.array_equal(a.curve, r['curve']) and a.ap.tobytes() == r['ap'].tobytes()


def test_a_capacity_overflow_stores_nothing_sets_the_error_bit_and_evaluate_raises(case):
    ev = evaluation.WIDERFACEEvaluator(annotations=case.ann, as_written=True)
    d = ev._state()
    small = ev._desc()
    small.det_capacity = 10
    bufs = ev._bufs()
    rows = torch.zeros((11, 6), dtype=torch.float64, device=d.dev)
    d.lib.check(d.lib.lib().lfd_eval_wf_append_rows_f64(C.byref(small), C.byref(bufs), d.lib.ptr(rows), 11, d.lib.stream_ptr()), 'rows')
    assert d.state.tolist()[:2] == [0, evaluation.ERR_CAPACITY]
    d.state.zero_()
    out = make_outputs([case.dets[9][:5], case.dets[10][:4]])             # 5 + 4 boxes and two dummy rows: 11 > 10
    ords = torch.tensor([9, 10], dtype=torch.int32, device=d.dev)
    args = (d.lib.ptr(out.dets), d.lib.ptr(out.labels), d.lib.ptr(out.counts), 2, int(out.dets.size(1)), d.lib.ptr(ords), d.lib.stream_ptr())
    d.lib.check(d.lib.lib().lfd_eval_wf_append_dets_f32(C.byref(small), C.byref(bufs), *args), 'dets')
    assert d.state.tolist()[:2] == [0, evaluation.ERR_CAPACITY]
    ev._upper = 1                                               # something was offered: evaluate() has to look at the status word
    with pytest.raises(RuntimeError, match='overflowed'):
        ev.evaluate()
    ev.evaluate()                                               # the error bits were cleared with the accumulation
    assert not ev.curve.any()
    small.det_capacity = 11
    d.lib.check(d.lib.lib().lfd_eval_wf_append_dets_f32(C.byref(small), C.byref(bufs), *args), 'dets')
    assert d.state.tolist()[:2] == [11, 0]
    bad = torch.tensor([len(case.ann)], dtype=torch.int32, device=d.dev)
    one = make_outputs([case.dets[9][:5]])
    d.lib.check(d.lib.lib().lfd_eval_wf_append_dets_f32(C.byref(ev._desc()), C.byref(bufs), d.lib.ptr(one.dets), d.lib.ptr(one.labels),
                                                        d.lib.ptr(one.counts), 1, int(one.dets.size(1)), d.lib.ptr(bad), d.lib.stream_ptr()), 'dets')
    assert d.state.tolist()[1] == evaluation.ERR_IMAGE
    ev._clear()


def rounding_scores():
    """4096 fp32 scores: every k / 2000 that fp32 holds exactly (k a multiple of 125: the sixteenths), the fp32 nearest to
    every tie (2k + 1) / 2000, the fp32 neighbours of all of these, 0, 1, values above 1 and seeded random ones"""
    exact = np.arange(17, dtype=np.float32) / np.float32(16)
    assert all(float(v) * 2000 == round(float(v) * 2000) for v in exact)
    ties = ((2 * np.arange(1000) + 1) / 2000.0).astype(np.float32)
    core = np.concatenate([exact, ties])
    s = np.concatenate([core, np.nextafter(core, np.float32(2)), np.nextafter(core, np.float32(-1)),
                        np.array([0.0, 1.0, 1.0000001, 1.5, 7.25, 0.0005, 0.9995, 0.99949997], np.float32)])
    rng = np.random.RandomState(11)
    s = np.concatenate([s, rng.uniform(0, 1.05, 4096 - len(s)).astype(np.float32)])
    assert len(s) == 4096 and s.dtype == np.float32
    return s


def test_the_resident_append_rounds_scores_as_the_text_file_does(case):
    s = rounding_scores()
    det = np.zeros((len(s), 5), np.float32)
    det[:, 0], det[:, 1], det[:, 2], det[:, 3], det[:, 4] = 3.25, 4.75, 10.5, 20.0, s
    ev = evaluation.WIDERFACEEvaluator(annotations=case.ann[:2], as_written=True)
    ev.update_resident(make_outputs([det]), case.meta[:1])
    d = ev._dev
    assert d.state.tolist()[:2] == [len(s) + 1, 0]
    got = d.det_score[:len(s) + 1].cpu().numpy()
    box = d.det_box[:len(s) + 1].cpu().numpy()
    want = np.array([0.001] + [float('%.03f' % min(float(v), 1)) for v in s], np.float64)
    ties = sum(1 for v in s if (float(v) * 2000) % 2 == 1)
    differ = int((got.view(np.int64) != want.view(np.int64)).sum())
    print('%d fp32 scores (%d exact ties): %d float64 results differ from the formatted string' % (len(s), ties, differ))
    assert ties >= 8 and differ == 0
    assert box[0].tolist() == [0, 0, 0, 0] and (box[1:] == [3.0, 4.0, 9.0, 17.0]).all()       # floor, floor, ceil(8.25), ceil(16.25)
    ev._clear()


def test_resident_list_and_oracle_agree_on_real_widerface_lfd_s_outputs_without_synchronising():
    n, h, w = 2, 256, 256
    m = configs.build_model('WIDERFACE_LFD_S')
    configs.perturb_weights(m)
    m.eval().cuda()
    x = (torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(11)) * 2 - 1).cuda()
    meta_t = torch.tensor([[float(w), float(h), 1.0]] * n).cuda()
    meta = [dict(image_id=9000 + 5 * i, resized_height=h, resized_width=w, resize_scale=1.0) for i in range(n)]
    chosen = None
    with torch.no_grad():
        for thr in (0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1, 0.05, 0.02, 0.01, 0.005, 0.002, 0.001):
            counts = m.detect_resident(x, meta_t, score_thr=thr).counts.cpu()
            if int(counts[:, 2].max()) == 0 and 50 <= int(counts[:, 1].min()) and int(counts[:, 1].max()) <= 2000:
                chosen = thr
                break
        assert chosen is not None, 'no score threshold gives between 50 and 2000 boxes per image'
        res = m.detect_resident(x, meta_t, score_thr=chosen)
        out = ops.DetectOutputs()
        out.dets, out.labels, out.counts = res.dets.clone(), res.labels.clone(), res.counts.clone()
        out.cand = out.point = out.ws = None
        m._classification_threshold = chosen
        lists = m.get_results(m.forward_resident(x), meta)
    kept = out.counts[:, 1].tolist()
    print('WIDERFACE_LFD_S 256 x 256, score threshold %g: %s boxes kept' % (chosen, kept))
    assert [len(r) for r in lists] == kept and 50 <= min(kept) and max(kept) <= 2000
    # random ground truth: boxes cut from every third detection (shifted and rescaled a little) and boxes that match nothing
    rng = np.random.RandomState(3)
    ann = []
    for mb, rows in zip(meta, lists):
        gb = [[r[2] + 0.7, r[3] - 0.4, r[4] * 1.05, r[5] * 0.97] for r in rows[::3]] + rng.uniform(1, 120, (5, 4)).tolist()
        kind = rng.randint(0, 4, len(gb))
        ann.append(dict(id=mb['image_id'], event='0--Real', stem='0_Real_%d' % mb['image_id'], boxes=np.array(gb, np.float64),
                        keep=dict(easy=np.nonzero(kind == 3)[0].tolist(), medium=np.nonzero(kind >= 2)[0].tolist(),
                                  hard=np.nonzero(kind >= 1)[0].tolist())))
    total = 0
    for as_written in (False, True):
        a = evaluation.WIDERFACEEvaluator(annotations=ann, as_written=as_written)
        a.update((lists, meta))
        a.evaluate(keep_matches=True)
        b = evaluation.WIDERFACEEvaluator(annotations=ann, as_written=as_written)
        b.update_resident(out, meta)                            # first use: buffers are sized here
        b.evaluate()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')
        try:
            b.update_resident(out, meta)
        finally:
            torch.cuda.set_sync_debug_mode('default')
        b.evaluate(keep_matches=True)
        assert same_snapshot(snapshot(a), snapshot(b))
        for d in range(3):
            ta, tb = a.match_table(d), b.match_table(d)
            assert all(np.array_equal(ta[k], tb[k]) for k in ta), d
        r = oracle.evaluate([(an['boxes'], an['keep'], xywhs(rows)) for an, rows in zip(ann, lists)], as_written=as_written)
        assert (r['curve'][:, -1, 1] > 0).all()
        total += check_against_oracle(b, r, [k + int(as_written) for k in kept], 'WIDERFACE_LFD_S, as_written %s' % as_written)[0]
    assert total > 0
