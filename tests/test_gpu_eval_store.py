"""The detection store and the grouping that the three evaluators share (csrc/eval_store.h under csrc/evaluate.hip,
evaluate_tt100k.hip and evaluate_widerface.hip), pinned where the protocol tests leave it open: what one appended row becomes
in every protocol on both append paths (floats bit for bit: every conversion is exact or one IEEE operation), what an image
ordinal or a category out of range does, what a capacity overflow leaves behind, and the grouping at the edges of its
one-workgroup scan (1 image; 1025 images or pairs: two per scan thread, the last threads empty)."""
import ctypes as C

import numpy as np
import pytest
import torch

import coco_eval_oracle
from lfd_amd import evaluation, ops
from lfd_amd.evaluation import ERR_CAPACITY, ERR_IMAGE, ERR_LABEL

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
UNMAPPED = 5                                   # a label that no evaluator below maps
# outputs.dets [3, 4, 5] x1 y1 x2 y2 score; kept counts 2, 0, 4; everything past the count is garbage
DETS = np.full((3, 4, 5), 12345.0, F32)
DETS[0, :2] = [[10.3, 20.7, 50.9, 61.1, 0.87654], [0.1, 0.2, 0.3, 0.4, 1.2]]
DETS[2] = [[100.5, 7.25, 163.3, 40.0, 0.0005], [3.7, 3.3, 9.9, 8.1, 0.4995], [640.1, 360.9, 700.7, 400.3, 0.25],
           [1e-3, 1e3, 1e4, 1e4 + 0.6, 0.9995]]
COUNTS = np.array([[99, 2, 98, 97], [99, 0, 98, 97], [99, 4, 98, 97]], np.int32)
LABELS = np.full((3, 4), 10 ** 6, np.int32)
LABELS[0, :2] = [0, 1]
LABELS[2] = [1, UNMAPPED, 0, 0]
WF_LABELS = np.full((3, 4), 10 ** 6, np.int32)          # label_index 0 filters one row
WF_LABELS[0, :2] = [0, 0]
WF_LABELS[2] = [0, 0, 1, 0]
IMAGE_IDS = [30, 10, 20]                       # the batch's images; their ordinals in every evaluator below are 2, 0, 1
ORDS = [2, 0, 1]


def outputs_of(dets, labels, counts):
    o = ops.DetectOutputs()
    o.dets, o.labels, o.counts = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (dets, labels, counts))
    o.cand = o.point = o.ws = None
    return o


def kept():
    """(batch entry, slot) of every kept detection, in store order"""
    return [(i, j) for i in range(3) for j in range(int(COUNTS[i, 1]))]


def wh32(d):
    """fp32 w = x2 - x1 + 1 and h: two roundings each"""
    return (d[2] - d[0]) + F32(1), (d[3] - d[1]) + F32(1)


def list_rows(labels, skip=()):
    """LFD.get_results rows [label, score, x, y, w, h] per batch entry, from the same numbers"""
    rows = [[], [], []]
    for i, j in kept():
        if int(labels[i, j]) in skip:
            continue
        d = DETS[i, j]
        w, h = wh32(d)
        rows[i].append([int(labels[i, j]), float(d[4]), float(d[0]), float(d[1]), float(w), float(h)])
    return rows


def coco_evaluator(**kw):
    ann = dict(images=[dict(id=i) for i in (10, 20, 30)], categories=[dict(id=c) for c in (1, 3)],
               annotations=[dict(id=1, image_id=10, category_id=1, bbox=[1, 1, 5, 5], area=25, iscrowd=0)])
    return evaluation.COCOEvaluator(None, {0: 3, 1: 1}, annotations=ann, **kw)          # label 0 -> index 1, label 1 -> index 0


def tt_evaluator(n_images=3, **kw):
    ann = dict(imgs=dict((str(10 * (i + 1)), dict(objects=[dict(bbox=dict(xmin=1, ymin=1, xmax=9, ymax=9), category='b')]))
                         for i in range(n_images)))
    return evaluation.TT100KEvaluator(annotations=ann, label_indexes_to_category_names=['a', 'b'], types=None, **kw)


def wf_evaluator(n_images=3, **kw):
    ann = [dict(id=10 * (i + 1), event='0--E', stem='0_E_%d' % i, boxes=np.array([[1.0, 1.0, 8.0, 8.0]]), keep=dict(easy=[0], medium=[0], hard=[0]))
           for i in range(n_images)]
    return evaluation.WIDERFACEEvaluator(annotations=ann, **kw)


def meta_of(image_ids):
    return [dict(image_id=i) for i in image_ids]


def read_store(ev, n=None):
    d = ev._dev
    state = d.state.cpu().numpy()
    n = int(state[0]) if n is None else n
    out = dict(state=state, box=d.det_box[:n].cpu().numpy(), score=d.det_score[:n].cpu().numpy(), img=d.det_img[:n].cpu().numpy())
    if getattr(d, 'det_cat', None) is not None:
        out['cat'] = d.det_cat[:n].cpu().numpy()
        out['mask'] = d.img_mask.cpu().numpy()
    return out


def check_store(got, want, label):
    want = dict(want, box=np.array(want['box'], F64).reshape(-1, 4), score=np.array(want['score'], F64))
    assert got['state'].tolist() == want['state'], (label, got['state'])
    for k in ('box', 'score'):
        assert got[k].dtype == F64 and got[k].shape == want[k].shape, (label, k)
        assert got[k].tobytes() == want[k].tobytes(), (label, k, got[k], want[k])
    for k in ('img', 'cat', 'mask'):
        assert (k in want) == (k in got), (label, k)
        if k in want:
            assert got[k].dtype == np.int32 and got[k].tolist() == list(want[k]), (label, k, got[k])


# ------------------------------------------------------------------------------------------------ what one row becomes
@pytest.mark.parametrize('all_images', [False, True])
@pytest.mark.parametrize('path', ['update', 'update_resident'])
def test_store_contents_coco(path, all_images):
    ev = coco_evaluator(all_images=all_images)
    cat_of = {0: 1, 1: 0}
    if path == 'update':
        with pytest.raises(KeyError):
            ev.update((list_rows(LABELS), meta_of(IMAGE_IDS)))                  # the unmapped label never reaches the device
        ev.update((list_rows(LABELS, skip=(UNMAPPED,)), meta_of(IMAGE_IDS)))
        use = [(i, j) for i, j in kept() if LABELS[i, j] != UNMAPPED]
        err = 0
    else:
        ev.update_resident(outputs_of(DETS, LABELS, COUNTS), meta_of(IMAGE_IDS))
        use, err = kept(), ERR_LABEL
    want = dict(state=[len(use), err, 0, 0], box=[], score=[], img=[ORDS[i] for i, j in use],
                cat=[cat_of.get(int(LABELS[i, j]), -1) for i, j in use],
                mask=[int(all_images), 1, 1])                                   # ordinal 0 kept nothing: marked only with all_images
    for i, j in use:
        d = DETS[i, j]
        w, h = wh32(d)
        want['box'].append([F64(d[0]), F64(d[1]), F64(w), F64(h)])              # {x, y, w, h}
        want['score'].append(F64(d[4]))                                         # as is
    check_store(read_store(ev), want, 'coco %s' % path)
    ev._clear()
    assert ev._dev.state.tolist() == [0, 0, 0, 0] and not ev._dev.img_mask.any()


@pytest.mark.parametrize('path', ['update', 'update_resident'])
def test_store_contents_tt100k(path):
    ev = tt_evaluator()
    if path == 'update':
        with pytest.raises(ValueError, match='no category name'):
            ev.update((list_rows(LABELS), meta_of(['30', '10', '20'])))
        ev.update((list_rows(LABELS, skip=(UNMAPPED,)), meta_of(IMAGE_IDS)))    # ids are compared as strings
        use = [(i, j) for i, j in kept() if LABELS[i, j] != UNMAPPED]
        err = 0
    else:
        ev.update_resident(outputs_of(DETS, LABELS, COUNTS), meta_of(IMAGE_IDS))
        use, err = kept(), ERR_LABEL
    want = dict(state=[len(use), err, 0, 0], box=[], score=[], img=[ORDS[i] for i, j in use],
                cat=[{0: 0, 1: 1}.get(int(LABELS[i, j]), -1) for i, j in use], mask=[1, 1, 1])       # every image passed is marked
    for i, j in use:
        d = DETS[i, j]
        w, h = wh32(d)
        want['box'].append([F64(d[0]), F64(d[1]), F64(w) + F64(d[0]), F64(h) + F64(d[1])])       # xmax = w + x in float64 from the fp32 w
        want['score'].append(F64(d[4]) * 100.0)
    check_store(read_store(ev), want, 'tt100k %s' % path)
    ev._clear()
    assert ev._dev.state.tolist() == [0, 0, 0, 0] and not ev._dev.img_mask.any()


@pytest.mark.parametrize('as_written', [False, True])
@pytest.mark.parametrize('path', ['update', 'update_resident'])
def test_store_contents_widerface(path, as_written):
    ev = wf_evaluator(as_written=as_written, label_index=0)
    if path == 'update':
        ev.update((list_rows(WF_LABELS), meta_of(IMAGE_IDS)))
    else:
        ev.update_resident(outputs_of(DETS, WF_LABELS, COUNTS), meta_of(IMAGE_IDS))
    want = dict(box=[], score=[], img=[])
    for i in range(3):
        if as_written:                                                          # the dummy row, also for the image that kept nothing
            want['box'].append([0.0, 0.0, 0.0, 0.0])
            want['score'].append(0.001)
            want['img'].append(ORDS[i])
        for j in range(int(COUNTS[i, 1])):
            take = WF_LABELS[i, j] == 0
            if path == 'update' and not take:
                continue                                                        # the list path drops the row on the host
            d = DETS[i, j]
            w, h = wh32(d)
            x, y, w, h, s = F64(d[0]), F64(d[1]), F64(w), F64(h), F64(d[4])
            if as_written:
                x, y, w, h, s = np.floor(x), np.floor(y), np.ceil(w), np.ceil(h), F64(float('%.03f' % min(float(s), 1)))
            want['box'].append([x, y, w, h])
            want['score'].append(s)
            want['img'].append(ORDS[i] if take else -1)                         # the resident path keeps the slot
    want['state'] = [len(want['img']), 0, 0, 0]
    assert len(want['img']) == 6 + 3 * int(as_written) - int(path == 'update')
    check_store(read_store(ev), want, 'widerface %s as_written %s' % (path, as_written))
    ev._clear()
    assert ev._dev.state.tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ the entry points, directly
SENT_IMG, SENT_CAT, SENT_F = 777, 555, -5.0


class Direct(object):
    """an evaluator's device state with the store pre-filled by sentinels, and its C entry points"""

    def __init__(self, kind, **kw):
        self.kind = kind
        self.ev = dict(coco=coco_evaluator, tt=tt_evaluator, wf=wf_evaluator)[kind](**kw)
        self.d = self.ev._state()
        self.lib, self.l = self.d.lib, self.d.lib.lib()
        self.desc, self.bufs = self.ev._desc(), self.ev._bufs()
        self.keep = []
        self.reset()

    def dev(self, a, dtype):
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()
        self.keep.append(t)
        return t

    def dets(self, ords, dets=DETS, labels=LABELS, counts=COUNTS):
        o = outputs_of(dets, labels, counts)
        self.keep.append(o)
        n, cap = int(o.dets.size(0)), int(o.dets.size(1))
        p, head = self.lib.ptr, (C.byref(self.desc), C.byref(self.bufs), self.lib.ptr(o.dets), self.lib.ptr(o.labels), self.lib.ptr(o.counts), n, cap)
        ords_t = self.dev(ords, np.int32)
        if self.kind == 'coco':
            st = self.l.lfd_eval_append_dets_f32(*head, p(self.d.label_map), int(self.d.label_map.numel()), p(ords_t), 0, self.lib.stream_ptr())
        elif self.kind == 'tt':
            st = self.l.lfd_eval_tt100k_append_dets_f32(*head, p(self.d.label_map), int(self.d.label_map.numel()), p(ords_t), self.lib.stream_ptr())
        else:
            st = self.l.lfd_eval_wf_append_dets_f32(*head, p(ords_t), self.lib.stream_ptr())
        assert st == 0

    def rows(self, rows, mark=()):
        cols = 6 if self.kind == 'wf' else 7
        rows_t = self.dev(np.array(rows, F64).reshape(-1, cols), F64) if len(rows) else None
        head = (C.byref(self.desc), C.byref(self.bufs), self.lib.ptr(rows_t), len(rows))
        if self.kind == 'wf':
            st = self.l.lfd_eval_wf_append_rows_f64(*head, self.lib.stream_ptr())
        else:
            mark_t = self.dev(mark, np.int32) if len(mark) else None
            fn = self.l.lfd_eval_append_rows_f64 if self.kind == 'coco' else self.l.lfd_eval_tt100k_append_rows_f64
            st = fn(*head, self.lib.ptr(mark_t), len(mark), self.lib.stream_ptr())
        assert st == 0

    def reset(self):
        self.d.state.zero_()
        self.d.det_box.fill_(SENT_F)
        self.d.det_score.fill_(SENT_F)
        self.d.det_img.fill_(SENT_IMG)
        if self.kind != 'wf':
            self.d.det_cat.fill_(SENT_CAT)
            self.d.img_mask.zero_()


BAD = [-1, 3, 1]                               # ordinals of the batch entries: below the range, num_images, a good one


@pytest.mark.parametrize('kind', ['coco', 'tt'])
def test_bad_ordinals_in_append_dets_coco_and_tt100k(kind):
    """ERR_IMAGE; the entry writes nothing, but the commit counts its slots"""
    x = Direct(kind)
    x.dets(BAD)
    got = read_store(x.ev)
    assert got['state'].tolist() == [6, ERR_IMAGE | ERR_LABEL, 0, 0]            # the unmapped label sits in the good entry
    assert got['img'].tolist() == [SENT_IMG] * 2 + [1] * 4 and got['cat'][:2].tolist() == [SENT_CAT] * 2
    assert (got['score'][:2] == SENT_F).all() and (got['box'][:2] == SENT_F).all() and (got['score'][2:] != SENT_F).all()
    assert got['mask'].tolist() == [0, 1, 0]
    x.reset()
    x.dets([0, 1, 3])                                                           # the bad entry last: what comes before is whole
    got = read_store(x.ev)
    assert got['state'].tolist() == [6, ERR_IMAGE, 0, 0]
    assert got['img'].tolist() == [0, 0] + [SENT_IMG] * 4
    assert got['mask'].tolist() == [1, int(kind == 'tt'), 0]                    # COCO (mark_all 0) marks an image that kept something


@pytest.mark.parametrize('as_written', [False, True])
def test_bad_ordinals_in_append_dets_widerface(as_written):
    """ERR_IMAGE; the entry's slots (the dummy row included) become det_img -1, det_score 0 and keep the box that was there"""
    x = Direct('wf', as_written=as_written)
    e = int(as_written)
    x.dets(BAD, labels=WF_LABELS)
    got = read_store(x.ev)
    assert got['state'].tolist() == [6 + 3 * e, ERR_IMAGE, 0, 0]
    n_bad = 2 + 2 * e                                                           # entry 0: two boxes; entry 1: none; a dummy row each
    assert got['img'].tolist() == [-1] * n_bad + [1] * (4 + e)
    assert (got['score'][:n_bad] == 0.0).all() and (got['box'][:n_bad] == SENT_F).all()
    assert (got['box'][n_bad:] != SENT_F).all() and (got['score'][n_bad:] > 0).all()


def row7(o, c, s=0.5, box=(1.0, 2.0, 3.0, 4.0)):
    return [o, c, s] + list(box)


def test_bad_ordinals_and_categories_in_append_rows_coco():
    x = Direct('coco')
    x.rows([row7(1, 2), row7(1, -1)])                                           # a category out of range: -1, silently
    got = read_store(x.ev)
    assert got['state'].tolist() == [2, 0, 0, 0] and got['cat'].tolist() == [-1, -1] and got['img'].tolist() == [1, 1]
    x.reset()
    x.rows([row7(-1, 1), row7(3, 0), row7(2, 1, 0.25)], mark=[1])
    got = read_store(x.ev)
    assert got['state'].tolist() == [3, ERR_IMAGE, 0, 0]
    assert got['img'].tolist() == [0, 0, 2] and got['cat'].tolist() == [-1, -1, 1]       # ordinal 0, category -1
    assert got['score'].tolist() == [0.5, 0.5, 0.25] and (got['box'] == [1.0, 2.0, 3.0, 4.0]).all()
    assert got['mask'].tolist() == [0, 1, 1]                                    # image 0 was named by no good row
    x.reset()
    x.rows([], mark=[-1, 0, 3])
    got = read_store(x.ev)
    assert got['state'].tolist() == [0, ERR_IMAGE, 0, 0] and got['mask'].tolist() == [1, 0, 0]


def test_bad_ordinals_and_categories_in_append_rows_tt100k():
    x = Direct('tt')
    K = len(x.ev.category_names)
    x.rows([row7(1, K), row7(1, -1)])                                           # a category out of range: -1 and ERR_LABEL
    got = read_store(x.ev)
    assert got['state'].tolist() == [2, ERR_LABEL, 0, 0] and got['cat'].tolist() == [-1, -1] and got['img'].tolist() == [1, 1]
    x.reset()
    x.rows([row7(-1, 1), row7(3, 0), row7(2, 1, 0.25)], mark=[1])
    got = read_store(x.ev)
    assert got['state'].tolist() == [3, ERR_IMAGE | ERR_LABEL, 0, 0]            # the bad ordinal's category -1 fails the category test too
    assert got['img'].tolist() == [-1, -1, 2] and got['cat'].tolist() == [-1, -1, 1]
    assert got['score'].tolist() == [50.0, 50.0, 25.0] and (got['box'] == [1.0, 2.0, 4.0, 6.0]).all()
    assert got['mask'].tolist() == [0, 1, 1]
    x.reset()
    x.rows([], mark=[-1, 0, 3])
    got = read_store(x.ev)
    assert got['state'].tolist() == [0, ERR_IMAGE, 0, 0] and got['mask'].tolist() == [1, 0, 0]


def test_bad_ordinals_in_append_rows_widerface():
    x = Direct('wf')
    x.rows([[-1, 0.5, 1.0, 2.0, 3.0, 4.0], [3, 0.5, 1.0, 2.0, 3.0, 4.0], [2, 0.25, 1.0, 2.0, 3.0, 4.0]])
    got = read_store(x.ev)
    assert got['state'].tolist() == [3, ERR_IMAGE, 0, 0] and got['img'].tolist() == [-1, -1, 2]
    assert got['score'].tolist() == [0.5, 0.5, 0.25] and (got['box'] == [1.0, 2.0, 3.0, 4.0]).all()


@pytest.mark.parametrize('kind', ['coco', 'tt', 'wf', 'wf_as_written'])
def test_capacity_overflow_leaves_the_count_and_sets_the_error_bit(kind):
    """det_capacity one short of what the append needs, on both entry points, after an append that fitted"""
    as_written = kind == 'wf_as_written'
    x = Direct('wf', as_written=as_written) if kind.startswith('wf') else Direct(kind)
    wf = x.kind == 'wf'
    first = [[2, 0.5, 1.0, 2.0, 3.0, 4.0]] if wf else [row7(2, 0)]
    three = [[0, 0.5, 1.0, 2.0, 3.0, 4.0]] * 3 if wf else [row7(0, 0)] * 3
    # rows: 1 stored, 3 offered, room for 3
    x.desc.det_capacity = 3
    x.rows(first)
    assert x.d.state.tolist() == [1, 0, 0, 0]
    x.rows(three, mark=() if wf else [1])
    got = read_store(x.ev, 4)
    assert got['state'].tolist() == [1, ERR_CAPACITY, 0, 0]
    assert got['img'].tolist() == [2] + [SENT_IMG] * 3                          # nothing was written
    if not wf:
        assert got['mask'].tolist() == [0, 1, 1]                                # the marks were processed, the rows' images were not
    # dets: 1 stored, 6 boxes (and three dummy rows) offered, room for one less
    x.d.state.zero_()
    need = 1 + 6 + 3 * int(as_written)
    x.desc.det_capacity = need - 1
    x.rows(first)
    if not wf:
        x.d.img_mask.zero_()
    x.dets([0, 1, 2], labels=WF_LABELS if wf else LABELS)                       # entries of 2, 0 and 4 boxes: only the last does not fit
    got = read_store(x.ev, need)
    assert got['state'].tolist()[0] == 1 and got['state'][1] & ERR_CAPACITY and not got['state'][1] & ERR_IMAGE
    assert got['img'][-4:].tolist() == [SENT_IMG] * 4                           # the entry that does not fit wrote nothing
    if x.kind == 'coco':
        assert got['mask'].tolist() == [1, 0, 0]                                # marked after the capacity test, and only with boxes
    if x.kind == 'tt':
        assert got['mask'].tolist() == [1, 1, 1]                                # marked before it
    x.desc.det_capacity = need
    x.d.state[1] = 0
    x.dets([0, 1, 2], labels=WF_LABELS if wf else LABELS)
    assert x.d.state.tolist()[0] == need and not x.d.state.tolist()[1] & ERR_CAPACITY


# ------------------------------------------------------------------------------------------------ grouping at the scan's edges
def scattered(num_images, seed):
    """[(image ordinal, number of detections 1 or 2)] in feeding order: a scattered subset that holds the first and the last
    image, shuffled so that the store is not in image order"""
    rng = np.random.RandomState(seed)
    if num_images == 1:
        return [(0, 2)]
    pick = set(rng.choice(num_images, 40, replace=False).tolist()) | {0, 1, num_images - 2, num_images - 1}
    pick = [int(v) for v in rng.permutation(sorted(pick))]
    return [(o, 1 + int(rng.randint(0, 2))) for o in pick]


def feed_scattered(ev, plan, image_id_of, rows_per_image_extra=0):
    """feeds the plan in batches of 7, every third batch through update_resident; -> store indices per image ordinal"""
    members, at = dict(), 0
    for b0 in range(0, len(plan), 7):
        batch = plan[b0:b0 + 7]
        dets = np.full((len(batch), 2, 5), 12345.0, F32)
        labels = np.zeros((len(batch), 2), np.int32)
        counts = np.zeros((len(batch), 4), np.int32)
        for i, (o, k) in enumerate(batch):
            counts[i, 1] = k
            for j in range(k):
                dets[i, j] = [2.0, 2.0, 8.0 + j, 8.0, 0.5 + 0.25 * j]
            at += rows_per_image_extra
            members[o] = list(range(at, at + k))
            at += k
        meta = meta_of([image_id_of(o) for o, k in batch])
        if (b0 // 7) % 3 == 2:
            ev.update_resident(outputs_of(dets, labels, counts), meta)
        else:
            rows = [[[0, float(d[4]), float(d[0]), float(d[1]), float(d[2] - d[0] + 1), float(d[3] - d[1] + 1)] for d in dets[i, :k]]
                    for i, (o, k) in enumerate(batch)]
            ev.update((rows, meta))
    return members


def expected_grouping(members, num_images):
    cnt = np.array([len(members.get(o, ())) for o in range(num_images)], np.int64)
    return np.concatenate([[0], np.cumsum(cnt)]), [members.get(o, []) for o in range(num_images)]


@pytest.mark.parametrize('num_images', [1, 1025])
def test_grouping_by_image_tt100k(num_images):
    ev = tt_evaluator(num_images)
    members = feed_scattered(ev, scattered(num_images, 3), lambda o: str(10 * (o + 1)))
    ev.evaluate(keep_matches=True)
    tab = ev.match_table()
    start, per_image = expected_grouping(members, num_images)
    assert tab['det_start'].shape == (num_images + 1,) and np.array_equal(tab['det_start'], start)
    assert tab['index'].tolist() == [s for m in per_image for s in m]           # insertion order inside every image
    assert int(ev.num_detections[0, 0, 0]) == 0 and int(ev.num_ground_truth[0, 0, 0]) == len(members)      # minscore 90 > every score


@pytest.mark.parametrize('as_written', [False, True])
@pytest.mark.parametrize('num_images', [1, 1025])
def test_grouping_by_image_widerface(num_images, as_written):
    ev = wf_evaluator(num_images, as_written=as_written)
    members = feed_scattered(ev, scattered(num_images, 4), lambda o: 10 * (o + 1), rows_per_image_extra=int(as_written))
    if as_written:
        members = dict((o, [m[0] - 1] + m) for o, m in members.items())         # the dummy row belongs to the image
    ev.evaluate(keep_matches=True)
    start, per_image = expected_grouping(members, num_images)
    assert ev._last['det_start'].shape == (num_images + 1,) and np.array_equal(ev._last['det_start'], start)
    tab = ev.match_table(0)                                                     # every image has ground truth: all are ranked
    assert np.array_equal(tab['image'], np.repeat(np.arange(num_images), np.diff(start)))
    for o in range(num_images):
        assert sorted(tab['index'][start[o]:start[o + 1]].tolist()) == per_image[o], o       # rank order: a permutation
    assert int(ev.faces[0]) == num_images


def test_grouping_by_pair_coco_with_1025_pairs():
    I, K = 205, 5
    rng = np.random.RandomState(5)
    image_ids, cat_ids = [3 * i + 1 for i in range(I)], [2 * k + 1 for k in range(K)]
    pairs = set(rng.choice(I * K, 60, replace=False).tolist()) | {0, 1, I * K - 2, I * K - 1}
    gts = [dict(id=n + 1, image_id=image_ids[p // K], category_id=cat_ids[p % K], bbox=[2.0, 2.0, 7.0, 7.0], area=49.0, iscrowd=0)
           for n, p in enumerate(sorted(rng.choice(I * K, 50, replace=False).tolist()))]
    ev = evaluation.COCOEvaluator(None, dict((k, cat_ids[k]) for k in range(K)), annotations=dict(
        images=[dict(id=i) for i in image_ids], categories=[dict(id=c) for c in cat_ids], annotations=gts))
    by_image = dict()
    for p in pairs:
        for j in range(1 + int(rng.randint(0, 2))):
            by_image.setdefault(p // K, []).append([p % K, float(rng.randint(1, 5)) / 4.0, 2.0, 2.0, 7.0 + j, 7.0])
    order = [int(v) for v in rng.permutation(sorted(by_image))]
    dts = []
    for b0 in range(0, len(order), 7):
        batch = order[b0:b0 + 7]
        ev.update(([by_image[o] for o in batch], meta_of([image_ids[o] for o in batch])))
        dts += [dict(image_id=image_ids[o], category_id=cat_ids[r[0]], score=r[1], bbox=r[2:]) for o in batch for r in by_image[o]]
    ref = coco_eval_oracle.evaluate(gts, dts, [image_ids[o] for o in order], cat_ids)
    ev.evaluate(keep_matches=True)
    want = [idx for key in sorted(ref['matches']) for idx in ref['matches'][key]['index']]       # pair-major, rank order inside a pair
    assert len(want) == len(dts) and sorted(want) == list(range(len(dts)))
    assert ev.match_table()['index'].tolist() == want
