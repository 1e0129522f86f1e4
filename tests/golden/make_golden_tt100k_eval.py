"""tests/golden/make_golden_tt100k_eval.py -- ref_tt100k_eval.npz: seeded synthetic TT100K annotation / detection sets scored by
the reference's own TT100K_train/official_eval.eval_annos (build container only: needs the reference checkout, LFD_REFERENCE or
/root/reference).  official_eval.py is loaded by path with empty stand-ins for `pylab` and `cv2` (only its drawing helpers
use them); nothing of it is copied here, the fixture holds data only.

    python tests/golden/make_golden_tt100k_eval.py            # writes the fixture (LFD_GOLDEN_OUT or this directory)
    python tests/golden/make_golden_tt100k_eval.py --check    # regenerates and compares with the committed file

The detections reach the reference through the reference's own arithmetic: fp32 [x1, y1, x2, y2, score] rows become
[label, score, x, y, w, h] with torch fp32 `x2 - x1 + 1` on the CPU and .tolist() (LFD.get_results), then the dictionary of
TT100K_train/evaluation.py:42-55 (score * 100, xmax = w + x).

What is recorded per group of runs (one group = one setting of types / check_type / match_same, all combinations of its
iou x minscore x size range lists): the integers right = len(right), counted detections = len(right) + len(wrong), counted
ground truth = len(miss) + the matched detections that were not erased (every such detection has exactly one counted ground
truth and the other way round); accuracy, recall and the report string as returned; per detection an outcome code and per
ground truth whether it was missed, recovered by tagging every object with a unique key.  The generator asserts that the
integers reproduce the returned ratios, and that every situation the tests rely on really occurs."""
import importlib.util
import json
import os
import sys
import types as pytypes

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import tt100k_eval_oracle as oracle   # noqa: E402  (only iou_matrix / long_side, for the assertions on the inputs)

OUT_NAME = 'ref_tt100k_eval.npz'
OTHER = ['zz_other1', 'zz_other2']       # labels 45, 46: names outside type45
GT_ONLY = 'zz_gtonly'                    # an annotation category no label maps to
NO_TYPE = '<no such type>'


def load_reference():
    root = os.environ.get('LFD_REFERENCE', '/root/reference')
    path = os.path.join(root, 'TT100K_train', 'official_eval.py')
    assert os.path.isfile(path), 'the reference checkout is needed (%s)' % path
    for name in ('pylab', 'cv2'):
        sys.modules.setdefault(name, pytypes.ModuleType(name))
    spec = importlib.util.spec_from_file_location('official_eval', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build_images(names, seed=20261016):
    """-> list of dict(id, gts=[(xmin, ymin, xmax, ymax, name)], dets=[(x1, y1, x2, y2, score, label)])"""
    rng = np.random.RandomState(seed)
    L = dict((n, i) for i, n in enumerate(names))

    def copy_of(g, score, name=None, dx=0.0):     # the detection whose results box is exactly g (integer coordinates)
        return (g[0] + dx, g[1], g[2] - 1 + dx, g[3] - 1, score, L[name or g[4]])
    images = []
    # exact IoU ties: duplicated ground truth, duplicated detections, mirrored shifts
    g = [(100, 100, 200, 200, 'pl40'), (100, 100, 200, 200, 'pn'), (300, 100, 400, 200, 'pl40'), (500, 100, 600, 200, 'p5'),
         (700, 100, 800, 200, 'il60'), (700, 100, 800, 200, 'il60')]
    d = [copy_of(g[0], 0.98), copy_of(g[2], 0.97, 'pn'), copy_of(g[2], 0.96), copy_of(g[3], 0.95, dx=10.0),
         copy_of(g[3], 0.99, dx=-10.0), copy_of(g[4], 0.94)]
    images.append(dict(id='70001', gts=g, dets=d))
    # a better-IoU pair steals a detection that a score-ordered matcher would give elsewhere
    g = [(0, 100, 100, 200, 'w57'), (40, 100, 140, 200, 'w57')]
    d = [(15, 100, 114, 199, 0.99, L['w57']), (0, 100, 104, 199, 0.91, L['w57'])]
    images.append(dict(id='70002', gts=g, dets=d))
    # box sizes exactly at 32 / 96 / 400 and just below
    g = [(0, 0, 32, 20, 'pl50'), (100, 0, 196, 50, 'pl50'), (0, 300, 400, 350, 'pl50'), (300, 0, 331.5, 20, 'pl50'),
         (500, 0, 595.999, 50, 'pl50')]
    d = [copy_of(x, 0.95) for x in g[:3]] + [(300, 0, 330.5, 19, 0.95, L['pl50']), (500, 0, 594.999, 49, 0.95, L['pl50'])]
    d += [(0, 500, 31, 510, 0.96, L['i5']), (100, 500, 195, 510, 0.96, L['i5']), (0, 600, 399, 610, 0.96, L['i5'])]
    images.append(dict(id='70003', gts=g, dets=d))
    # a matched pair whose ground truth is outside the band (32, 96) while the detection is inside, and the converse
    g = [(100, 100, 200, 200, 'ph5'), (400, 100, 490, 190, 'ph5')]
    d = [(105, 105, 194, 194, 0.93, L['ph5']), (395, 95, 494, 194, 0.93, L['ph5'])]
    images.append(dict(id='70004', gts=g, dets=d))
    # categories outside type45
    g = [(10, 10, 60, 60, GT_ONLY), (100, 10, 150, 60, OTHER[0]), (200, 10, 250, 60, 'i2')]
    d = [(10, 10, 59, 59, 0.94, L['i2']), (100, 10, 149, 59, 0.9, L[OTHER[0]]), (200, 10, 249, 59, 0.97, L[OTHER[1]])]
    images.append(dict(id='70005', gts=g, dets=d))
    # scores exactly at 50 and 75; fp32 0.9 * 100 is below 90
    g = [(10 + 150 * k, 10, 110 + 150 * k, 110, 'pne') for k in range(4)]
    d = [copy_of(g[0], 0.5), copy_of(g[1], 0.75), copy_of(g[2], 0.9), copy_of(g[3], 0.90625)]
    images.append(dict(id='70006', gts=g, dets=d))
    images.append(dict(id='70007', gts=[], dets=[(5, 5, 50, 50, 0.99, L['io']), (200, 200, 260, 240, 0.6, L['ip']),
                                                  (300, 300, 320, 330, 0.92, L[OTHER[0]])]))
    images.append(dict(id='70008', gts=[(50, 50, 120, 130, 'wo'), (300, 300, 340, 420, 'w13')], dets=[]))
    images.append(dict(id='70009', gts=[], dets=[]))
    # zero-area detections (never a zero-area ground truth next to one: the reference divides 0 by 0 there)
    images.append(dict(id='70010', gts=[(50, 50, 100, 100, 'io')],
                       dets=[(60, 60, 59, 90, 0.95, L['io']), (70, 70, 69, 69, 0.95, L['io']), (50, 50, 99, 99, 0.96, L['io'])]))
    # more than 64 ground-truth boxes and more than 1024 detections in one image
    pool = ['pl40', 'pl50', 'pn', 'p5', 'w57']
    g, d = [], []
    for r in range(8):
        for c in range(10):
            s = int(rng.randint(20, 61))
            g.append((100 * c + 10, 100 * r + 10, 100 * c + 10 + s, 100 * r + 10 + int(rng.randint(20, 61)), pool[int(rng.randint(5))]))
    for x in g:
        for _ in range(int(rng.randint(4, 9))):
            j = rng.randint(-3, 4, 4)
            name = x[4] if rng.rand() < 0.85 else pool[int(rng.randint(5))]
            d.append((x[0] + j[0], x[1] + j[1], x[2] - 1 + j[2], x[3] - 1 + j[3], round(float(rng.uniform(0.3, 1.0)), 2), L[name]))
    while len(d) < 1200:
        x, y = rng.randint(0, 1000), rng.randint(0, 800)
        d.append((x, y, x + int(rng.randint(5, 80)), y + int(rng.randint(5, 80)), round(float(rng.uniform(0.3, 1.0)), 2),
                  L[pool[int(rng.randint(5))]]))
    order = rng.permutation(len(d))
    images.append(dict(id='70011', gts=g, dets=[d[i] for i in order]))
    # random images: float coordinates, sizes over all bands, jittered copies, exact duplicates, false positives
    pool = ['i2', 'i4', 'pl100', 'pm20', 'w32', 'wo', OTHER[0], GT_ONLY]
    for n in range(40):
        g, d = [], []
        for _ in range(int(rng.randint(0, 9))):
            w, h = np.exp(rng.uniform(np.log(10), np.log(450), 2))
            x, y = rng.uniform(0, 1500), rng.uniform(0, 1500)
            g.append((float(x), float(y), float(x + w), float(y + h), pool[int(rng.randint(len(pool)))]))
        for x in g:
            for _ in range(int(rng.randint(0, 4))):
                w, h = x[2] - x[0], x[3] - x[1]
                j = rng.normal(0, 0.07, 4) * [w, h, w, h]
                name = x[4] if (x[4] != GT_ONLY and rng.rand() < 0.8) else pool[int(rng.randint(len(pool) - 1))]
                d.append((x[0] + j[0], x[1] + j[1], x[2] + j[2], x[3] + j[3], float(rng.choice([0.5, 0.75, 0.8, 0.9, 0.95, 0.99])), L[name]))
                if rng.rand() < 0.25:
                    d.append(d[-1][:4] + (round(float(rng.uniform(0.4, 1.0)), 2), d[-1][5]))
        for _ in range(int(rng.randint(0, 6))):
            w, h = np.exp(rng.uniform(np.log(10), np.log(450), 2))
            x, y = rng.uniform(0, 1500), rng.uniform(0, 1500)
            d.append((x, y, x + w, y + h, round(float(rng.uniform(0.3, 1.0)), 2), L[pool[int(rng.randint(len(pool) - 1))]]))
        order = rng.permutation(len(d))
        images.append(dict(id=str(10000 + 37 * n), gts=g, dets=[d[i] for i in order]))
    return images


def to_arrays(images, names):
    cat_names = list(names) + [GT_ONLY]
    C = dict((n, i) for i, n in enumerate(cat_names))
    gt_box = np.array([x[:4] for im in images for x in im['gts']], np.float64).reshape(-1, 4)
    gt_cat = np.array([C[x[4]] for im in images for x in im['gts']], np.int32)
    gt_img = np.array([i for i, im in enumerate(images) for _ in im['gts']], np.int32)
    det = np.array([x[:5] for im in images for x in im['dets']], np.float32).reshape(-1, 5)
    det_label = np.array([x[5] for im in images for x in im['dets']], np.int32)
    det_img = np.array([i for i, im in enumerate(images) for _ in im['dets']], np.int32)
    return dict(names=np.array(names), cat_names=np.array(cat_names), image_ids=np.array([im['id'] for im in images]),
                gt_box=gt_box, gt_cat=gt_cat, gt_img=gt_img, det=det, det_label=det_label, det_img=det_img)


def rows_of(det_f32, labels):
    """LFD.get_results' rows from fp32 detections: torch fp32 arithmetic on the CPU, then .tolist()"""
    import torch
    if len(labels) == 0:
        return []
    d = torch.from_numpy(np.ascontiguousarray(det_f32)).clone()
    d[:, 2] = d[:, 2] - d[:, 0] + 1
    d[:, 3] = d[:, 3] - d[:, 1] + 1
    rows = torch.cat([torch.from_numpy(labels.astype(np.float32))[:, None], d[:, [4, 0, 1, 2, 3]]], dim=1).tolist()
    return [[int(r[0])] + r[1:] for r in rows]


def results_dict(arr, with_keys):
    """the results dictionary of TT100K_train/evaluation.py:42-57 for every image"""
    names = [str(n) for n in arr['names']]
    out = dict(imgs=dict())
    for i, iid in enumerate(arr['image_ids']):
        sel = np.nonzero(arr['det_img'] == i)[0]
        temp = dict(id=str(iid), objects=list())
        for k, result in zip(sel, rows_of(arr['det'][sel], arr['det_label'][sel])):
            obj = dict(bbox={'xmin': result[2], 'ymin': result[3], 'xmax': result[4] + result[2], 'ymax': result[5] + result[3]},
                       category=names[result[0]], score=result[1] * 100)
            if with_keys:
                obj['key'] = int(k)
            temp['objects'].append(obj)
        out['imgs'][str(iid)] = temp
    return out


def annotations_dict(arr, with_keys):
    cats = [str(n) for n in arr['cat_names']]
    out = dict(imgs=dict(), types=cats)
    for i, iid in enumerate(arr['image_ids']):
        objs = []
        for k in np.nonzero(arr['gt_img'] == i)[0]:
            b = arr['gt_box'][k]
            obj = dict(bbox=dict(xmin=float(b[0]), ymin=float(b[1]), xmax=float(b[2]), ymax=float(b[3])), category=cats[arr['gt_cat'][k]])
            if with_keys:
                obj['key'] = int(k)
            objs.append(obj)
        out['imgs'][str(iid)] = dict(id=str(iid), path='test/%s.jpg' % iid, objects=objs)
    return out


def groups_of(type45):
    bands = [[0, 400], [0, 32], [32, 96], [96, 400]]
    gs = [dict(types=list(type45), check_type=True, match_same=True, ious=[0.5, 0.75], minscores=[50, 75, 90], size_ranges=bands),
          dict(types=list(type45), check_type=True, match_same=False, ious=[0.5], minscores=[50], size_ranges=[[0, 400], [32, 96]]),
          dict(types=list(type45), check_type=False, match_same=False, ious=[0.5], minscores=[50], size_ranges=[[0, 400], [32, 96]]),
          dict(types=None, check_type=True, match_same=True, ious=[0.5], minscores=[50, 90], size_ranges=[[0, 400]]),
          dict(types=None, check_type=True, match_same=False, ious=[0.5, 0.3], minscores=[50], size_ranges=[[0, 400], [32.0, 96.5]])]
    for name in ('pl40', 'p5', 'w57', 'pl50', OTHER[0]):     # per-category counts: one name and one that matches nothing
        gs.append(dict(types=[name, NO_TYPE], check_type=True, match_same=True, ious=[0.5], minscores=[50], size_ranges=[[0, 400], [32, 96]]))
    return gs


def run_group(ref, gd, rt, grp, D, G):
    T, M, S = len(grp['ious']), len(grp['minscores']), len(grp['size_ranges'])
    out = dict(right=np.zeros((T, M, S), np.int64), num_detections=np.zeros((T, M, S), np.int64),
               num_ground_truth=np.zeros((T, M, S), np.int64), accuracy=np.zeros((T, M, S)), recall=np.zeros((T, M, S)),
               det_code=np.zeros((T, M, S, D), np.uint8), gt_missed=np.zeros((T, M, S, G), bool), report=np.zeros((T, M, S), 'U200'))
    for t, iou in enumerate(grp['ious']):
        for m, minscore in enumerate(grp['minscores']):
            for s, (lo, hi) in enumerate(grp['size_ranges']):
                r = ref.eval_annos(annos_gd=gd, annos_rt=rt, iou=iou, imgids=None, check_type=grp['check_type'], types=grp['types'],
                                   minscore=minscore, minboxsize=lo, maxboxsize=hi, match_same=grp['match_same'])
                right = wrong = matched_wrong = miss = 0
                for iid in rt['imgs']:
                    for o in r['right']['imgs'][iid]['objects']:
                        out['det_code'][t, m, s, o['key']] = oracle.DET_RIGHT
                        right += 1
                    for o in r['wrong']['imgs'][iid]['objects']:
                        none = o['correct_catelog'] == 'none'
                        out['det_code'][t, m, s, o['key']] = oracle.DET_UNMATCHED if none else oracle.DET_WRONG
                        wrong += 1
                        matched_wrong += 0 if none else 1
                    for o in r['miss']['imgs'][iid]['objects']:
                        out['gt_missed'][t, m, s, o['key']] = True
                        miss += 1
                ac_n, rc_n = right + wrong, miss + right + matched_wrong
                assert r['accuracy'] == (1 if ac_n == 0 else right * 1.0 / ac_n), (grp, t, m, s)
                assert r['recall'] == (1 if rc_n == 0 else right * 1.0 / rc_n), (grp, t, m, s)
                out['right'][t, m, s], out['num_detections'][t, m, s], out['num_ground_truth'][t, m, s] = right, ac_n, rc_n
                out['accuracy'][t, m, s], out['recall'][t, m, s] = r['accuracy'], r['recall']
                assert len(r['report']) < 200
                out['report'][t, m, s] = r['report']
    return out


def check_inputs(arr, images, groups, res):
    """every situation the tests rely on occurs"""
    box, score = oracle.detections_from_f32(arr['det'])
    names = [str(n) for n in arr['cat_names']]
    tie_gt = tie_det = False
    for i in range(len(images)):
        gs, ds = np.nonzero(arr['gt_img'] == i)[0], np.nonzero(arr['det_img'] == i)[0]
        if len(gs) and len(ds):
            t = oracle.iou_matrix(arr['gt_box'][gs], box[ds])
            for row in t:
                v = row[row > 0.5]
                tie_det |= len(set(v.tolist())) < len(v)
            for col in t.T:
                v = col[col > 0.5]
                tie_gt |= len(set(v.tolist())) < len(v)
    assert tie_gt and tie_det, 'exact IoU ties between two ground truths / two detections'
    st = images[1]
    t = oracle.iou_matrix(np.array([x[:4] for x in st['gts']], np.float64),
                          oracle.detections_from_f32(np.array([x[:5] for x in st['dets']], np.float32))[0])
    # dets[0] has the higher score and prefers gts[0], but (gts[0], dets[1]) has the best IoU and takes gts[0] first
    assert st['dets'][0][4] > st['dets'][1][4] and t[0, 1] > t[0, 0] > t[1, 0] > 0.5 > t[1, 1]
    a = groups[0]
    assert res[0]['det_code'][0, 0, 0][arr['det_img'] == 1].tolist() == [oracle.DET_RIGHT, oracle.DET_RIGHT]
    assert any((score == m).any() for m in a['minscores']), 'a score exactly at minscore'
    assert (score[arr['det_img'] == 5] == [50.0, 75.0, np.float64(np.float32(0.9)) * 100, 90.625]).all() and score[arr['det_img'] == 5][2] < 90
    gsz, dsz = oracle.long_side(arr['gt_box']), oracle.long_side(box)
    for v in (32.0, 96.0, 400.0):
        assert (gsz == v).any() and (dsz == v).any(), v
    # a matched pair whose ground truth falls outside the band: the detection is in the band, in types, above minscore, yet excluded
    s = a['size_ranges'].index([32, 96])
    code = res[0]['det_code'][0, 0, s]
    in_types = np.array([names[c] in a['types'] for c in range(len(names))])
    det_cat = arr['det_label']
    kill = (code == 0) & (dsz >= 32) & (dsz < 96) & (score >= a['minscores'][0]) & in_types[det_cat]
    assert kill.any() and kill[arr['det_img'] == 3].tolist() == [True, False]
    assert (~in_types[arr['gt_cat']]).any() and (~in_types[det_cat]).any()
    n_gt = np.bincount(arr['gt_img'], minlength=len(images))
    n_dt = np.bincount(arr['det_img'], minlength=len(images))
    assert ((n_gt == 0) & (n_dt > 0)).any() and ((n_gt > 0) & (n_dt == 0)).any() and ((n_gt == 0) & (n_dt == 0)).any()
    assert n_gt.max() > 64 and n_dt.max() > 1024 and int(np.argmax(n_gt)) == int(np.argmax(n_dt))
    area = (box[:, 2] - box[:, 0]) * (box[:, 3] - box[:, 1])
    assert (area == 0).sum() >= 2 and ((arr['gt_box'][:, 2] - arr['gt_box'][:, 0]) * (arr['gt_box'][:, 3] - arr['gt_box'][:, 1]) > 0).all()
    assert any(not g['match_same'] and g['check_type'] for g in groups) and any(not g['match_same'] and not g['check_type'] for g in groups)
    assert any(g['types'] is None for g in groups)
    assert (res[1]['det_code'] == oracle.DET_WRONG).any() and not (res[2]['det_code'] == oracle.DET_WRONG).any()
    assert not np.array_equal(res[1]['right'], res[2]['right'])
    assert len(set(int(v) for v in res[0]['right'].ravel())) > 6      # the combinations really differ


def generate():
    ref = load_reference()
    type45 = list(ref.type45)
    assert len(type45) == 45
    names = type45 + OTHER
    images = build_images(names)
    arr = to_arrays(images, names)
    gd, rt = annotations_dict(arr, True), results_dict(arr, True)
    groups = groups_of(type45)
    res = [run_group(ref, gd, rt, g, len(arr['det_label']), len(arr['gt_cat'])) for g in groups]
    check_inputs(arr, images, groups, res)
    out = dict(arr)
    out['type45'] = np.array(type45)
    out['num_groups'] = np.array(len(groups))
    for i, (g, r) in enumerate(zip(groups, res)):
        out['g%d_params' % i] = np.array(json.dumps(g))
        for k, v in r.items():
            out['g%d_%s' % (i, k)] = v
    # the results dictionary a user writes for the official tool, first two images, without the tagging keys
    plain = results_dict(arr, False)
    out['results_json'] = np.array(json.dumps(dict(imgs=dict((k, plain['imgs'][k]) for k in list(plain['imgs'])[:2]))))
    return out


def main():
    out = generate()
    if '--check' in sys.argv:
        old = np.load(os.path.join(HERE, OUT_NAME), allow_pickle=False)
        bad = sorted(set(out) ^ set(old.files))
        worst = 0.0
        for k in sorted(set(out) & set(old.files)):
            a, b = np.asarray(out[k]), old[k]
            if a.shape != b.shape or a.dtype != b.dtype:
                bad.append(k)
            elif a.dtype.kind in 'USb':
                bad += [] if bool(np.all(a == b)) else [k]
            elif a.size:
                worst = max(worst, float(np.max(np.abs(a.astype(np.float64) - b.astype(np.float64)))))
        print('%s: %d arrays, max abs diff %g, %d arrays differ in keys / shape / text %s' % (OUT_NAME, len(out), worst, len(bad), bad[:6]))
        return 1 if (bad or worst != 0.0) else 0
    path = os.path.join(os.environ.get('LFD_GOLDEN_OUT', HERE), OUT_NAME)
    np.savez_compressed(path, **out)
    print('wrote %s: %d bytes, %d images, %d ground truth, %d detections, %d groups' % (
        path, os.path.getsize(path), len(out['image_ids']), len(out['gt_cat']), len(out['det_label']), int(out['num_groups'])))
    return 0


if __name__ == '__main__':
    sys.exit(main())
