"""COCO-style bbox evaluation as plain numpy / Python loops: the definition of DESIGN.md "Evaluation" written down once more,
sharing no code with lfd_amd/evaluation.py or csrc/evaluate.hip.  It restates COCOeval (iouType 'bbox', useCats 1,
maxDets [100, 300, 1000]) from knowledge of pycocotools 2.0.x; pycocotools itself was never run against it.

evaluate(gts, dts, image_ids, category_ids) ->
    dict(precision [T,R,K,A,M], recall [T,K,A,M], stats [12], matches {(image_id, category_id): dict(index, matched, ignored)})
gts: dicts with image_id, category_id, bbox [x,y,w,h], area, iscrowd;  dts: dicts with image_id, category_id, bbox, score, in
insertion order;  image_ids: the images that are evaluated;  category_ids: the categories (K).
"""
import numpy as np

IOU_THRS = np.linspace(.5, .95, 10)
REC_THRS = np.linspace(0, 1, 101)
AREA_RNG = [[0, 1e10], [0, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e10]]
MAX_DETS = [100, 300, 1000]


def iou(d, g, crowd):
    dx, dy, dw, dh = d
    gx, gy, gw, gh = g
    w = min(dx + dw, gx + gw) - max(dx, gx)
    h = min(dy + dh, gy + gh) - max(dy, gy)
    if w <= 0 or h <= 0:
        return 0.0
    inter = w * h
    union = dw * dh if crowd else dw * dh + gw * gh - inter
    return inter / union


def match_pair(gt, dt, max_det):
    """gt, dt: the lists of one (image, category); dt in insertion order, each with its insertion 'index'.
    -> (indexes of the ranked detections, matched [T,A,D], ignored [T,A,D], non-ignored ground truth per area [A])"""
    # step 1: stable sort by score descending, cut
    order = sorted(range(len(dt)), key=lambda i: -dt[i]['score'])      # sorted() is stable
    dt = [dt[i] for i in order[:max_det]]
    T, A, D = len(IOU_THRS), len(AREA_RNG), len(dt)
    matched = np.zeros((T, A, D), bool)
    ignored = np.zeros((T, A, D), bool)
    npig = np.zeros(A, np.int64)
    # step 2
    ious = [[iou([float(v) for v in d['bbox']], [float(v) for v in g['bbox']], bool(g['iscrowd'])) for g in gt] for d in dt]
    for a, (lo, hi) in enumerate(AREA_RNG):
        # step 3
        g_ign = [bool(g['iscrowd']) or g['area'] < lo or g['area'] > hi for g in gt]
        gord = sorted(range(len(gt)), key=lambda j: g_ign[j])
        npig[a] = sum(1 for j in gord if not g_ign[j])
        for t, thr in enumerate(IOU_THRS):
            # step 4
            g_matched = [False] * len(gt)
            for di, d in enumerate(dt):
                best = min(thr, 1 - 1e-10)
                m = -1
                for j in gord:
                    if g_matched[j] and not gt[j]['iscrowd']:
                        continue
                    if m > -1 and not g_ign[m] and g_ign[j]:
                        break
                    if ious[di][j] < best:
                        continue
                    best = ious[di][j]
                    m = j
                if m > -1:
                    matched[t, a, di] = True
                    ignored[t, a, di] = g_ign[m]
                    g_matched[m] = True
                else:
                    # step 5
                    darea = float(d['bbox'][2]) * float(d['bbox'][3])
                    ignored[t, a, di] = darea < lo or darea > hi
    return [d['index'] for d in dt], matched, ignored, npig


def accumulate_cell(scores, matched, ignored, npig):
    """One (category, area, maxDets, threshold): scores / matched / ignored already concatenated over the images.
    -> (precision [R], recall)"""
    R = len(REC_THRS)
    if npig == 0:
        return np.full(R, -1.0), -1.0
    order = np.argsort(-np.asarray(scores, np.float64), kind='mergesort')
    tp = np.zeros(len(order), np.float64)
    fp = np.zeros(len(order), np.float64)
    ctp = cfp = 0.0
    for n, i in enumerate(order):
        if matched[i] and not ignored[i]:
            ctp += 1
        if not matched[i] and not ignored[i]:
            cfp += 1
        tp[n], fp[n] = ctp, cfp
    rc = tp / npig
    pr = tp / (fp + tp + np.spacing(1))
    recall = rc[-1] if len(rc) else 0.0
    for j in range(len(pr) - 1, 0, -1):
        pr[j - 1] = max(pr[j - 1], pr[j])
    q = np.zeros(R)
    p = 0
    for ri, r in enumerate(REC_THRS):      # ascending, and rc never decreases: the first index with rc[p] >= r only moves forward
        while p < len(rc) and rc[p] < r:
            p += 1
        q[ri] = pr[p] if p < len(rc) else 0.0
    return q, recall


def summarize(precision, recall):
    def mean(x):
        x = x[x > -1]
        return float(np.mean(x)) if x.size else -1.0
    return np.array([mean(precision[:, :, :, 0, 0]), mean(precision[0, :, :, 0, 2]), mean(precision[5, :, :, 0, 2]),
                     mean(precision[:, :, :, 1, 2]), mean(precision[:, :, :, 2, 2]), mean(precision[:, :, :, 3, 2]),
                     mean(recall[:, :, 0, 0]), mean(recall[:, :, 0, 1]), mean(recall[:, :, 0, 2]),
                     mean(recall[:, :, 1, 2]), mean(recall[:, :, 2, 2]), mean(recall[:, :, 3, 2])])


def evaluate(gts, dts, image_ids, category_ids):
    image_ids = sorted(set(image_ids))
    category_ids = sorted(set(category_ids))
    T, R, K, A, M = len(IOU_THRS), len(REC_THRS), len(category_ids), len(AREA_RNG), len(MAX_DETS)
    by_gt, by_dt = {}, {}
    for g in gts:
        by_gt.setdefault((g['image_id'], g['category_id']), []).append(g)
    for n, d in enumerate(dts):
        by_dt.setdefault((d['image_id'], d['category_id']), []).append(dict(d, index=n))
    matches = {}
    for i in image_ids:
        for k in category_ids:
            gt, dt = by_gt.get((i, k), []), by_dt.get((i, k), [])
            if not gt and not dt:
                continue
            index, matched, ignored, npig = match_pair(gt, dt, MAX_DETS[-1])
            by_index = dict((d['index'], d['score']) for d in dt)
            matches[(i, k)] = dict(index=index, matched=matched, ignored=ignored, npig=npig,
                                   scores=[by_index[x] for x in index])
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    for ki, k in enumerate(category_ids):
        pairs = [matches[(i, k)] for i in image_ids if (i, k) in matches]
        if not pairs:
            continue
        for a in range(A):
            npig = sum(int(p['npig'][a]) for p in pairs)
            for mi, md in enumerate(MAX_DETS):
                scores = [s for p in pairs for s in p['scores'][:md]]
                for t in range(T):
                    mt = [v for p in pairs for v in p['matched'][t, a, :md]]
                    ig = [v for p in pairs for v in p['ignored'][t, a, :md]]
                    precision[t, :, ki, a, mi], recall[t, ki, a, mi] = accumulate_cell(scores, mt, ig, npig)
    return dict(precision=precision, recall=recall, stats=summarize(precision, recall), matches=matches)
