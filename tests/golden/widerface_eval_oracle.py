"""The WIDERFACE protocol (easy / medium / hard AP) as plain numpy loops: DESIGN.md 9c, step by step.  It restates the
dataset's eval_tools (wider_eval.m, evaluation.m, read_pred.m, norm_score.m, boxoverlap.m) and VOC's VOCap from knowledge of
them; agreement with those tools is not verified.  Nothing here is imported from the package: the kernels and
lfd_amd.evaluation are tested against this file, and test_widerface_eval_host.py pins this file to answers worked out by hand.

An image is (boxes [G, 4] xywh, keep, dets): keep is {'easy' | 'medium' | 'hard': 0-based indices into boxes}; dets is a
[n, 5] array of rows [x, y, w, h, score], or None for an image that was never passed to the evaluator."""
import math

import numpy as np

DIFFICULTIES = ('easy', 'medium', 'hard')


def thresholds(T=1000):
    return np.array([1 - (t + 1) / T for t in range(T)], np.float64)


def quantise_row(r):
    """SIO_evaluation line 41: what the text file keeps of one row [x, y, w, h, score]"""
    s = float(r[4])
    return [float(math.floor(r[0])), float(math.floor(r[1])), float(math.ceil(r[2])), float(math.ceil(r[3])),
            float('%.03f' % min(s, 1))]


def as_written_rows(dets):
    """the rows of one image's text file: the dummy row of line 39 first"""
    return [[0.0, 0.0, 0.0, 0.0, 0.001]] + [quantise_row(r) for r in np.asarray(dets, np.float64).reshape(-1, 5)]


def iou(d, g):
    """+1 convention on corner boxes x2 = x + w, y2 = y + h"""
    dx, dy, dw, dh = (np.float64(v) for v in d[:4])
    gx, gy, gw, gh = (np.float64(v) for v in g[:4])
    iw = (min(dx + dw, gx + gw) - max(dx, gx)) + 1
    ih = (min(dy + dh, gy + gh) - max(dy, gy)) + 1
    if iw <= 0 or ih <= 0:
        return np.float64(0.0)
    inter = iw * ih
    return inter / (((dw + 1) * (dh + 1) + (gw + 1) * (gh + 1)) - inter)


def voc_ap(rec, prec):
    mrec = [0.0] + [float(v) for v in rec] + [1.0]
    mpre = [0.0] + [float(v) for v in prec] + [0.0]
    for i in range(len(mpre) - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    ap = 0.0
    for i in range(len(mrec) - 1):
        if mrec[i + 1] != mrec[i]:
            ap += (mrec[i + 1] - mrec[i]) * mpre[i + 1]
    return ap


def evaluate(images, iou_thresh=0.5, as_written=False, T=1000):
    """-> dict: curve int64 [3, T, 2], faces int64 [3], precision / recall float64 [3, T], ap float64 [3], lo, hi and, per
    image, None (no detections or no ground truth) or a dict with order (rank -> row of the image's detections), score
    (normalised, ranked), m, over and, per difficulty, proposal and rec [3, n]."""
    thr = thresholds(T)
    dets = []
    for boxes, keep, d in images:
        if d is None:
            dets.append(np.zeros((0, 5)))
        elif as_written:
            dets.append(np.array(as_written_rows(d), np.float64).reshape(-1, 5))
        else:
            dets.append(np.array(d, np.float64).reshape(-1, 5))
    scores = [float(s) for d in dets for s in d[:, 4]]
    lo = min(scores) if scores else 0.0
    hi = max(scores) if scores else 0.0
    diff = np.float64(hi) - np.float64(lo)
    if diff == 0:
        diff = np.float64(1.0)
    curve = np.zeros((3, T, 2), np.int64)
    faces = np.zeros(3, np.int64)
    per_image = []
    for (boxes, keep, _), d in zip(images, dets):
        boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
        G, n = len(boxes), len(d)
        for k, name in enumerate(DIFFICULTIES):
            faces[k] += len(keep[name])
        if G == 0 or n == 0:
            per_image.append(None)
            continue
        order = sorted(range(n), key=lambda i: -d[i, 4])               # stable: ties keep insertion order
        norm = [(np.float64(d[i, 4]) - np.float64(lo)) / diff for i in order]
        m, over = [], []
        for i in order:
            best, arg = None, 0
            for g in range(G):
                v = iou(d[i], boxes[g])
                if best is None or v > best:
                    best, arg = v, g
            m.append(arg)
            over.append(bool(best >= iou_thresh))
        norm_arr = np.array(norm, np.float64)
        count = [int((norm_arr >= thr[t]).sum()) for t in range(T)]      # n of step 5
        proposal, rec = np.zeros((3, n), np.int64), np.zeros((3, n), np.int64)
        for k, name in enumerate(DIFFICULTIES):
            kept = np.zeros(G, bool)
            for g in keep[name]:
                kept[int(g)] = True
            hit = np.zeros(G, np.int64)
            for h in range(n):
                proposal[k, h] = 1
                if over[h] and not kept[m[h]]:
                    hit[m[h]] = -1
                    proposal[k, h] = 0
                if over[h] and kept[m[h]] and hit[m[h]] == 0:
                    hit[m[h]] = 1
                rec[k, h] = int((hit == 1).sum())
            prop_run = np.cumsum(proposal[k])
            for t in range(T):
                cnt = count[t]
                if cnt > 0:
                    curve[k, t, 0] += prop_run[cnt - 1]
                    curve[k, t, 1] += rec[k, cnt - 1]
        per_image.append(dict(order=np.array(order), score=norm_arr, m=np.array(m), over=np.array(over),
                              proposal=proposal, rec=rec))
    precision, recall = np.zeros((3, T), np.float64), np.zeros((3, T), np.float64)
    ap = np.zeros(3, np.float64)
    for k in range(3):
        for t in range(T):
            if curve[k, t, 0] != 0:
                precision[k, t] = np.float64(curve[k, t, 1]) / np.float64(curve[k, t, 0])
            if faces[k] != 0:
                recall[k, t] = np.float64(curve[k, t, 1]) / np.float64(faces[k])
        ap[k] = voc_ap(recall[k], precision[k])
    return dict(curve=curve, faces=faces, precision=precision, recall=recall, ap=ap, lo=lo, hi=hi, images=per_image, thr=thr)
