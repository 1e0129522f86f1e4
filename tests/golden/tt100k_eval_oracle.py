"""The TT100K protocol (accuracy / recall) as plain numpy / Python: the definition of DESIGN.md 9b written for this repository,
the role coco_eval_oracle.py has for the COCO evaluator.  tests/test_tt100k_eval_host.py pins it to the fixture recorded from
the reference's own official_eval.eval_annos (tests/golden/ref_tt100k_eval.npz) exactly; the GPU tests compare the kernels
with it on fresh inputs.  All arithmetic is float64 in the order the definition writes it.

Outcome codes (include/lfd_hip.h LFD_TT100K_*): detection 0 excluded / 1 right / 2 wrong category / 3 unmatched; ground truth
0 excluded / 1 missed / 2 matched."""
import numpy as np

DET_EXCLUDED, DET_RIGHT, DET_WRONG, DET_UNMATCHED = 0, 1, 2, 3
GT_EXCLUDED, GT_MISSED, GT_MATCHED = 0, 1, 2


def detections_from_f32(dets_f32):
    """fp32 [D, 5] = {x1, y1, x2, y2, score} -> (boxes float64 [D, 4] = {xmin, ymin, xmax, ymax}, scores float64 0..100): the
    width is x2 - x1 + 1 in fp32 (LFD._pack), xmax is the float64 sum of that width and x1, the score is scaled in float64."""
    d = np.asarray(dets_f32, np.float32).reshape(-1, 5)
    one = np.float32(1.0)
    w = (d[:, 2] - d[:, 0]) + one
    h = (d[:, 3] - d[:, 1]) + one
    x, y = d[:, 0].astype(np.float64), d[:, 1].astype(np.float64)
    boxes = np.stack([x, y, w.astype(np.float64) + x, h.astype(np.float64) + y], 1)
    return boxes, d[:, 4].astype(np.float64) * 100.0


def detections_from_rows(rows):
    """[label, score, x, y, w, h] rows (LFD.get_results) -> (labels, boxes, scores) with the same arithmetic in float64"""
    r = np.asarray(rows, np.float64).reshape(-1, 6)
    boxes = np.stack([r[:, 2], r[:, 3], r[:, 4] + r[:, 2], r[:, 5] + r[:, 3]], 1)
    return r[:, 0].astype(np.int64), boxes, r[:, 1] * 100.0


def _area(b):
    return np.maximum(0.0, (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1]))


def iou_matrix(gt, det):
    """[G, D]; 0 / 0 is NaN (no candidate), where the reference raises"""
    g, d = gt[:, None, :], det[None, :, :]
    x1, y1 = np.maximum(g[..., 0], d[..., 0]), np.maximum(g[..., 1], d[..., 1])
    x2, y2 = np.minimum(g[..., 2], d[..., 2]), np.minimum(g[..., 3], d[..., 3])
    x2, y2 = np.maximum(x2, x1), np.maximum(y2, y1)
    ac = np.maximum(0.0, (x2 - x1) * (y2 - y1))
    with np.errstate(invalid='ignore', divide='ignore'):
        return ac / (_area(g) + _area(d) - ac)


def long_side(b):
    b = np.asarray(b, np.float64).reshape(-1, 4)
    return np.maximum(b[:, 2] - b[:, 0], b[:, 3] - b[:, 1])


def match_image(gt_box, gt_cat, det_box, det_cat, det_score, iou, minscore, in_types=None, match_same=True):
    """Steps 1-3 for one image.  gt_cat / det_cat: category indices; in_types: bool per category index or None.
    -> (match_g [G], match_r [D]): partner index, -1 free, -2 taken out before the matching."""
    gt_box = np.asarray(gt_box, np.float64).reshape(-1, 4)
    det_box = np.asarray(det_box, np.float64).reshape(-1, 4)
    gt_cat, det_cat = np.asarray(gt_cat, np.int64).reshape(-1), np.asarray(det_cat, np.int64).reshape(-1)
    G, D = len(gt_cat), len(det_cat)
    mg, mr = np.full(G, -1, np.int64), np.full(D, -1, np.int64)
    if in_types is not None:
        mg[~np.asarray(in_types, bool)[gt_cat]] = -2
        mr[~np.asarray(in_types, bool)[det_cat]] = -2
    mr[np.asarray(det_score, np.float64).reshape(-1) < minscore] = -2
    if G == 0 or D == 0:
        return mg, mr
    t = iou_matrix(gt_box, det_box)
    with np.errstate(invalid='ignore'):
        ok = (t > iou) & (mg[:, None] != -2) & (mr[None, :] != -2)
    if match_same:
        ok &= gt_cat[:, None] == det_cat[None, :]
    gi, dj = np.nonzero(ok)                                  # generation order: i ascending, then j ascending
    for k in np.argsort(-t[gi, dj], kind='stable'):
        i, j = gi[k], dj[k]
        if mg[i] == -1 and mr[j] == -1:
            mg[i], mr[j] = j, i
    return mg, mr


def band_codes(gt_box, gt_cat, det_box, det_cat, mg, mr, lo, hi, check_type=True):
    """Steps 4-5 for one image and one size band -> (det_code [D], gt_code [G])"""
    gt_cat, det_cat = np.asarray(gt_cat, np.int64).reshape(-1), np.asarray(det_cat, np.int64).reshape(-1)
    gs, ds = long_side(gt_box), long_side(det_box)
    g_in = (gs >= lo) & (gs < hi)
    d_in = (ds >= lo) & (ds < hi)
    gt_code = np.where((mg == -2) | ~g_in, GT_EXCLUDED, np.where(mg >= 0, GT_MATCHED, GT_MISSED)).astype(np.uint8)
    det_code = np.zeros(len(det_cat), np.uint8)
    for j in range(len(det_cat)):
        m = mr[j]
        if m >= 0:
            if g_in[m]:
                det_code[j] = DET_RIGHT if (not check_type or gt_cat[m] == det_cat[j]) else DET_WRONG
        elif m == -1 and d_in[j]:
            det_code[j] = DET_UNMATCHED
    return det_code, gt_code


def ratio(right, n):
    """the reference's expression: the int 1 when nothing was counted"""
    return 1 if n == 0 else right * 1.0 / n


def evaluate(images, ious, minscores, size_ranges, in_types=None, check_type=True, match_same=True, num_categories=None):
    """images: list of (gt_box [G, 4], gt_cat [G], det_box [D, 4], det_cat [D], det_score [D]).
    -> dict: right, num_detections, num_ground_truth int64 [T, M, S]; accuracy, recall float64; per_category int64
    [T, M, S, K, 3] = {right, detections, ground truth}; det_code / gt_code / det_gt: per image, lists indexed [t][m][s]."""
    T, M, S = len(ious), len(minscores), len(size_ranges)
    K = num_categories if num_categories is not None else (len(in_types) if in_types is not None else 1 + max(
        [int(np.max(c)) for im in images for c in (im[1], im[3]) if len(c)] + [0]))
    tot = np.zeros((T, M, S, 3), np.int64)
    per = np.zeros((T, M, S, K, 3), np.int64)
    det_code, gt_code, det_gt = [], [], []
    for gb, gc, db, dc, sc in images:
        gc, dc = np.asarray(gc, np.int64).reshape(-1), np.asarray(dc, np.int64).reshape(-1)
        dcode = [[[None] * S for _ in range(M)] for _ in range(T)]
        gcode = [[[None] * S for _ in range(M)] for _ in range(T)]
        dgt = [[None] * M for _ in range(T)]
        for t in range(T):
            for m in range(M):
                mg, mr = match_image(gb, gc, db, dc, sc, ious[t], minscores[m], in_types, match_same)
                dgt[t][m] = mr
                for s, (lo, hi) in enumerate(size_ranges):
                    d_, g_ = band_codes(gb, gc, db, dc, mg, mr, lo, hi, check_type)
                    dcode[t][m][s], gcode[t][m][s] = d_, g_
                    tot[t, m, s] += [int((d_ == DET_RIGHT).sum()), int((d_ != DET_EXCLUDED).sum()), int((g_ != GT_EXCLUDED).sum())]
                    np.add.at(per[t, m, s, :, 0], dc[d_ == DET_RIGHT], 1)
                    np.add.at(per[t, m, s, :, 1], dc[d_ != DET_EXCLUDED], 1)
                    np.add.at(per[t, m, s, :, 2], gc[g_ != GT_EXCLUDED], 1)
        det_code.append(dcode)
        gt_code.append(gcode)
        det_gt.append(dgt)
    acc = np.array([float(ratio(int(r), int(n))) for r, n in zip(tot[..., 0].ravel(), tot[..., 1].ravel())]).reshape(T, M, S)
    rec = np.array([float(ratio(int(r), int(n))) for r, n in zip(tot[..., 0].ravel(), tot[..., 2].ravel())]).reshape(T, M, S)
    return dict(right=tot[..., 0].copy(), num_detections=tot[..., 1].copy(), num_ground_truth=tot[..., 2].copy(), accuracy=acc,
                recall=rec, per_category=per, det_code=det_code, gt_code=gt_code, det_gt=det_gt)


def report(iou, lo, hi, types, check_type, right, num_detections, num_ground_truth):
    """the reference's report line; `types`: list of names or None.  A single name prints as itself (the reference raises)."""
    if types is None:
        styps = 'all'
    else:
        distinct = list(dict.fromkeys(types))
        if len(distinct) == 1:
            styps = distinct[0]
        elif not check_type or len(distinct) == 0:
            styps = 'none'
        else:
            styps = '[%s, ...total %s...]' % (distinct[0], len(distinct))
    return 'iou:%s, size:[%s,%s), types:%s, accuracy:%s, recall:%s' % (
        iou, lo, hi, styps, ratio(int(right), int(num_detections)), ratio(int(right), int(num_ground_truth)))
