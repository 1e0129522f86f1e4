"""Times the device evaluator (lfd_amd/evaluation.py, csrc/evaluate.hip) on a synthetic set of COCO val2017's shape:
5000 images, 80 categories, about 7 ground-truth boxes and --dets detections per image, seeded.

  (a) evaluate() on the device, stage 1 (match) and stage 2 (accumulate) separately: device events, median of --runs runs
      after 3 warm-ups;
  (b) update_resident per batch of 8 (device events around the enqueued appends) against update on the lists of the same
      batches (host clock, ends in a synchronise; the lists are made outside the timed window);
  (c) the numpy restatement of the definition (tests/golden/coco_eval_oracle.py) on a 500-image slice: the only host figure
      available.  It is plain Python loops, NOT pycocotools; pycocotools itself was not measured.

--protocol tt100k times the TT100K protocol instead (lfd_amd.evaluation.TT100KEvaluator, csrc/evaluate_tt100k.hip) on a set of
TT100K's test split's shape -- 3000 images, 45 classes, a few signs and --dets detections per image: update_resident per batch
of 8, then evaluate() (device events around the enqueued kernels, and the host clock around the whole call, which ends in
the one device-to-host copy) for the reference's default call and for a 3-band x 10-minscore sweep; beside it the numpy
restatement tests/golden/tt100k_eval_oracle.py on a slice, on the host CPU.

Prints one JSON line.  Needs the MI355X: there is no CPU path."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, 'lfd-a-light-and-fast-detector_amd'), os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)


def synthetic(images, cats, dets, seed):
    rng = np.random.RandomState(seed)
    anns, batches = [], []
    det_all = np.zeros((images, dets, 5), np.float32)
    lab_all = np.zeros((images, dets), np.int32)
    for i in range(images):
        n_gt = int(rng.poisson(7))
        wh = np.exp(rng.uniform(np.log(8), np.log(300), (n_gt, 2)))
        xy = rng.uniform(0, 500, (n_gt, 2))
        gcat = rng.randint(0, cats, n_gt)
        for j in range(n_gt):
            anns.append(dict(id=len(anns) + 1, image_id=i + 1, category_id=int(gcat[j]) + 1, iscrowd=int(rng.rand() < 0.02),
                             bbox=[float(xy[j, 0]), float(xy[j, 1]), float(wh[j, 0]), float(wh[j, 1])], area=float(wh[j, 0] * wh[j, 1])))
        # detections: jittered ground truth first, random boxes for the rest
        k = min(dets, 2 * n_gt)
        src = rng.randint(0, max(n_gt, 1), k)
        box = np.zeros((dets, 4))
        lab = rng.randint(0, cats, dets)
        if n_gt:
            jit = rng.normal(0, 0.06, (k, 4)) * np.concatenate([wh[src], wh[src]], 1)
            box[:k, :2] = xy[src] + jit[:, :2]
            box[:k, 2:] = np.maximum(1.0, wh[src] + jit[:, 2:])
            lab[:k] = gcat[src]
        else:
            k = 0
        box[k:, :2] = rng.uniform(0, 500, (dets - k, 2))
        box[k:, 2:] = np.exp(rng.uniform(np.log(8), np.log(300), (dets - k, 2)))
        det_all[i, :, 0:2] = box[:, :2]
        det_all[i, :, 2:4] = box[:, :2] + box[:, 2:] - 1
        det_all[i, :, 4] = np.round(rng.uniform(0.05, 1.0, dets), 3)
        lab_all[i] = lab
    coco = dict(images=[dict(id=i + 1) for i in range(images)], categories=[dict(id=c + 1) for c in range(cats)], annotations=anns)
    return coco, det_all, lab_all


def main_tt100k(args):
    import torch
    from lfd_amd import evaluation, ops
    import tt100k_eval_oracle as oracle
    assert torch.cuda.is_available(), 'bench_eval needs the MI355X'
    names = list(evaluation.TYPE45)[:args.categories] + ['class_%d' % i for i in range(len(evaluation.TYPE45), args.categories)]
    coco, det_all, lab_all = synthetic(args.images, args.categories, args.dets, args.seed)
    imgs = dict((str(i + 1), dict(objects=[])) for i in range(args.images))
    for a in coco['annotations']:
        x, y, w, h = a['bbox']
        imgs[str(a['image_id'])]['objects'].append(dict(bbox=dict(xmin=x, ymin=y, xmax=x + w, ymax=y + h), category=names[a['category_id'] - 1]))
    ann = dict(imgs=imgs)
    B = 8
    outs = []
    for i in range(0, args.images, B):
        o = ops.DetectOutputs()
        o.dets = torch.from_numpy(det_all[i:i + B]).cuda()
        o.labels = torch.from_numpy(lab_all[i:i + B]).cuda()
        o.counts = torch.zeros((o.dets.size(0), 4), dtype=torch.int32, device='cuda')
        o.counts[:, 1] = args.dets
        o.cand = o.point = o.ws = None
        outs.append((o, [dict(image_id=j + 1) for j in range(i, min(i + B, args.images))]))
    sweep = dict(minscore=[5 + 10 * k for k in range(10)], size_ranges=((0, 32), (32, 96), (96, 400)))
    n_or = min(args.oracle_images, args.images)
    gt_by_img = [[] for _ in range(n_or)]
    for a in coco['annotations']:
        if a['image_id'] <= n_or:
            x, y, w, h = a['bbox']
            gt_by_img[a['image_id'] - 1].append(([x, y, x + w, y + h], a['category_id'] - 1))
    or_images = []
    for i in range(n_or):
        box, score = oracle.detections_from_f32(det_all[i])
        or_images.append((np.array([g[0] for g in gt_by_img[i]], np.float64).reshape(-1, 4), np.array([g[1] for g in gt_by_img[i]], np.int64),
                          box, lab_all[i], score))
    res = dict(protocol='tt100k', images=args.images, categories=args.categories, dets_per_image=args.dets,
               ground_truth=len(coco['annotations']), runs=args.runs, numpy_oracle_images=n_or)
    for tag, kw in (('default', dict()), ('sweep', sweep)):
        ev = evaluation.TT100KEvaluator(annotations=ann, label_indexes_to_category_names=names, types=names, **kw)

        def fill():
            for o, meta in outs:
                ev.update_resident(o, meta)
        fill()
        ev.evaluate()                         # warm-up of every kernel, sizes the store
        torch.cuda.synchronize()
        app, dev, wall = [], [], []
        for _ in range(args.runs):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            fill()
            e[1].record()
            e[2].record()
            ev._run()
            e[3].record()
            torch.cuda.synchronize()
            app.append(e[0].elapsed_time(e[1]) / len(outs))
            dev.append(e[2].elapsed_time(e[3]))
            t0 = time.perf_counter()
            ev.evaluate()
            wall.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        ref = oracle.evaluate(or_images, [float(v) for v in ev.ious], [float(v) for v in ev.minscores],
                              [[float(a), float(b)] for a, b in ev.size_ranges], None, True, True, num_categories=args.categories)
        oracle_s = time.perf_counter() - t0
        res[tag] = dict(combinations=int(ev.right.size), update_resident_ms_per_batch8=round(float(np.median(app)), 4),
                        evaluate_device_ms=round(float(np.median(dev)), 3), evaluate_call_ms=round(float(np.median(wall)), 3),
                        numpy_oracle_s=round(oracle_s, 2), accuracy=float(ev.accuracy.ravel()[0]), recall=float(ev.recall.ravel()[0]),
                        oracle_slice_recall=float(ref['recall'].ravel()[0]))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--protocol', choices=['coco', 'tt100k'], default='coco')
    ap.add_argument('--images', type=int, default=None, help='default: 5000 (coco), 3000 (tt100k)')
    ap.add_argument('--categories', type=int, default=None, help='default: 80 (coco), 45 (tt100k)')
    ap.add_argument('--dets', type=int, default=None, help='detections per image; default: 100 (coco), 20 (tt100k)')
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--oracle-images', type=int, default=500)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    for k, coco_default, tt_default in (('images', 5000, 3000), ('categories', 80, 45), ('dets', 100, 20)):
        if getattr(args, k) is None:
            setattr(args, k, tt_default if args.protocol == 'tt100k' else coco_default)
    if args.protocol == 'tt100k':
        return main_tt100k(args)
    import torch
    from lfd_amd import evaluation, ops
    from lfd_amd.model.lfd import LFD
    assert torch.cuda.is_available(), 'bench_eval needs the MI355X'
    coco, det_all, lab_all = synthetic(args.images, args.categories, args.dets, args.seed)
    label_map = dict((c, c + 1) for c in range(args.categories))
    B = 8
    outs = []
    for i in range(0, args.images, B):
        o = ops.DetectOutputs()
        o.dets = torch.from_numpy(det_all[i:i + B]).cuda()
        o.labels = torch.from_numpy(lab_all[i:i + B]).cuda()
        o.counts = torch.zeros((o.dets.size(0), 4), dtype=torch.int32, device='cuda')
        o.counts[:, 1] = args.dets
        o.cand = o.point = o.ws = None
        outs.append((o, [dict(image_id=j + 1) for j in range(i, min(i + B, args.images))]))
    ev = evaluation.COCOEvaluator(None, label_map, annotations=coco)

    def fill():
        for o, meta in outs:
            ev.update_resident(o, meta)

    # (b) appends: device-resident
    fill()
    ev.evaluate()                         # warm-up of every kernel, sizes the store
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fill()
    e1.record()
    host_enqueue = time.perf_counter() - t0
    torch.cuda.synchronize()
    resident_ms = e0.elapsed_time(e1) / len(outs)
    resident_host_ms = host_enqueue * 1e3 / len(outs)
    # (a) the two stages
    timing = []
    for _ in range(3 + args.runs):
        ev._run(timing=timing)
    torch.cuda.synchronize()
    match_ms = float(np.median([t[0].elapsed_time(t[1]) for t in timing[3:]]))
    acc_ms = float(np.median([t[1].elapsed_time(t[2]) for t in timing[3:]]))
    ev.evaluate()
    stats_resident = ev.stats.copy()
    # (b) appends: the reference's lists
    n_list_batches = min(len(outs), 64)
    lists = [([LFD._pack(o.dets[i, :args.dets], o.labels[i, :args.dets]) for i in range(o.dets.size(0))], meta)
             for o, meta in outs[:n_list_batches]]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for l, meta in lists:
        ev.update((l, meta))
    torch.cuda.synchronize()
    list_ms = (time.perf_counter() - t0) * 1e3 / n_list_batches
    ev.evaluate()
    # (c) the host oracle on a slice
    import coco_eval_oracle as oracle
    n_or = min(args.oracle_images, n_list_batches * B)
    dts = [dict(image_id=meta[i]['image_id'], category_id=label_map[r[0]], score=r[1], bbox=r[2:])
           for l, meta in lists for i in range(len(meta)) if meta[i]['image_id'] <= n_or for r in l[i]]
    gts = [a for a in coco['annotations'] if a['image_id'] <= n_or]
    t0 = time.perf_counter()
    ref = oracle.evaluate(gts, dts, list(range(1, n_or + 1)), sorted(label_map.values()))
    oracle_s = time.perf_counter() - t0
    print(json.dumps(dict(images=args.images, categories=args.categories, dets_per_image=args.dets, ground_truth=len(coco['annotations']),
                          runs=args.runs, match_ms=round(match_ms, 3), accumulate_ms=round(acc_ms, 3),
                          evaluate_device_ms=round(match_ms + acc_ms, 3),
                          update_resident_ms_per_batch8=round(resident_ms, 4), update_resident_host_ms_per_batch8=round(resident_host_ms, 4),
                          update_lists_ms_per_batch8=round(list_ms, 3), list_batches_timed=n_list_batches,
                          numpy_oracle_images=n_or, numpy_oracle_s=round(oracle_s, 2), numpy_oracle_is_pycocotools=False,
                          mAP=round(float(stats_resident[0]), 5), mAP_50=round(float(stats_resident[1]), 5),
                          oracle_slice_mAP_50=round(float(ref['stats'][1]), 5))))


if __name__ == '__main__':
    main()
