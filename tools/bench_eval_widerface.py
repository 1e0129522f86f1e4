"""Times the device WIDERFACE evaluator (lfd_amd.evaluation.WIDERFACEEvaluator, csrc/evaluate_widerface.hip) on a seeded
synthetic set of WIDERFACE val's shape: 3226 images, about 39.7 k faces with a long-tailed faces-per-image distribution (one
image with about 2000), for two loads: about 100 and about 1000 detections per image.

  append      update_resident for the whole set in batches of 8: device events around the enqueued appends;
  match       lfd_eval_wf_match (score range, grouping, ranking, matching, walks, threshold sweep): device events;
  evaluate()  the host clock around evaluate(): the kernels, the one device-to-host copy and the APs on the host;
  oracle      the numpy restatement tests/golden/widerface_eval_oracle.py on a slice of the images, host clock.  It is plain
              Python loops, NOT the dataset's Matlab tools or their Python port; neither was measured.

Device figures are the median of --runs runs after 3 warm-ups.  Prints a table and one JSON line.  Needs the MI355X."""
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


def synthetic_ground_truth(images, seed):
    rng = np.random.RandomState(seed)
    faces = np.minimum(2000, np.ceil(rng.lognormal(1.375, 1.5, images))).astype(np.int64)
    faces[rng.randint(0, images)] = 1968                       # the crowd image at the end of the tail
    ann = []
    for i in range(images):
        g = int(faces[i])
        wh = np.exp(rng.uniform(np.log(6), np.log(300 if g < 50 else 40), (g, 2)))
        xy = rng.uniform(0, 1000, (g, 2))
        kind = rng.randint(0, 4, g)                             # none, hard, medium + hard, all three
        ann.append(dict(id=i, event='%d--Event' % (i % 61), stem='%d_Event_%d' % (i % 61, i), boxes=np.concatenate([xy, wh], 1),
                        keep=dict(easy=np.nonzero(kind == 3)[0].tolist(), medium=np.nonzero(kind >= 2)[0].tolist(),
                                  hard=np.nonzero(kind >= 1)[0].tolist())))
    return ann


def synthetic_detections(ann, dets, seed):
    """fp32 [images, dets, 5] x1 y1 x2 y2 score: jittered ground truth first, random boxes for the rest"""
    rng = np.random.RandomState(seed)
    out = np.zeros((len(ann), dets, 5), np.float32)
    for i, a in enumerate(ann):
        g = len(a['boxes'])
        k = min(dets, 2 * g)
        box = np.zeros((dets, 4))
        if k:
            src = a['boxes'][rng.randint(0, g, k)]
            jit = rng.normal(0, 0.06, (k, 4)) * np.concatenate([src[:, 2:], src[:, 2:]], 1)
            box[:k, :2] = src[:, :2] + jit[:, :2]
            box[:k, 2:] = np.maximum(1.0, src[:, 2:] + jit[:, 2:])
        box[k:, :2] = rng.uniform(0, 1000, (dets - k, 2))
        box[k:, 2:] = np.exp(rng.uniform(np.log(6), np.log(300), (dets - k, 2)))
        out[i, :, 0:2] = box[:, :2]
        out[i, :, 2:4] = box[:, :2] + box[:, 2:] - 1
        out[i, :, 4] = rng.uniform(0.01, 1.0, dets)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--images', type=int, default=3226)
    ap.add_argument('--loads', type=int, nargs='+', default=[100, 1000])
    ap.add_argument('--runs', type=int, default=20)
    ap.add_argument('--oracle-images', type=int, default=24)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()
    import torch
    from lfd_amd import evaluation, ops
    import widerface_eval_oracle as oracle
    assert torch.cuda.is_available(), 'bench_eval_widerface needs the MI355X'
    ann = synthetic_ground_truth(args.images, args.seed)
    faces = sum(len(a['boxes']) for a in ann)
    res = dict(protocol='widerface', images=args.images, faces=faces, max_faces_per_image=max(len(a['boxes']) for a in ann),
               runs=args.runs, loads=[])
    B = 8
    for dets in args.loads:
        det_all = synthetic_detections(ann, dets, args.seed + dets)
        outs = []
        for i in range(0, args.images, B):
            o = ops.DetectOutputs()
            o.dets = torch.from_numpy(det_all[i:i + B]).cuda()
            o.labels = torch.zeros((o.dets.size(0), dets), dtype=torch.int32, device='cuda')
            o.counts = torch.zeros((o.dets.size(0), 4), dtype=torch.int32, device='cuda')
            o.counts[:, 1] = dets
            o.cand = o.point = o.ws = None
            outs.append((o, [dict(image_id=j) for j in range(i, min(i + B, args.images))]))
        ev = evaluation.WIDERFACEEvaluator(annotations=ann)

        def fill():
            for o, meta in outs:
                ev.update_resident(o, meta)
        t_append, t_match, t_eval = [], [], []
        aps = None
        for run in range(3 + args.runs):
            e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            e[0].record()
            fill()
            e[1].record()
            e[2].record()
            keep = ev._run()                                    # the kernels alone; evaluate() below runs them again
            e[3].record()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            aps = ev.evaluate()
            t1 = time.perf_counter()
            del keep
            if run >= 3:
                t_append.append(e[0].elapsed_time(e[1]))
                t_match.append(e[2].elapsed_time(e[3]))
                t_eval.append((t1 - t0) * 1e3)
        n_or = min(args.oracle_images, args.images)
        images = []
        for i in range(n_or):
            d = det_all[i]
            w, h = d[:, 2] - d[:, 0] + np.float32(1), d[:, 3] - d[:, 1] + np.float32(1)
            images.append((ann[i]['boxes'], ann[i]['keep'], np.stack([d[:, 0], d[:, 1], w, h, d[:, 4]], 1).astype(np.float64)))
        t0 = time.perf_counter()
        oracle.evaluate(images)
        t_or = time.perf_counter() - t0
        res['loads'].append(dict(dets_per_image=dets, detections=dets * args.images, append_ms=float(np.median(t_append)),
                                 match_ms=float(np.median(t_match)), evaluate_ms=float(np.median(t_eval)),
                                 ap=[aps[k] for k in ('easy', 'medium', 'hard')], numpy_oracle_images=n_or,
                                 numpy_oracle_faces=sum(len(im[0]) for im in images), numpy_oracle_s=t_or))
    print('| detections per image | detections | append ms | match ms | evaluate() ms | numpy oracle, %d images, s |' % res['loads'][0]['numpy_oracle_images'])
    print('|---|---|---|---|---|---|')
    for l in res['loads']:
        print('| %d | %d | %.2f | %.2f | %.2f | %.1f |' % (l['dets_per_image'], l['detections'], l['append_ms'], l['match_ms'],
                                                          l['evaluate_ms'], l['numpy_oracle_s']))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
