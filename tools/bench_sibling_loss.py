"""tools/bench_sibling_loss.py -- get_loss of the sibling meta-architectures: the host route (`device_targets = False`:
targets per image with [P,G] tensor algebra on the host, uploaded; op-by-op loss modules) against the device route
(lfd_assign_targets_{fcos,v2}_f32 + the fused get_loss kernels), forward + backward to the prediction gradients, and the
target kernel alone.  FCOS_FPN and LFDV2_SIMPLE at 640x640, batch 32, 2-6 boxes per image (seeded).

    python tools/bench_sibling_loss.py [--iters 30] [--warmup 5] [--batch 32] [--size 640]

Each iteration is timed on the host clock between device synchronisations (get_loss ends in a host sync by contract: it
returns floats), the target kernel with device events; medians of `--iters` warmed-up iterations, min / max alongside.  One
JSON line per model."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'lfd-a-light-and-fast-detector_amd'), os.path.join(ROOT, 'tests', 'golden')):
    sys.path.insert(0, p)

from lfd_amd import configs, ops  # noqa: E402
import sibling_cases as SC  # noqa: E402


def level_sizes(strides, size):
    out = []
    for s in strides:
        out.append(((size + s - 1) // s, (size + s - 1) // s))
    return out


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))


def timed_events(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return dict(median_ms=statistics.median(ts), min_ms=min(ts), max_ms=max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=640)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    for name in ('FCOS_FPN', 'LFDV2_SIMPLE'):
        spec = configs.SIBLINGS[name]
        model = configs.build_sibling_model(name, seed=1).to(dev)
        C_ = spec['head']['num_classes']
        strides = list(model._point_strides)
        sizes = level_sizes(strides, args.size)
        for i, hw in enumerate(sizes):
            model._head_indexes_to_feature_map_sizes[i] = hw
        P = sum(h * w for h, w in sizes)
        ann = SC.synth_annotations(5, args.batch, args.size, args.size, C_)
        g = torch.Generator().manual_seed(1)
        fcos = spec['meta'] == 'FCOS'
        ch = C_ + (1 if spec.get('classification_loss_type') == 'CrossEntropyLoss' else 0)
        preds = [torch.randn(args.batch, P, ch, generator=g)]
        preds.append(torch.rand(args.batch, P, 4, generator=g) * 60 + 1 if fcos else torch.randn(args.batch, P, 4, generator=g))
        if fcos:
            preds.append(torch.randn(args.batch, P, 1, generator=g))
        preds = [p.to(dev).requires_grad_(True) for p in preds]

        def step():
            for p in preds:
                p.grad = None
            lo = model.get_loss(tuple(preds), ann)
            lo['loss'].backward()
            return lo['loss_values']['loss']

        res = dict(model=name, batch=args.batch, size=args.size, points=P, boxes=int(sum(len(l) for _, l in ann)))
        model.device_targets = False
        res['host_route'] = timed(step, args.iters, args.warmup)
        res['host_route']['loss'] = step()
        model.device_targets = True
        res['device_route'] = timed(step, args.iters, args.warmup)
        res['device_route']['loss'] = step()
        if fcos:
            ranges = [(int(lo), int(hi)) for lo, hi in model._regress_ranges]
            d, total = ops.make_assign_fcos_desc(args.batch, sizes, strides, ranges, C_)
            gt = ops._concat_gt_host(ann, dev)
            res['target_kernel'] = timed_events(lambda: ops._assign_fcos_launch(d, total, gt, dev), args.iters, args.warmup)
            res['targets_from_host'] = timed(lambda: ops.assign_targets_fcos_from_host(sizes, strides, ranges, C_, ann, dev),
                                             args.iters, args.warmup)
        else:
            a = (sizes, strides, model._regression_ranges, model._gray_ranges, C_, model._range_assign_mode,
                 model._regression_loss_type == 'independent')
            d, total = ops.make_assign_desc(args.batch, *a)
            gt = ops._concat_gt_host(ann, dev)
            res['target_kernel'] = timed_events(lambda: ops._assign_v2_launch(d, total, gt, dev), args.iters, args.warmup)
            res['targets_from_host'] = timed(lambda: ops.assign_targets_v2_from_host(*a, ann, dev), args.iters, args.warmup)
        res['speedup'] = res['host_route']['median_ms'] / res['device_route']['median_ms']
        print(json.dumps(res))


if __name__ == '__main__':
    main()
