"""tools/bench_loss_pairs.py -- the fused get_loss of the loss pairs beyond Focal / CrossEntropy + IoU (csrc/getloss_ex.hip)
against the op-by-op route it replaces, `LFD_FUSED_LOSS_EX` 1 against 0 (the sibling of tools/bench_sibling_loss.py, which times
the device targets).  Rows, at 640x640, batch 32:
    LFDV2_SFPN loss        get_loss + backward to the prediction gradients on fixed predictions (Focal + GIoU, LFDv2 targets)
    TL_LFD_L loss          the same for a TrafficLight configuration (QualityFocal + IoU)
    LFDV2_SFPN iteration   forward, device targets, loss, backward -- the iteration of tools/bench_sibling_train.py
    TL_LFD_L train_step    the eager lfd_amd.train.train_step of tools/bench_train.py --model TL_LFD_L (clip + SGD included)

    python tools/bench_loss_pairs.py [--procs 3] [--iters 10] [--rounds 3] [--warmup 3] [--batch 32] [--size 640]

Protocol (tools/bench_sibling_train.py): a process warms both routes up, then times `--rounds` x (`--iters` iterations with the
switch on, then off), device events around each iteration (get_loss ends in a host synchronisation by contract); it reports its
median per route.  The parent starts `--procs` fresh processes one after the other and prints one JSON line per row: median
[min - max] of the processes' medians per route, and `ranges_separate` -- the slowest process of the fused route beats the
fastest process of the op-by-op route.

Kernel times and launch counts come from a trace, in a run of its own:
    rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python tools/bench_loss_pairs.py --trace LFDV2_SFPN --ex 1
    python tools/bench_loss_pairs.py --summarise DIR/.../NAME_kernel_trace.csv --trace LFDV2_SFPN
`--trace` runs `--warmup` + `--iters` iterations of the model's iteration row; `--summarise` prints the launches per iteration
(all launches of the timed iterations / `--iters`) and, for the two row kernels, the bytes the algorithm needs (computed from
the shapes, below) over the kernel time."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'lfd-a-light-and-fast-detector_amd'), os.path.join(ROOT, 'tests', 'golden')):
    sys.path.insert(0, p)

ROWS = ('LFDV2_SFPN loss', 'TL_LFD_L loss', 'LFDV2_SFPN iteration', 'TL_LFD_L train_step')
ROUTES = (('fused', '1'), ('op_by_op', '0'))      # route -> LFD_FUSED_LOSS_EX


def level_sizes(strides, size):
    return [((size + s - 1) // s, (size + s - 1) // s) for s in strides]


def row_kernel_bytes(rows, channels, num_classes):
    """bytes the two row kernels need: the sums pass reads every row's logits, regression outputs, class targets and
    regression targets once; the backward reads the same and writes d cls and d reg"""
    read = rows * (channels + 4 + num_classes + 4) * 4
    return dict(partial=read, bwd=read + rows * (channels + 4) * 4)


def build(name, args, dev):
    """-> (callable running one iteration of the row, geometry dict)"""
    import torch
    from lfd_amd import configs, optim, train
    import sibling_cases as SC
    model_name, kind = name.split(' ')
    sibling = model_name in configs.SIBLINGS
    model = (configs.build_sibling_model(model_name, seed=1) if sibling else configs.build_model(model_name)).to(dev).train()
    C_ = model._num_classes
    ann = SC.synth_annotations(5, args.batch, args.size, args.size, C_)
    sizes = level_sizes(list(model._point_strides), args.size)
    P = sum(h * w for h, w in sizes)
    ch = C_ + (1 if model._is_ce() else 0)
    geo = dict(points=P, rows=args.batch * P, channels=ch, num_classes=C_, boxes=int(sum(len(l) for _, l in ann)))
    if kind == 'loss':
        for i, hw in enumerate(sizes):
            model._head_indexes_to_feature_map_sizes[i] = hw
        g = torch.Generator().manual_seed(1)
        preds = [torch.randn(args.batch, P, ch, generator=g).to(dev).requires_grad_(True),
                 torch.randn(args.batch, P, 4, generator=g).to(dev).requires_grad_(True)]

        def step():
            for p in preds:
                p.grad = None
            lo = model.get_loss(tuple(preds), ann)
            lo['loss'].backward()
            return lo['loss_values']['loss']
        return step, geo, model
    g = torch.Generator().manual_seed(7)
    x = (torch.rand(args.batch, 3, args.size, args.size, generator=g) * 2 - 1).to(dev)
    if kind == 'iteration':
        def step():
            model.zero_grad()
            lo = model.get_loss(model(x), ann)
            lo['loss'].backward()
            return lo['loss_values']['loss']
        return step, geo, model
    opt = optim.SGD(model.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    clip = dict(max_norm=10, norm_type=2)
    return (lambda: train.train_step(model, opt, x, ann, clip, True)[0]['loss']), geo, model


def worker(args):
    import torch
    dev = torch.device('cuda:0')
    out = {}
    for name in ROWS:
        step, geo, model = build(name, args, dev)
        res = {}
        for route, ex in ROUTES:
            os.environ['LFD_FUSED_LOSS_EX'] = ex
            for _ in range(args.warmup):
                loss = step()
            res[route] = dict(ms=[], loss=loss, took=model.last_loss_route)
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for route, ex in ROUTES:
                os.environ['LFD_FUSED_LOSS_EX'] = ex
                for _ in range(args.iters):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    step()
                    b.record()
                    b.synchronize()
                    res[route]['ms'].append(a.elapsed_time(b))
        out[name] = dict(geometry=geo, **{route: dict(median_ms=statistics.median(r['ms']), min_ms=min(r['ms']), max_ms=max(r['ms']),
                                                     loss=r['loss'], took=r['took']) for route, r in res.items()})
        del step, model
        torch.cuda.empty_cache()
    print('WORKER ' + json.dumps(out))


def trace(args):
    import torch
    os.environ['LFD_FUSED_LOSS_EX'] = str(args.ex)
    step, geo, model = build(args.trace + (' iteration' if args.trace in ('LFDV2_SFPN',) else ' train_step'), args, torch.device('cuda:0'))
    for _ in range(args.warmup + args.iters):
        step()
    torch.cuda.synchronize()
    print(json.dumps(dict(trace=args.trace, ex=args.ex, took=model.last_loss_route, warmup=args.warmup, iters=args.iters, **geo)))


def summarise(args):
    import csv
    rows = list(csv.DictReader(open(args.summarise)))
    ev = sorted(((int(r['Start_Timestamp']), int(r['End_Timestamp']), r['Kernel_Name']) for r in rows), key=lambda t: t[0])
    # every iteration of either route launches the target-assignment kernel exactly once: the launches between two
    # consecutive ones are one iteration; the timed iterations are the last `iters` of the trace
    marks = [i for i, e in enumerate(ev) if 'k_assign' in e[2]]
    assert len(marks) == args.warmup + args.iters, (len(marks), args.warmup, args.iters)
    per = [marks[i + 1] - marks[i] for i in range(len(marks) - args.iters - 1, len(marks) - 1)]
    out = dict(trace=args.trace, launches_in_trace=len(ev), launches_per_iteration=statistics.median(per),
               launches_per_iteration_range=[min(per), max(per)])
    from lfd_amd import configs
    model = configs.build_sibling_model(args.trace, seed=1) if args.trace in configs.SIBLINGS else configs.build_model(args.trace)
    P = sum(h * w for h, w in level_sizes(list(model._point_strides), args.size))
    ch = model._num_classes + (1 if model._is_ce() else 0)
    need = row_kernel_bytes(args.batch * P, ch, model._num_classes)
    for key, pat in (('partial', 'k_lossx_partial'), ('bwd', 'k_lossx_bwd')):
        d = [e[1] - e[0] for e in ev if pat in e[2]][-args.iters:]
        if d:
            us = statistics.median(d) / 1e3
            out[key] = dict(calls=len(d), median_us=round(us, 2), bytes=need[key], tb_per_s=round(need[key] / (us * 1e-6) / 1e12, 3))
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--procs', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--worker', action='store_true')
    ap.add_argument('--trace', default=None, help='LFDV2_SFPN | TL_LFD_L: run warmup + iters iterations and exit (under rocprofv3)')
    ap.add_argument('--ex', type=int, default=1, choices=(0, 1), help='LFD_FUSED_LOSS_EX of a --trace run')
    ap.add_argument('--summarise', default=None, help='kernel_trace.csv of a --trace run (give the same --trace / sizes)')
    args = ap.parse_args()
    if args.summarise:
        return summarise(args)
    if args.trace:
        return trace(args)
    if args.worker:
        return worker(args)
    runs = []
    for _ in range(args.procs):
        cmd = [sys.executable, os.path.abspath(__file__), '--worker'] + [
            '--%s=%d' % (k, getattr(args, k)) for k in ('iters', 'rounds', 'warmup', 'batch', 'size')]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=500)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit('a measuring process ended with status %d: nothing more is started' % r.returncode)
        runs.append(json.loads([l for l in r.stdout.splitlines() if l.startswith('WORKER ')][-1][7:]))
    for name in ROWS:
        line = dict(row=name, batch=args.batch, size=args.size, procs=args.procs, iters_per_route=args.iters * args.rounds,
                    **runs[0][name]['geometry'])
        for route, _ in ROUTES:
            rs = [r[name][route] for r in runs]
            meds = [v['median_ms'] for v in rs]
            line[route] = dict(median_ms=round(statistics.median(meds), 3), min_ms=round(min(meds), 3), max_ms=round(max(meds), 3),
                               fastest_iteration_ms=round(min(v['min_ms'] for v in rs), 3), loss=rs[0]['loss'], took=rs[0]['took'])
        line['ranges_separate'] = line['fused']['max_ms'] < line['op_by_op']['min_ms']
        line['speedup'] = round(line['op_by_op']['median_ms'] / line['fused']['median_ms'], 3)
        print(json.dumps(line))


if __name__ == '__main__':
    main()
