"""tools/bench_sibling_train.py -- one training iteration of the pyramid siblings: forward, device targets, fused loss, backward
(no optimizer) of FCOS_FPN and LFDV2_SFPN at 640x640, batch 32, 2-6 boxes per image (seeded; the shape of
tools/bench_sibling_loss.py), on the routes a model has:
    head_node      LFD_HIP_HEAD=1: backbone + neck + head as one autograd node (train_engine.DetectorTrainFunction; FCOS_FPN
                   with the FCOSHead glue, LFDV2_SFPN with the LFDHead glue)
    node           LFD_HIP_HEAD=0: the backbone + neck node (train_engine.PyramidTrainFunction), the head under autograd
    autograd_neck  LFD_HIP_NECK=0: the backbone node, neck and head as PyTorch-ROCm modules under autograd, where that route
                   exists -- autograd refuses LFDV2_SFPN's neck (an in-place op on a tensor ReluBackward saved), reported as such.

    python tools/bench_sibling_train.py [--procs 3] [--iters 10] [--rounds 3] [--warmup 3] [--batch 32] [--size 640]

Protocol: every process warms the routes up, then times `--rounds` x (`--iters` iterations of one route, then of the next) --
the routes alternate inside one process, so clock and neighbours hit all alike.  An iteration is timed with device events
(get_loss ends in a host synchronisation by contract).  A process reports its median per route; the parent starts `--procs` fresh
processes one after the other and prints, per model, one JSON line with the median [min - max] of the processes' medians."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'lfd-a-light-and-fast-detector_amd'), os.path.join(ROOT, 'tests', 'golden')):
    sys.path.insert(0, p)

MODELS = ('FCOS_FPN', 'LFDV2_SFPN')
# route -> the environment that selects it (the head switch only moves a model whose head the detector node admits)
ROUTES = {'FCOS_FPN': (('head_node', dict(LFD_HIP_NECK='1', LFD_HIP_HEAD='1')), ('node', dict(LFD_HIP_NECK='1', LFD_HIP_HEAD='0')),
                       ('autograd_neck', dict(LFD_HIP_NECK='0', LFD_HIP_HEAD='0'))),
          'LFDV2_SFPN': (('head_node', dict(LFD_HIP_NECK='1', LFD_HIP_HEAD='1')), ('node', dict(LFD_HIP_NECK='1', LFD_HIP_HEAD='0')),
                         ('autograd_neck', dict(LFD_HIP_NECK='0', LFD_HIP_HEAD='0')))}


def worker(args):
    import torch
    from lfd_amd import configs
    import sibling_cases as SC
    dev = torch.device('cuda:0')
    out = {}
    for name in MODELS:
        spec = configs.SIBLINGS[name]
        model = configs.build_sibling_model(name, seed=1).to(dev).train()
        g = torch.Generator().manual_seed(7)
        x = (torch.rand(args.batch, 3, args.size, args.size, generator=g) * 2 - 1).to(dev)
        ann = SC.synth_annotations(5, args.batch, args.size, args.size, spec['head']['num_classes'])

        def iteration():
            model.zero_grad()
            lo = model.get_loss(model(x), ann)
            lo['loss'].backward()
            return lo['loss_values']['loss']

        routes = {}
        for route, env in ROUTES[name]:
            os.environ.update(env)
            try:
                for _ in range(args.warmup):
                    loss = iteration()
                routes[route] = dict(ms=[], loss=loss)
            except RuntimeError as e:
                if 'inplace' not in str(e):
                    raise
                routes[route] = None          # autograd refuses this neck
                model.zero_grad()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for route, env in ROUTES[name]:
                if routes[route] is None:
                    continue
                os.environ.update(env)
                for _ in range(args.iters):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    iteration()
                    b.record()
                    b.synchronize()
                    routes[route]['ms'].append(a.elapsed_time(b))
        out[name] = {route: (None if r is None else dict(median_ms=statistics.median(r['ms']), min_ms=min(r['ms']), max_ms=max(r['ms']),
                                                         loss=r['loss'])) for route, r in routes.items()}
        del model, x
        torch.cuda.empty_cache()
    print('WORKER ' + json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--procs', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--size', type=int, default=640)
    ap.add_argument('--worker', action='store_true')
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    runs = []
    for _ in range(args.procs):
        cmd = [sys.executable, os.path.abspath(__file__), '--worker'] + [
            '--%s=%d' % (k, getattr(args, k)) for k in ('iters', 'rounds', 'warmup', 'batch', 'size')]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=400)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            sys.exit('a measuring process ended with status %d: nothing more is started' % r.returncode)
        runs.append(json.loads([l for l in r.stdout.splitlines() if l.startswith('WORKER ')][-1][7:]))
    for name in MODELS:
        line = dict(model=name, batch=args.batch, size=args.size, procs=args.procs, iters_per_route=args.iters * args.rounds)
        for route, _ in ROUTES[name]:
            rs = [r[name][route] for r in runs]
            if any(v is None for v in rs):
                line[route] = 'refused by autograd'
                continue
            meds = [v['median_ms'] for v in rs]
            line[route] = dict(median_ms=round(statistics.median(meds), 3), min_ms=round(min(meds), 3), max_ms=round(max(meds), 3),
                               fastest_iteration_ms=round(min(v['min_ms'] for v in rs), 3), loss=rs[0]['loss'])
        if isinstance(line['node'], dict) and isinstance(line['autograd_neck'], dict):
            a, b = line['node'], line['autograd_neck']
            line['medians_separate'] = a['max_ms'] < b['min_ms'] or b['max_ms'] < a['min_ms']
        if isinstance(line.get('head_node'), dict) and isinstance(line['node'], dict):
            # the head node stays default-on only if its slowest process beats the fastest process of the LFD_HIP_HEAD=0 route
            line['head_node_ranges_separate'] = line['head_node']['max_ms'] < line['node']['min_ms']
        print(json.dumps(line))


if __name__ == '__main__':
    main()
