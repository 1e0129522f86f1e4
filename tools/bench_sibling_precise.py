"""The four configs.SIBLINGS models in 'fp16' against 'fp32_storage', and the fused lateral merge of the latter
(lfd_p32_conv2d_merge_nhwc_f32) against its two-launch route (LFD_P32_MERGE=0): forward time per batch under HIP-graph
replay, HIP-event timed.  The variants of one model are timed in ALTERNATING windows in the same process (other work shares
the host and the device); reported: the median window per variant and the spread (max - min) / median of its windows.
One JSON line per model.  Nothing here is a gate; DESIGN 9i quotes the numbers.

    python tools/bench_sibling_precise.py [--n 8] [--h 720] [--w 1280] [--windows 7] [--reps 20]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'lfd-a-light-and-fast-detector_amd'))
import numpy as np
import torch
from lfd_amd import configs, engine_sibling_p32

VARIANTS = (('fp16', 'fp16', '1'), ('fp32_storage', 'fp32_storage', '1'), ('fp32_storage_two_launch_merge', 'fp32_storage', '0'))


def window(fn, reps):
    """ms per call over `reps` back-to-back replays between two events"""
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=8)
    ap.add_argument('--h', type=int, default=720)
    ap.add_argument('--w', type=int, default=1280)
    ap.add_argument('--windows', type=int, default=7)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--models', default=','.join(sorted(configs.SIBLINGS)))
    a = ap.parse_args()
    dev = torch.device('cuda', 0)
    for name in a.models.split(','):
        x = (torch.rand(a.n, 3, a.h, a.w, generator=torch.Generator().manual_seed(7)) * 2 - 1).to(dev)
        runs = {}
        for key, precision, merge in VARIANTS:
            model = configs.build_sibling_model(name, seed=1).eval().to(dev)      # one model per variant: its own plan and graphs
            if key.endswith('two_launch_merge') and not engine_sibling_p32.covers(model):
                continue                                      # SimpleNeck + LFDHead: engine_p32's plan, no lateral merge
            model.precision = precision
            model.use_graph = True
            fwd = (lambda m=model: m.forward_resident(x)) if hasattr(model, 'forward_resident') else (lambda m=model: m(x))
            runs[key] = (fwd, merge)
        times = {k: [] for k in runs}
        with torch.no_grad():
            for k, (fwd, merge) in runs.items():              # capture + warm-up of every variant before any timing
                os.environ['LFD_P32_MERGE'] = merge
                for _ in range(3):
                    fwd()
            torch.cuda.synchronize()
            for _ in range(a.windows):
                for k, (fwd, merge) in runs.items():
                    os.environ['LFD_P32_MERGE'] = merge
                    times[k].append(window(fwd, a.reps))
        rec = dict(config=name, batch=a.n, input=[a.h, a.w], windows=a.windows, reps_per_window=a.reps)
        for k, ts in times.items():
            med = float(np.median(ts))
            rec[k] = dict(ms_median=round(med, 4), spread=round((max(ts) - min(ts)) / med, 4),
                          images_per_s=round(a.n / (med * 1e-3), 1))
        rec['fp32_storage_over_fp16'] = round(rec['fp32_storage']['ms_median'] / rec['fp16']['ms_median'], 3)
        if 'fp32_storage_two_launch_merge' in rec:
            rec['two_launch_over_fused_merge'] = round(rec['fp32_storage_two_launch_merge']['ms_median']
                                                       / rec['fp32_storage']['ms_median'], 4)
        print(json.dumps(rec), flush=True)
        del runs, x
        torch.cuda.empty_cache()
    os.environ.pop('LFD_P32_MERGE', None)


if __name__ == '__main__':
    main()
