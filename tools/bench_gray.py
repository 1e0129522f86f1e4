"""Grayscale (input_channels=1) against RGB frames on the headline workload: WIDERFACE_LFD_S, 8 x 1920x1080, forward only
(LFD.forward_resident on frames resident in device memory), both precision modes, fp16 and uint8 NHWC frames.

    python tools/bench_gray.py [steps] [--eager]

Per (mode, dtype): the median HIP-event time of a batch for the gray twin and for the RGB model (same seed, same weights
apart from the first conv), interleaved so both see the same machine state.  Graph replay by default (the bench's setting);
--eager launches every kernel (for rocprofv3 --kernel-trace --stats, where each launch is a trace row).  Prints one JSON line."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'lfd-a-light-and-fast-detector_amd')):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from lfd_amd import configs  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith('--')]
steps = int(args[0]) if args else 20
graph = '--eager' not in sys.argv
BS, H, W = 8, 1080, 1920
assert torch.cuda.is_available(), 'bench_gray.py measures on the GPU'


def model(cin):
    m = configs.build_model('WIDERFACE_LFD_S', input_channels=cin)
    configs.perturb_weights(m)
    m.eval().cuda()
    m.use_graph = graph
    return m


def frames(cin, dtype):
    g = torch.Generator(device='cuda').manual_seed(1)
    if dtype == 'uint8':
        return torch.randint(0, 256, (BS, H, W, cin), device='cuda', generator=g, dtype=torch.uint8)
    return (torch.rand(BS, H, W, cin, device='cuda', generator=g) * 2 - 1).half()


def batch_ms(m, x):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    m.forward_resident(x)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


res = dict(workload='WIDERFACE_LFD_S %d x %dx%d forward_resident, %s' % (BS, W, H, 'graph replay' if graph else 'eager launches'),
           steps=steps)
models = {1: model(1), 3: model(3)}
with torch.no_grad():
    for mode in ('fp16', 'fp32_storage'):
        for dtype in ('float16', 'uint8'):
            xs = {c: frames(c, dtype) for c in (1, 3)}
            for c in (1, 3):
                models[c].precision = mode
                for _ in range(3):
                    models[c].forward_resident(xs[c])
            torch.cuda.synchronize()
            ts = {1: [], 3: []}
            for _ in range(steps):
                for c in (1, 3):
                    ts[c].append(batch_ms(models[c], xs[c]))
            g, r = float(np.median(ts[1])), float(np.median(ts[3]))
            res['%s_%s' % (mode, dtype)] = dict(gray_ms=round(g, 4), rgb_ms=round(r, 4), gray_minus_rgb_ms=round(g - r, 4),
                                                gray_spread_ms=round(float(np.percentile(ts[1], 90) - np.percentile(ts[1], 10)), 4),
                                                rgb_spread_ms=round(float(np.percentile(ts[3], 90) - np.percentile(ts[3], 10)), 4))
            del xs
            torch.cuda.empty_cache()
print(json.dumps(res))
