"""LFDResNet's own presets (lfd_amd.configs.PRESETS: block = stem = body = 'fast' | 'faster' | 'fastest') under SimpleNeck(128) +
LFDHead, 'fp16' mode, frames resident in device memory (NHWC fp16):

    python tools/bench_presets.py [steps] [--no-torch] [--out=FILE]

  * forward time (LFD.forward_resident, graph replay) of the three presets at 8 x 1920x1080 and at 1 x 1920x1080: the median
    HIP-event time of `steps` batches after warm-up, and the 10..90 % spread;
  * per layer that runs on csrc/conv_wide.hip in those forwards (every conv with cin or cout above 128, at the map size and
    batch it has there): the time of one ops.conv2d_nhwc call against one torch.nn.functional.conv2d call (fp16,
    channels_last, bias; + residual add + ReLU as separate torch ops where the layer has them) on the same tensors -- HIP events
    around `reps` back-to-back calls, alternating the two sides, the median of `rounds` such windows divided by `reps`.  These
    are call times (kernel + launch), not profiler kernel times.  The outputs of the two sides are compared first.

Records, no pass / fail gate.  Prints one JSON line; --out=FILE also keeps the results gathered so far in FILE after every
measurement (a run that is cut short leaves what it had)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'lfd-a-light-and-fast-detector_amd')):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from lfd_amd import configs, engine, engine_sibling, ops  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith('--')]
steps = int(args[0]) if args else 50
H, W = 1080, 1920
REPS, ROUNDS = 40, 9
assert torch.cuda.is_available(), 'bench_presets.py measures on the GPU'
res = dict(workload='LFDResNet presets + SimpleNeck(128) + LFDHead, %dx%d NHWC fp16 frames, forward_resident, graph replay' % (W, H),
           steps=steps, forward_ms={}, wide_layers=[])


OUT = ([a[len('--out='):] for a in sys.argv[1:] if a.startswith('--out=')] or [None])[0]


def save():
    if OUT:
        json.dump(res, open(OUT, 'w'), indent=1)


def window_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


layers = {}
with torch.no_grad():
    for mode in ('fast', 'faster', 'fastest'):
        m = configs.build_model(configs.PRESETS['%s_%s_%s' % (mode, mode, mode)])
        configs.perturb_weights(m)
        m.eval().cuda()
        for bs in (8, 1):
            x = (torch.rand(bs, H, W, 3, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1)) * 2 - 1).half()
            m.use_graph = True
            for _ in range(3):
                m.forward_resident(x)
            torch.cuda.synchronize()
            ts = [window_ms(lambda: m.forward_resident(x), 1) for _ in range(steps)]
            res['forward_ms']['%s bs%d' % (mode, bs)] = dict(median=round(float(np.median(ts)), 4),
                                                             spread_10_90=round(float(np.percentile(ts, 90) - np.percentile(ts, 10)), 4))
            # the layers of this forward that run on the wide kernel, at their map sizes
            sp = engine_sibling.get_plan(m, m._backbone, m._neck, m._head, x.device)
            st = sp.bb_plan.state_for(bs, H, W)
            for c in sp.bb_plan.convs:
                if engine.wide_conv(c.cin, c.cout, c.ks, c.stride) and max(c.cin, c.cout) > 128:
                    layers.setdefault((bs, st.bufs[c.src].shape[1], st.bufs[c.src].shape[2], c.cin, c.cout, c.ks, c.stride, c.res is not None,
                                       bool(c.relu)), mode)
            for t in sp.bb_plan.taps:
                if st.bufs[t].shape[-1] > 128:
                    layers.setdefault((bs, st.bufs[t].shape[1], st.bufs[t].shape[2], st.bufs[t].shape[-1], 128, 1, 1, False, True), mode)
            save()
            del x
        del m
        torch.cuda.empty_cache()

    if '--no-torch' not in sys.argv:
        g = torch.Generator(device='cuda').manual_seed(2)
        for (bs, h, w, cin, cout, ks, stride, has_res, relu), mode in sorted(layers.items()):
            x = (torch.randn(bs, h, w, cin, device='cuda', generator=g) * 0.5).half()
            wt = (torch.randn(cout, cin, ks, ks, device='cuda', generator=g) * (1.0 / (cin * ks * ks) ** 0.5)).half()
            b = torch.randn(cout, device='cuda', generator=g) * 0.1
            wp = ops.pack_conv_weight(wt.float()).cuda()
            oh, ow = (h + 2 * (ks // 2) - ks) // stride + 1, (w + 2 * (ks // 2) - ks) // stride + 1
            r = (torch.randn(bs, oh, ow, cout, device='cuda', generator=g) * 0.5).half() if has_res else None
            out = torch.empty((bs, oh, ow, cout), dtype=torch.float16, device='cuda')
            xt = x.permute(0, 3, 1, 2)                       # NCHW view of the NHWC storage = channels_last
            wtc = wt.contiguous(memory_format=torch.channels_last)
            bh = b.half()
            rt = r.permute(0, 3, 1, 2) if has_res else None

            def ours():
                return ops.conv2d_nhwc(x, wp, b, cin, cout, ks, stride, relu, residual=r, out=out)

            def theirs():
                y = F.conv2d(xt, wtc, bh, stride=stride, padding=ks // 2)
                if has_res:
                    y = y + rt
                return y.relu_() if relu else y

            a, t = ours().float(), theirs().permute(0, 2, 3, 1).float()
            err = float((a - t).abs().max())
            for _ in range(2):
                window_ms(ours, REPS)
                window_ms(theirs, REPS)
            to, tt = [], []
            for _ in range(ROUNDS):
                to.append(window_ms(ours, REPS))
                tt.append(window_ms(theirs, REPS))
            res['wide_layers'].append(dict(preset=mode, n=bs, h=h, w=w, cin=cin, cout=cout, ks=ks, stride=stride, residual=has_res,
                                           hip_us=round(1e3 * float(np.median(to)), 2), torch_us=round(1e3 * float(np.median(tt)), 2),
                                           hip_spread_us=round(1e3 * float(max(to) - min(to)), 2),
                                           torch_spread_us=round(1e3 * float(max(tt) - min(tt)), 2), max_abs_diff=round(err, 5)))
            save()
print(json.dumps(res))
