"""The 256-channel siblings on the fp16 inference path (lfd_amd.configs.WIDE_SIBLINGS), frames resident in device memory (NHWC
fp16, 1920 x 1080):

    python tools/bench_wide_siblings.py [steps] [--no-torch] [--no-models] [--no-layer] [--out=FILE]

  * the 3x3 stride-1 256 -> 256 conv alone (the tower / FPN output layer) on the five FCOS level maps of 8 x 1080p -- 135x240,
    68x120, 34x60, 17x30, 9x15 -- through three routes: lfd_conv256_nhwc_f16 (csrc/conv256.hip), lfd_conv2d_nhwc_f16
    (csrc/conv_wide.hip) and torch's fp16 channels_last conv on the same tensors.  The protocol of tools/bench_presets.py /
    bench_resnet.py: HIP events around `reps` back-to-back calls, the routes alternating, ROUNDS windows each; per route the
    median microseconds per call, [min .. max] of the windows and PFLOP/s (2 * 2304 * 256 FLOP per output pixel) at the median.
    `conv256_below_wide` says whether EVERY conv256 window lies below EVERY conv_wide window (`wide_below_conv256`: the
    converse).  Call times (kernel + launch), outputs compared first;
  * forward time of both models (engine_sibling.sibling_forward, graph replay) at 8 x and 1 x 1080p, the median HIP-event time
    of `steps` batches after warm-up and the 10..90 % spread (no parent figure exists: these models do not run without
    csrc/conv256.hip's fp32-output form); R18_FCOS_FPN256 next to the fp16 channels_last forward of the same modules as plain
    torch ops (eager).  LFDV2_SFPN256 has no torch figure: this package's LFDResNet is a parameter container without a torch
    forward.

Records, no pass / fail gate.  Prints one JSON line; --out=FILE also keeps the results gathered so far after every measurement."""
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'lfd-a-light-and-fast-detector_amd')):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from lfd_amd import configs, engine_sibling, ops  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith('--')]
steps = int(args[0]) if args else 30
H, W = 1080, 1920
ROUNDS = 7
TORCH = '--no-torch' not in sys.argv
OUT = ([a[len('--out='):] for a in sys.argv[1:] if a.startswith('--out=')] or [None])[0]
LEVEL_MAPS = ((135, 240), (68, 120), (34, 60), (17, 30), (9, 15))
assert torch.cuda.is_available(), 'bench_wide_siblings.py measures on the GPU'
res = dict(workload='256-channel FCOS / LFDv2 siblings, %dx%d NHWC fp16 frames' % (W, H), steps=steps,
           crossover_pixels=engine_sibling.CONV256_MIN_PIXELS, layer={}, forward_ms={})


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


def alternate(sides, reps):
    """-> the window times [side][round] of the sides, alternating"""
    for _ in range(2):
        for f in sides:
            window_ms(f, reps)
    ts = [[] for _ in sides]
    for _ in range(ROUNDS):
        for k, f in enumerate(sides):
            ts[k].append(window_ms(f, reps))
    return ts


with torch.no_grad():
    if '--no-layer' not in sys.argv:
        g = torch.Generator(device='cuda').manual_seed(1)
        wt = (torch.randn(256, 256, 3, 3, device='cuda', generator=g) / 48.0)
        bias = torch.randn(256, device='cuda', generator=g) * 0.1
        wp = ops.pack_conv_weight(wt).cuda()
        wcl = wt.half().contiguous(memory_format=torch.channels_last)
        bh = bias.half()
        for h, w in LEVEL_MAPS:
            x = (torch.randn(8, h, w, 256, device='cuda', generator=g) * 0.5).half()
            xt = x.permute(0, 3, 1, 2)
            a = ops.conv256_nhwc(x, wp, bias, 256, 3, relu=False)
            b = ops.conv2d_nhwc(x, wp, bias, 256, 256, 3, 1, False)
            sides = [lambda: ops.conv256_nhwc(x, wp, bias, 256, 3, relu=False, out=a),
                     lambda: ops.conv2d_nhwc(x, wp, bias, 256, 256, 3, 1, False, out=b)]
            names = ['conv256', 'conv_wide']
            ent = dict(pixels=8 * h * w, max_abs_diff_routes=round(float((a.float() - b.float()).abs().max()), 5))
            if TORCH:
                sides.append(lambda: F.conv2d(xt, wcl, bh, padding=1))
                names.append('torch')
                ent['max_abs_diff_torch'] = round(float((a.float() - sides[2]().permute(0, 2, 3, 1).float()).abs().max()), 5)
            flop = 2.0 * 2304 * 256 * 8 * h * w
            ts = alternate(sides, 20 if h < 100 else 5)
            for nm, t in zip(names, ts):
                med = float(np.median(t))
                ent[nm] = dict(us=round(1e3 * med, 2), min_us=round(1e3 * min(t), 2), max_us=round(1e3 * max(t), 2),
                               PFLOPs=round(flop / (med * 1e-3) / 1e15, 4))
            ent['conv256_below_wide'] = bool(max(ts[0]) < min(ts[1]))
            ent['wide_below_conv256'] = bool(max(ts[1]) < min(ts[0]))
            res['layer']['%dx%d' % (h, w)] = ent
            save()
            del x, xt, a, b
        torch.cuda.empty_cache()

    if '--no-models' not in sys.argv:
        for name in sorted(configs.WIDE_SIBLINGS):
            m = configs.build_wide_sibling_model(name)
            m.eval()
            m.cuda()
            tm = None
            if TORCH and 'resnet' in configs.WIDE_SIBLINGS[name]:
                # the same modules as plain torch ops: ResNet.forward is torch; FPN.forward and FCOSHead.forward take their
                # PyTorch-ROCm route in training mode with grad enabled (no BatchNorm in either, GroupNorm has no eval mode,
                # so the arithmetic is the eval forward's); nothing requires grad, so no graph is recorded
                tb, tn, th = (copy.deepcopy(p).half().to(memory_format=torch.channels_last) for p in (m._backbone, m._neck, m._head))
                tb.eval()
                tn.train()
                th.train()
                for p in list(tb.parameters()) + list(tn.parameters()) + list(th.parameters()):
                    p.requires_grad_(False)

                def tm(xt):
                    with torch.enable_grad():
                        return th(tn(tb(xt)))
            for bs in (8, 1):
                x = (torch.rand(bs, H, W, 3, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1)) * 2 - 1).half()
                for _ in range(2):
                    engine_sibling.sibling_forward(m, x, use_graph=True)
                torch.cuda.synchronize()
                ts = [window_ms(lambda: engine_sibling.sibling_forward(m, x, use_graph=True), 1) for _ in range(steps)]
                ent = dict(median=round(float(np.median(ts)), 4),
                           spread_10_90=round(float(np.percentile(ts, 90) - np.percentile(ts, 10)), 4))
                if tm is not None:
                    xt = x.permute(0, 3, 1, 2)
                    for _ in range(2):
                        tm(xt)
                    torch.cuda.synchronize()
                    tt = [window_ms(lambda: tm(xt), 1) for _ in range(max(5, steps // 3))]
                    ent.update(torch_median=round(float(np.median(tt)), 4),
                               torch_spread_10_90=round(float(np.percentile(tt, 90) - np.percentile(tt, 10)), 4))
                    del xt
                res['forward_ms']['%s bs%d' % (name, bs)] = ent
                save()
                del x
                plan = engine_sibling.get_plan(m, m._backbone, m._neck, m._head, torch.device('cuda', torch.cuda.current_device()))
                plan.__dict__.pop('graphs', None)
                getattr(plan.bb_plan, '_shape_cache', {}).clear()
                torch.cuda.empty_cache()
            del m, tm
            torch.cuda.empty_cache()
print(json.dumps(res))
