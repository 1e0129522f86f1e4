"""The torchvision-style ResNet-18 / 34 backbone on the fp16 inference path (lfd_amd.configs.RESNET_SIBLINGS), frames resident
in device memory (NHWC fp16, 1920 x 1080):

    python tools/bench_resnet.py [steps] [--no-torch] [--out=FILE]

  * forward time of R18_FCOS_FPN and R34_LFDV2_SFPN (engine_sibling.sibling_forward, graph replay) at 8 x and 1 x 1080p: the
    median HIP-event time of `steps` batches after warm-up, and the 10..90 % spread;
  * the backbone alone (ResNetPlan.run_backbone, eager launches) against the same module's own torch forward in fp16
    channels_last on the same frames -- ResNet.forward is plain torch ops, so this is PyTorch-ROCm (MIOpen) on the same weights;
  * lfd_stem7_conv_f16 and the max-pool behind it on their own against F.conv2d + ReLU / F.max_pool2d (fp16, channels_last) on
    the same tensors: microseconds per call and achieved GB/s (bytes read + bytes written; the stem conv is write-bound:
    531 MB out for 50 MB in at 8 x 1080p).
  The pairs follow tools/bench_presets.py: HIP events around `reps` back-to-back calls, alternating the two sides, the median of
  `rounds` such windows divided by `reps` -- call times (kernel + launch), not profiler kernel times; outputs compared first.

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
from lfd_amd import _lib, configs, engine, engine_sibling  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith('--')]
steps = int(args[0]) if args else 50
H, W = 1080, 1920
REPS, ROUNDS = 20, 9
TORCH = '--no-torch' not in sys.argv
OUT = ([a[len('--out='):] for a in sys.argv[1:] if a.startswith('--out=')] or [None])[0]
assert torch.cuda.is_available(), 'bench_resnet.py measures on the GPU'
res = dict(workload='ResNet-18 / 34 models, %dx%d NHWC fp16 frames' % (W, H), steps=steps, forward_ms={}, backbone_ms={}, stem={})


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


def pair(ours, theirs, reps=REPS):
    """-> (median ms of ours, of theirs | None, spreads) over alternating windows"""
    sides = [ours] + ([theirs] if theirs is not None else [])
    for _ in range(2):
        for f in sides:
            window_ms(f, reps)
    ts = [[] for _ in sides]
    for _ in range(ROUNDS):
        for k, f in enumerate(sides):
            ts[k].append(window_ms(f, reps))
    return [(float(np.median(t)), float(max(t) - min(t))) for t in ts]


with torch.no_grad():
    for name in ('R18_FCOS_FPN', 'R34_LFDV2_SFPN'):
        m = configs.build_resnet_model(name)
        m.eval()
        m.cuda()
        bb = m._backbone
        tb = copy.deepcopy(bb).half().to(memory_format=torch.channels_last) if TORCH else None
        for bs in (8, 1):
            x = (torch.rand(bs, H, W, 3, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1)) * 2 - 1).half()
            for _ in range(3):
                engine_sibling.sibling_forward(m, x, use_graph=True)
            torch.cuda.synchronize()
            ts = [window_ms(lambda: engine_sibling.sibling_forward(m, x, use_graph=True), 1) for _ in range(steps)]
            res['forward_ms']['%s bs%d' % (name, bs)] = dict(median=round(float(np.median(ts)), 4),
                                                            spread_10_90=round(float(np.percentile(ts, 90) - np.percentile(ts, 10)), 4))
            save()
            # ---- the backbone alone, eager, against its own torch forward
            sp = engine_sibling.get_plan(m, bb, m._neck, m._head, x.device)
            plan = sp.bb_plan
            st = plan.state_for(bs, H, W)
            xt = x.permute(0, 3, 1, 2)               # NCHW view of the NHWC storage = channels_last
            theirs = (lambda: tb(xt)) if TORCH else None
            if TORCH:
                plan.run_backbone(x, engine.IN_NHWC_F16, st)
                taps = tb(xt)
                err = max(float((st.bufs[t].float() - y.permute(0, 2, 3, 1).float()).abs().max() / y.float().abs().max())
                          for t, y in zip(plan.taps, taps))
                del taps
            got = pair(lambda: plan.run_backbone(x, engine.IN_NHWC_F16, st), theirs, reps=5)
            ent = dict(hip_ms=round(got[0][0], 4), hip_spread_ms=round(got[0][1], 4), launches=2 + len(plan.convs))
            if TORCH:
                ent.update(torch_ms=round(got[1][0], 4), torch_spread_ms=round(got[1][1], 4), max_rel_tap_diff=round(err, 5))
            res['backbone_ms']['ResNet-%d bs%d' % (bb.depth, bs)] = ent
            save()
            # ---- the stem conv and the pool on their own (once per batch size: the same layer in both depths)
            if name == 'R18_FCOS_FPN':
                y, p = st.bufs[plan.stem_out], st.bufs[plan.pool_out]
                wp, b7 = plan.stem7
                l, sptr = _lib.lib(), _lib.stream_ptr()

                def stem():
                    _lib.check(l.lfd_stem7_conv_f16(_lib.ptr(x), 1, bs, H, W, _lib.ptr(wp), _lib.ptr(b7), _lib.ptr(y), sptr), 'lfd_stem7_conv_f16')

                def pool():
                    _lib.check(l.lfd_maxpool3x3s2_nhwc_f16(_lib.ptr(y), _lib.ptr(p), bs, y.shape[1], y.shape[2], 64, sptr), 'lfd_maxpool3x3s2_nhwc_f16')

                (_, _, w7, bias7), = plan.stem_ref
                wt = w7.half().contiguous(memory_format=torch.channels_last)
                bh = bias7.half()
                stem()
                yt = y.permute(0, 3, 1, 2)
                t_stem = (lambda: F.conv2d(xt, wt, bh, stride=2, padding=3).relu_()) if TORCH else None
                t_pool = (lambda: F.max_pool2d(yt, 3, 2, 1)) if TORCH else None
                for tag, ours, theirs, nbytes in (('stem7', stem, t_stem, x.numel() * 2 + y.numel() * 2),
                                                  ('maxpool', pool, t_pool, y.numel() * 2 + p.numel() * 2)):
                    got = pair(ours, theirs)
                    ent = dict(hip_us=round(1e3 * got[0][0], 2), hip_spread_us=round(1e3 * got[0][1], 2),
                               hip_GBps=round(nbytes / (got[0][0] * 1e-3) / 1e9, 1), MB=round(nbytes / 1e6, 1))
                    if TORCH:
                        ent.update(torch_us=round(1e3 * got[1][0], 2), torch_spread_us=round(1e3 * got[1][1], 2),
                                   torch_GBps=round(nbytes / (got[1][0] * 1e-3) / 1e9, 1))
                        if tag == 'stem7':
                            ent['max_abs_diff'] = round(float((y.float() - t_stem().permute(0, 2, 3, 1).float()).abs().max()), 5)
                    res['stem']['%s bs%d' % (tag, bs)] = ent
                    save()
            del x, xt, st
            plan._shape_cache.clear()
            torch.cuda.empty_cache()
        del m, tb
        torch.cuda.empty_cache()
print(json.dumps(res))
