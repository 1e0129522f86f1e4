"""The INT8 calibration rules side by side (lfd_amd/calibration.py, csrc/calib_hist.hip):

    python tools/calib_compare.py [CONFIG[:gray] ...] [--timing-size=1080x1920] [--timing-bs=8] [--no-timing] [--out=FILE]

Accuracy, per shipped configuration of DESIGN 4j's table (default: all four), on the weights and frames of
tests/golden/ref_model_<ARCH>.npz with the calibration set of tests/test_gpu_int8_engine.py (the fixture frames plus four seeded
frames, one frame per batch): one histogram pass, then per rule ('amax', 'percentile' 99.99 / 99.9 / 99, 'entropy', 'mse') the
thresholds, the plan's scales and one forward of the fixture frames:
  * max and RMS of |sigmoid(out) - sigmoid(reference fp32 fixture)| for cls and reg;
  * detections of the fp16 mode found again (IoU >= 0.5, same label, score threshold at the 0.9 quantile of the fp16 scores), as
    DESIGN 4j counts them;
  * how many tensors the rule clips and the largest clipped share.
Timing (first configuration, NHWC fp16 frames of --timing-size, batch --timing-bs; HIP events around `reps` back-to-back calls,
alternating the sides, median of `rounds` windows, max - min as the spread -- call times, not profiler kernel times):
  * per distinct tensor shape of the calibration walk: the histogram kernel (us and GB/s against 2 * rows * c bytes read), the
    same count by torch.bincount on the bit patterns, and the amax reduction Int8Plan.calibrate does;
  * the whole calibration pass, host clock around a device synchronise: Int8Plan.calibrate against calibrate_histograms.

Records, no pass / fail gate.  Prints one JSON line; --out=FILE also keeps the results gathered so far."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'lfd-a-light-and-fast-detector_amd')):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from lfd_amd import calibration, configs, deployment, engine_i8, ops  # noqa: E402


def opt(name, default):
    return ([a[len(name) + 3:] for a in sys.argv[1:] if a.startswith('--%s=' % name)] or [default])[0]


NAMES = [a for a in sys.argv[1:] if not a.startswith('--')] or ['WIDERFACE_LFD_S', 'WIDERFACE_LFD_XS', 'TT100K_LFD_L',
                                                                 'WIDERFACE_LFD_S:gray']
TH, TW = [int(v) for v in opt('timing-size', '1080x1920').split('x')]
TBS = int(opt('timing-bs', '8'))
OUT = opt('out', None)
RULES = [('amax', 'amax', {}), ('percentile99.99', 'percentile', {}), ('percentile99.9', 'percentile', dict(percentile=99.9)),
         ('percentile99', 'percentile', dict(percentile=99.0)), ('entropy', 'entropy', {}), ('mse', 'mse', {})]
REPS, ROUNDS = 10, 7
assert torch.cuda.is_available(), 'calib_compare.py measures on the GPU'
res = dict(workload='INT8 calibration rules: accuracy on the reference fixtures, histogram kernel timing', reps=REPS, rounds=ROUNDS,
           configs={})


def save():
    if OUT:
        json.dump(res, open(OUT, 'w'), indent=1)


def iou(a, b):
    x1, y1 = np.maximum(a[0], b[:, 0]), np.maximum(a[1], b[:, 1])
    x2, y2 = np.minimum(a[0] + a[2], b[:, 0] + b[:, 2]), np.minimum(a[1] + a[3], b[:, 1] + b[:, 3])
    inter = np.clip(x2 - x1, 0, None) * np.clip(y2 - y1, 0, None)
    return inter / (a[2] * a[3] + b[:, 2] * b[:, 3] - inter)


def window_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def sides_ms(*sides, reps=REPS):
    for f in sides:
        window_ms(f, 2)
    ts = [[] for _ in sides]
    for _ in range(ROUNDS):
        for k, f in enumerate(sides):
            ts[k].append(window_ms(f, reps))
    return [(float(np.median(t)), float(max(t) - min(t))) for t in ts]


def accuracy(name, ch):
    g = np.load(os.path.join(ROOT, 'tests', 'golden', ('ref_model_gray_%s.npz' if ch == 1 else 'ref_model_%s.npz') % name))
    m = configs.build_model(name, seed=666, input_channels=ch)
    configs.perturb_weights(m, seed=1)
    m.eval()
    assert deployment.state_sha256(m.state_dict()) == str(g['sha'])
    n, h, w = [int(v) for v in g['shape']]
    x = torch.rand(n, ch, h, w, generator=torch.Generator().manual_seed(int(g['x_seed']))) * 2 - 1
    extra = torch.rand(4, ch, h, w, generator=torch.Generator().manual_seed(1234)) * 2 - 1
    m.cuda()
    data = torch.cat([x, extra])
    plan = engine_i8.Int8Plan(m._backbone, m._neck, m._head, torch.device('cuda', torch.cuda.current_device()))
    hists = plan.calibrate_histograms(data[i:i + 1].cuda() for i in range(data.shape[0]))
    xc = x.cuda()
    ref16 = m(xc)
    multi = g['cls'].shape[2] != 1
    scores16 = (ref16[0].softmax(-1)[..., :-1] if multi else ref16[0].sigmoid()).cpu().numpy()
    meta_rows = [dict(resized_height=h, resized_width=w, resize_scale=1.0)] * n
    old = m._classification_threshold
    m._classification_threshold = float(np.quantile(scores16, 0.9))
    rows16 = m.get_results(ref16, meta_rows)
    out = dict(tensors=len(plan.tensor_names), fp16={})
    for o, k in zip(ref16, ('cls', 'reg')):
        d = (o.cpu().sigmoid() - torch.from_numpy(g[k]).sigmoid()).abs().double()
        out['fp16'][k + '_max'], out['fp16'][k + '_rms'] = float(d.max()), float(d.pow(2).mean().sqrt())
    for tag, algorithm, params in RULES:
        t0 = time.time()
        r = calibration.thresholds(hists, algorithm, **params)
        host_s = time.time() - t0
        plan.set_scales(r['threshold'])
        eng = deployment.Int8Engine(m, plan, True)
        outs = eng(xc)
        e = dict(threshold_host_seconds=round(host_s, 3), tensors_clipped=sum(int(v > 0) for v in r['clipped'].values()),
                 largest_clipped_share=max(r['clipped'].values()),
                 smallest_t_over_amax=min(r['threshold'][k] / r['amax'][k] for k in r['amax'] if r['amax'][k] > 0))
        for o, k in zip(outs, ('cls', 'reg')):
            d = (o.cpu().sigmoid() - torch.from_numpy(g[k]).sigmoid()).abs().double()
            e[k + '_max'], e[k + '_rms'] = float(d.max()), float(d.pow(2).mean().sqrt())
        rows8 = eng.get_results(outs, meta_rows)
        found = total = 0
        for r8, r16 in zip(rows8, rows16):
            b8 = np.array(r8, np.float64).reshape(-1, 6)
            for row in r16:
                total += 1
                same = b8[b8[:, 0] == row[0]]
                found += int(len(same) > 0 and float(iou(np.array(row[2:]), same[:, 2:]).max()) >= 0.5)
        e['fp16_detections_found'], e['fp16_detections'], e['own_detections'] = found, total, sum(len(r_) for r_ in rows8)
        out[tag] = e
    m._classification_threshold = old
    return out


def timing(name):
    m = configs.build_model(name)
    configs.perturb_weights(m)
    m.eval().cuda()
    plan = engine_i8.Int8Plan(m._backbone, m._neck, m._head, torch.device('cuda', torch.cuda.current_device()))
    x = (torch.rand(TBS, TH, TW, 3, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1)) * 2 - 1).half()
    tensors = {}

    def see(tname, t, c_real):
        key = 'x'.join(str(v) for v in t.shape) + ' (%d real)' % c_real
        if key not in tensors:
            tensors[key] = (t.contiguous().clone(), c_real)

    plan._calibration_walk([x], see)
    out = dict(frames='%dx%dx%d NHWC fp16' % (TBS, TH, TW), tensors={})
    for key, (t, c_real) in tensors.items():
        hist = torch.zeros(ops.ABS_HIST_BINS, dtype=torch.int64, device='cuda')
        want = torch.bincount((t[..., :c_real].reshape(-1).view(torch.int16) & 0x7fff).int(), minlength=ops.ABS_HIST_BINS)
        assert torch.equal(ops.abs_histogram_f16(t, c_real), want), key
        got = sides_ms(lambda: ops.abs_histogram_f16(t, c_real, out=hist),
                       lambda: torch.bincount((t.view(torch.int16) & 0x7fff).reshape(-1).int(), minlength=ops.ABS_HIST_BINS),
                       lambda: t.float().abs().max())
        nbytes = 2.0 * t.numel()
        out['tensors'][key] = dict(
            elements=t.numel(), zero_share=round(float((t[..., :c_real] == 0).double().mean()), 4),
            hist_us=round(1e3 * got[0][0], 1), hist_spread_us=round(1e3 * got[0][1], 1),
            hist_GBps=round(nbytes / (got[0][0] * 1e-3) / 1e9, 1),
            bincount_us=round(1e3 * got[1][0], 1), bincount_spread_us=round(1e3 * got[1][1], 1),
            amax_us=round(1e3 * got[2][0], 1), amax_spread_us=round(1e3 * got[2][1], 1))
        res['timing'] = out
        save()
        del hist, want
    del tensors

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn([x])
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    wall(plan.calibrate), wall(plan.calibrate_histograms)
    ts = [[], []]
    for _ in range(ROUNDS):
        ts[0].append(wall(plan.calibrate))
        ts[1].append(wall(plan.calibrate_histograms))
    out['pass_ms'] = dict(amax=round(float(np.median(ts[0])), 2), amax_spread=round(max(ts[0]) - min(ts[0]), 2),
                          histogram=round(float(np.median(ts[1])), 2), histogram_spread=round(max(ts[1]) - min(ts[1]), 2))
    return out


with torch.no_grad():
    for spec in NAMES:
        name, ch = (spec.split(':')[0], 1) if spec.endswith(':gray') else (spec, 3)
        res['configs'][spec] = accuracy(name, ch)
        save()
        torch.cuda.empty_cache()
    if '--no-timing' not in sys.argv[1:]:
        res['timing'] = timing(NAMES[0].split(':')[0])
        save()
print(json.dumps(res))
