"""Inference time against the number of classes: what a head with more than 64 output rows (lfd_head_forward_wide_f16) costs in the
'fp16' mode, frames resident in device memory (NHWC fp16, 1920x1080), graph replay -- the protocol of tools/bench_presets.py:

    python tools/bench_classes.py [steps] [--batches=8,1] [--out=FILE]

  * WIDERFACE_LFD_S (merged head) with num_classes 1, 60 (64 final rows, the last narrow head), 61 (the first wide one), 80, 124;
  * TT100K_LFD_S with 80 classes (CrossEntropyLoss: 81 channels, separate towers on two streams);
  * next to them the 80-class WIDERFACE_LFD_S on the two other routes that run it: precision='fp32_storage' (the layer-by-layer
    PrecisePlan), and the layer-by-layer fp16 engine (engine_sibling) that an `Unsupported` fused plan falls back to -- selected
    here by marking the fused plan as not applicable, which is what a build without the wide output pass decides for this model.
Per configuration and batch: LFD.forward_resident and LFD.detect_resident (forward + decode + threshold + NMS; the threshold is
set so that about a thousand candidates per image pass), the median HIP-event time of `steps` calls after warm-up and the 10..90 %
spread.  Records, no pass / fail gate.  Prints one JSON line; --out=FILE keeps what was gathered so far after every measurement."""
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
steps = int(args[0]) if args else 50
BATCHES = [int(b) for b in ([a[len('--batches='):] for a in sys.argv[1:] if a.startswith('--batches=')] or ['8,1'])[0].split(',')]
OUT = ([a[len('--out='):] for a in sys.argv[1:] if a.startswith('--out=')] or [None])[0]
H, W = 1080, 1920
assert torch.cuda.is_available(), 'bench_classes.py measures on the GPU'
res = dict(workload='%dx%d NHWC fp16 frames, forward_resident / detect_resident, graph replay' % (W, H), steps=steps, runs=[])


def save():
    if OUT:
        json.dump(res, open(OUT, 'w'), indent=1)


def call_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ts):
    return dict(median=round(float(np.median(ts)), 4), spread_10_90=round(float(np.percentile(ts, 90) - np.percentile(ts, 10)), 4))


RUNS = [('WIDERFACE_LFD_S', k, 'fp16', 'fused') for k in (1, 60, 61, 80, 124)] + [
    ('TT100K_LFD_S', 80, 'fp16', 'fused'), ('WIDERFACE_LFD_S', 80, 'fp32_storage', 'layers'), ('WIDERFACE_LFD_S', 80, 'fp16', 'layers')]



def measure(m, name, classes, precision, route, bs):
    softmax = configs.ARCHS[name]['classification_loss_type'] == 'CrossEntropyLoss'
    x = (torch.rand(bs, H, W, 3, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1)) * 2 - 1).half()
    meta = torch.tensor([[float(W), float(H), 1.0]] * bs, dtype=torch.float32, device='cuda')
    m.use_graph = True
    for _ in range(3):
        cls, _ = m.forward_resident(x)
    sc = cls[0].softmax(-1)[:, :-1] if softmax else cls[0].sigmoid()
    thr = float(torch.topk(sc.reshape(-1), 1000).values[-1])
    torch.cuda.synchronize()
    fwd = [call_ms(lambda: m.forward_resident(x)) for _ in range(steps)]
    for _ in range(3):
        out = m.detect_resident(x, meta, score_thr=thr)
    torch.cuda.synchronize()
    det = [call_ms(lambda: m.detect_resident(x, meta, score_thr=thr)) for _ in range(steps)]
    counts = out.counts.cpu().numpy()
    return dict(model=name, classes=classes, cls_channels=int(cls.shape[2]), precision=precision, route=route, batch=bs,
                forward_ms=stats(fwd), detect_ms=stats(det), candidates=int(counts[:, 0].max()), kept=int(counts[:, 1].max()))


with torch.no_grad():
    for name, classes, precision, route in RUNS:
        m = configs.build_model(dict(configs.ARCHS[name], num_classes=classes))
        configs.perturb_weights(m)
        m.eval().cuda()
        m.precision = precision
        if precision == 'fp16' and route == 'layers':
            m.__dict__['_fused_ok'] = False          # LFD._fused_plan_ok: the answer of a fused plan that raised Unsupported
        for bs in BATCHES:
            try:
                res['runs'].append(measure(m, name, classes, precision, route, bs))
            except RuntimeError as e:          # a route that does not take the configuration: recorded, the others still run
                res['runs'].append(dict(model=name, classes=classes, precision=precision, route=route, batch=bs, error=str(e)[:200]))
            print(json.dumps(res['runs'][-1]), file=sys.stderr)
            save()
            torch.cuda.empty_cache()
        del m
print(json.dumps(res))
