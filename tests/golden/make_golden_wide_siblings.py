"""tests/golden/make_golden_wide_siblings.py -- regenerates wide_sibling_<CASE>.npz: the REAL reference classes (imported
through oracle/ref_import.py) in the 256-channel compositions of lfd_amd.configs.WIDE_SIBLINGS, run on the CPU.

    python tests/golden/make_golden_wide_siblings.py            # writes the fixtures
    python tests/golden/make_golden_wide_siblings.py --check    # regenerates and compares with the committed files

Weights are NOT stored: configs.synthetic_weights(seed=1) draws them per state_dict key; the sha256 of the reference state_dict
(make_golden_siblings.state_sha) and its key / shape list are.  Inputs are NOT stored either: frame(shape, seed) below draws
them, rounded to fp16 values (so the fp32 NCHW and the fp16 NHWC frame are the same operand).  Shapes: 2 x 3 x 128 x 160 for
both, 1 x 3 x 101 x 150 for R18_FCOS_FPN256 (a file of its own, suffix '_odd').

Stored per file: the level-concatenated forward tensors cls / reg (/ ctr) with all 80 classes of the FCOS entry (they fit: 274 KB
of the file), the level sizes, get_results for two metas at the 0.9 quantile of the scores (JSON rows), and every backbone tap
and neck output SAMPLED -- every cs-th channel and s-th row and column (sample_steps: at most 2048 values per map) -- which is
what keeps a file near the 250-370 KB of the narrow sibling fixtures.  The neck outputs are what the neck returns, i.e. with
the in-place ReLU in front of a conv extra level already applied to the level it reads (fpn.py:66-79).
"""
import json
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'lfd-a-light-and-fast-detector_amd'))
sys.path.insert(0, HERE)
warnings.filterwarnings('ignore')

from lfd_amd import configs  # noqa: E402

SHAPES = {'': ((2, 128, 160), 7), '_odd': ((1, 101, 150), 8)}        # suffix -> (n, h, w), seed
ODD_CASES = ('R18_FCOS_FPN256',)
MAP_VALUES = 2048
RESULTS_IOU = 0.45


def frame(shape, seed):
    n, h, w = shape
    return (torch.rand(n, 3, h, w, generator=torch.Generator().manual_seed(seed)) * 2 - 1).half().float()


def sample_steps(shape):
    """(channel step, pixel step) of a stored [n, c, h, w] map: the smallest channel step, then the smallest pixel step"""
    n, c, h, w = shape
    for cs in (1, 2, 4, 8, 16, 32, 64):
        for s in (1, 2, 4):
            if n * -(-c // cs) * -(-h // s) * -(-w // s) <= MAP_VALUES:
                return cs, s
    raise ValueError(shape)


def sample(t):
    cs, s = sample_steps(t.shape)
    return t[:, ::cs, ::s, ::s].contiguous()


def key_shapes(sd):
    return json.dumps([[k, list(v.shape)] for k, v in sd.items()])


def generate(name, suffix):
    from oracle import ref_import
    from make_golden_siblings import state_sha
    M = ref_import.import_reference()
    import lfd.model.backbone as RB
    import lfd.model.head as RH
    import lfd.model.losses as RL
    import lfd.model.neck as RN
    model = configs.build_wide_sibling(name, RB, RN, RH, M, RL, seed=1)
    sd = model.state_dict()
    shape, seed = SHAPES[suffix]
    n, h, w = shape
    out = dict(sha=state_sha(sd), keys=key_shapes(sd), shape=np.array(shape), x_seed=seed)
    model.eval()
    x = frame(shape, seed)
    with torch.no_grad():
        taps = model._backbone(x)
        feats = model._neck(taps)
        outs = model(x)
    for nm, t in zip(('cls', 'reg', 'ctr'), outs):
        out[nm] = t.numpy()
    out['sizes'] = np.array([model.head_indexes_to_feature_map_sizes[i] for i in range(len(model._point_strides))])
    for tag, maps in (('tap', taps), ('neck', feats)):
        out[tag + '_shapes'] = np.array([t.shape for t in maps])
        out[tag + '_steps'] = np.array([sample_steps(t.shape) for t in maps])
        for i, t in enumerate(maps):
            out['%s%d' % (tag, i)] = sample(t).numpy()
    sc = outs[0].sigmoid() * outs[2].sigmoid() if len(outs) == 3 else outs[0].sigmoid()
    thr = float(np.quantile(sc.numpy(), 0.9))
    model._classification_threshold = thr
    model._nms_cfg = dict(type='nms', iou_thr=RESULTS_IOU)
    out['results_thr'], out['results_iou'] = thr, RESULTS_IOU
    out['results'] = json.dumps(model.get_results(outs, [dict(resized_height=h, resized_width=w, resize_scale=1.0)] * n))
    out['results_scaled'] = json.dumps(model.get_results(outs, [dict(resized_height=h - 6, resized_width=w - 10, resize_scale=0.5)] * n))
    return out


def main():
    check = '--check' in sys.argv
    bad = 0
    for name in configs.WIDE_SIBLINGS:
        for suffix in SHAPES:
            if suffix and name not in ODD_CASES:
                continue
            out = generate(name, suffix)
            path = os.path.join(HERE, 'wide_sibling_%s%s.npz' % (name, suffix))
            if check:
                old = np.load(path)
                same = sorted(old.files) == sorted(out) and all(np.array_equal(old[k], out[k]) for k in out)
                print(name + suffix, 'identical' if same else 'DIFFERS')
                bad += not same
            else:
                np.savez_compressed(path, **out)
                print(name + suffix, '%d KiB' % (os.path.getsize(path) // 1024), 'results',
                      [len(r) for r in json.loads(out['results'])])
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
