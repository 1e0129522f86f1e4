"""tests/golden/make_golden_presets.py -- regenerates presets_<CASE>.npz: the REAL reference (imported through
oracle/ref_import.py, as make_golden.py does) built from LFDResNet's own block / stem / body presets (lfd_resnet.py:222-231;
lfd_amd.configs.PRESETS) under SimpleNeck(128) + the WIDERFACE LFDHead, seeded, perturbed, and run on the CPU on a
2 x 3 x 128 x 192 batch.

    python tests/golden/make_golden_presets.py            # writes the fixtures
    python tests/golden/make_golden_presets.py --check    # regenerates and compares with the committed files

Weights are NOT stored: torch.manual_seed(666) + lfd_amd.configs.perturb_weights(seed=1) regenerate them (the convention of
make_golden.py); the sha256 of the reference state_dict is stored so a drift in init order or RNG is detected instead of
silently changing the inputs.  Stored: that sha256, the input as uint8 codes k (x = k / 128 - 1: every value an fp16, so the
engine's first rounding is not part of what is measured), cls / reg, and the five tapped backbone maps -- sampled every
s-th row and column (s = the smallest of 1, 2, 4, 8 that leaves at most 16384 values, tap_step) to keep a fixture under 1 MiB.
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'lfd-a-light-and-fast-detector_amd'))
warnings.filterwarnings('ignore')

from oracle import ref_import  # noqa: E402
from lfd_amd import configs  # noqa: E402  (only the arch dicts + perturbation helper)

SHAPE = (2, 128, 192)
X_SEED = 23
TAP_VALUES = 16384


def state_sha(sd):
    import hashlib
    h = hashlib.sha256()
    for k in sd:
        h.update(k.encode())
        h.update(sd[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def input_codes():
    n, h, w = SHAPE
    return torch.randint(0, 256, (n, 3, h, w), generator=torch.Generator().manual_seed(X_SEED), dtype=torch.uint8)


def decode_input(codes):
    return codes.float() / 128 - 1


def tap_step(shape):
    for s in (1, 2, 4, 8):
        if shape[0] * shape[1] * -(-shape[2] // s) * -(-shape[3] // s) <= TAP_VALUES:
            return s
    raise ValueError(shape)


def generate(name):
    M = ref_import.import_reference()
    import lfd.model.backbone as RB
    import lfd.model.head as RH
    import lfd.model.losses as RL
    import lfd.model.neck as RN
    arch = configs.PRESETS[name]
    model = configs.build_modules(arch, RB.LFDResNet, RN.SimpleNeck, RH.LFDHead, M.LFD, RL.FocalLoss, RL.IoULoss,
                                  RL.CrossEntropyLoss, seed=666, qfl_cls=RL.QualityFocalLoss)
    configs.perturb_weights(model, seed=1)
    sha = state_sha(model.state_dict())
    model.eval()
    codes = input_codes()
    x = decode_input(codes)
    with torch.no_grad():
        taps = model._backbone(x)
        cls, reg = model(x)
    out = dict(sha=sha, x_codes=codes.numpy(), cls=cls.numpy(), reg=reg.numpy(),
               sizes=np.array([model.head_indexes_to_feature_map_sizes[i] for i in range(len(taps))]),
               tap_shapes=np.array([t.shape for t in taps]), tap_steps=np.array([tap_step(t.shape) for t in taps]))
    for i, t in enumerate(taps):
        s = tap_step(t.shape)
        out['tap%d' % i] = t[:, :, ::s, ::s].contiguous().numpy()
    return out


def main():
    check = '--check' in sys.argv
    bad = 0
    for name in configs.PRESETS:
        out = generate(name)
        path = os.path.join(HERE, 'presets_%s.npz' % name)
        if check:
            old = np.load(path)
            same = sorted(old.files) == sorted(out) and all(np.array_equal(old[k], out[k]) for k in out)
            print(name, 'identical' if same else 'DIFFERS')
            bad += not same
        else:
            np.savez_compressed(path, **out)
            print(name, tuple(out['cls'].shape), tuple(out['reg'].shape), [tuple(s) for s in out['tap_shapes']],
                  '%d KiB' % (os.path.getsize(path) // 1024))
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
