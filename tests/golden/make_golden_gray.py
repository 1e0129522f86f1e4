"""tests/golden/make_golden_gray.py -- regenerates ref_model_gray_<ARCH>.npz: the REAL reference (imported through
oracle/ref_import.py, as make_golden.py does) built with input_channels=1 -- the grayscale option of its backbone
(`# input image channels: BGR--3, gray--1`, TT100K_LFD_L.py:77-78) -- seeded, perturbed, and run on a one-channel
batch [N,1,H,W] at a small shape.

    python tests/golden/make_golden_gray.py

Weights are NOT stored: torch.manual_seed(666) + lfd_amd.configs.perturb_weights(seed=1) regenerate them; the sha256 of
the reference state_dict is stored so a drift in init order or RNG is detected instead of silently changing the inputs.
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

CASES = (('WIDERFACE_LFD_S', (2, 72, 104)), ('TL_LFD_S', (1, 72, 120)))
X_SEED = 7


def state_sha(sd):
    import hashlib
    h = hashlib.sha256()
    for k in sd:
        h.update(k.encode())
        h.update(sd[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def main():
    M = ref_import.import_reference()
    import lfd.model.backbone as RB
    import lfd.model.head as RH
    import lfd.model.losses as RL
    import lfd.model.neck as RN
    for name, (N, H, W) in CASES:
        arch = configs.ARCHS[name]
        model = configs.build_modules(arch, RB.LFDResNet, RN.SimpleNeck, RH.LFDHead, M.LFD, RL.FocalLoss, RL.IoULoss,
                                      RL.CrossEntropyLoss, seed=666, qfl_cls=RL.QualityFocalLoss, input_channels=1)
        assert model._backbone._input_channels == 1
        sha_init = state_sha(model.state_dict())
        configs.perturb_weights(model, seed=1)
        sha = state_sha(model.state_dict())
        model.eval()
        x = torch.rand(N, 1, H, W, generator=torch.Generator().manual_seed(X_SEED)) * 2 - 1
        with torch.no_grad():
            cls, reg = model(x)
        sizes = [model.head_indexes_to_feature_map_sizes[i] for i in range(len(arch['regression_ranges']))]
        np.savez_compressed(os.path.join(HERE, 'ref_model_gray_%s.npz' % name), x_seed=X_SEED, shape=np.array([N, H, W]),
                            cls=cls.numpy(), reg=reg.numpy(), sizes=np.array(sizes), sha_init=sha_init, sha=sha)
        print(name, 'gray', tuple(cls.shape), tuple(reg.shape))


if __name__ == '__main__':
    main()
