"""tests/golden/make_golden_sibling_targets.py -- ref_sibling_targets.npz: the training targets the REAL reference classes
(FCOS, FCOSv1, LFDv2; imported through oracle/ref_import.py in the build container) assign to the edge-case batch of
sibling_target_cases.py.  Data only (labels and distances); inputs are rebuilt from the case module.

    python tests/golden/make_golden_sibling_targets.py

Keys: fcos_labels [3,P], fcos_reg [3,P,4]; fcosv1_labels [2,P,C], fcosv1_reg [2,P,4] for images 1 and 2 only (the
reference's FCOSv1 returns a [P] vector for an image without boxes, fcos.py:570-572, which its own torch.stack refuses next
to [P,C] rows); v2_<i>_cls [3,P,C], v2_<i>_reg [3,P,4] for the i-th entry of V2_CASES.

torch.sqrt on fp32 CPU tensors is a <= 1 ulp vector routine whose last bit depends on the host's CPU; while the reference
runs here it is evaluated correctly rounded (through fp64, exact for fp32 inputs), like the `ieee_sqrt` fixture of
tests/conftest.py, so the stored scores are the IEEE values on every host -- what the kernels compute.
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
sys.path.insert(0, HERE)
warnings.filterwarnings('ignore')

from oracle import ref_import  # noqa: E402
import sibling_target_cases as TC  # noqa: E402


def targets_of(model, ann):
    for i, hw in enumerate(TC.SIZES):
        model._head_indexes_to_feature_map_sizes[i] = hw
    pts = model.generate_point_coordinates(model._head_indexes_to_feature_map_sizes)
    a, b = model.annotation_to_target(pts, [torch.from_numpy(x) for x, _ in ann], [torch.from_numpy(l) for _, l in ann])
    return a.numpy(), b.numpy()


def main():
    real_sqrt = torch.sqrt
    torch.sqrt = lambda x, *a, **k: real_sqrt(x.double()).float() if (not a and not k and x.dtype == torch.float32) \
        else real_sqrt(x, *a, **k)
    M = ref_import.import_reference()
    import lfd.model.losses as RL
    ann = TC.annotations()
    out = {}
    m = M.FCOS(num_classes=TC.NUM_CLASSES, regress_ranges=TC.FCOS_RANGES, point_strides=TC.STRIDES)
    out['fcos_labels'], out['fcos_reg'] = targets_of(m, ann)
    m = M.FCOSv1(num_classes=TC.NUM_CLASSES, regress_ranges=TC.FCOS_RANGES, point_strides=TC.STRIDES)
    out['fcosv1_labels'], out['fcosv1_reg'] = targets_of(m, ann[1:])
    for i, (mode, loss) in enumerate(TC.V2_CASES):
        m = M.LFDv2(num_classes=TC.NUM_CLASSES, regression_ranges=TC.V2_RANGES, gray_range_factors=TC.GRAY_FACTORS,
                    range_assign_mode=mode, point_strides=TC.STRIDES, classification_loss_func=RL.FocalLoss(),
                    regression_loss_func=getattr(RL, loss)(), distance_to_bbox_mode='exp')
        out['v2_%d_cls' % i], out['v2_%d_reg' % i] = targets_of(m, ann)
    np.savez_compressed(os.path.join(HERE, 'ref_sibling_targets.npz'), **out)
    for k, v in out.items():
        print(k, v.shape, v.dtype, 'nonzero', int((v != 0).sum()))
    fl = out['fcos_labels']
    print('fcos positives per image', [(int((fl[i] != TC.NUM_CLASSES).sum())) for i in range(3)])
    print('bytes', os.path.getsize(os.path.join(HERE, 'ref_sibling_targets.npz')))


if __name__ == '__main__':
    main()
