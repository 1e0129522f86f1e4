"""tests/golden/train_step_gray_cases.py -- the seeded inputs of the GRAYSCALE training-iteration fixtures (input_channels=1,
the task scripts' `num_input_channels`, TT100K_LFD_L.py:77-78), shared by the generator (make_golden_train_step_gray.py) and
the tests (tests/test_gray_train_host.py, tests/test_gpu_gray_train.py).  Same protocol, shapes, annotations and optimizer as
train_step_cases.py; the images are one plane."""
import torch

import train_step_cases as rgb
from train_step_cases import GRAD_CLIP, ITERATIONS, LR, MOMENTUM, WEIGHT_DECAY, annotations  # noqa: F401  (same protocol)

INPUT_CHANNELS = 1
# the RGB shapes of the configurations whose gray twin trains on the all-HIP path (TL_LFD_L: autograd head, see the GPU test)
CASES = {k: rgb.CASES[k] for k in ('WIDERFACE_LFD_S', 'WIDERFACE_LFD_XS', 'TT100K_LFD_L')}
# every BatchNorm of the network sees >= 512 elements per channel (see train_step_cases.LARGE_CASES); summaries only
LARGE_CASES = {'WIDERFACE_LFD_S@8x512x512': ('WIDERFACE_LFD_S', 8, 512, 512)}


def shape_of(name):
    """-> (arch name, images, height, width) for a key of CASES or LARGE_CASES"""
    if name in CASES:
        return (name,) + tuple(CASES[name])
    return LARGE_CASES[name]


def file_tag(name):
    return 'gray_' + name.replace('@', '_at_')


def images(name):
    _, n, h, w = shape_of(name)
    return torch.rand(n, 1, h, w, generator=torch.Generator().manual_seed(11)) * 2 - 1
