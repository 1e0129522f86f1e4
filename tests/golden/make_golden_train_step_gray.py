"""tests/golden/make_golden_train_step_gray.py -- three TRAINING ITERATIONS of the real reference with input_channels=1,
frozen as fixtures.

    python tests/golden/make_golden_train_step_gray.py [case ...]

The protocol of make_golden_train_step.py (the reference's Executor.train loop body with its own OptimizerHook and the SGD its
configs build, on CPU), run by that script's own main() on the grayscale twins: the reference LFDResNet built with
input_channels=1 (lfd_resnet.py:354-439) and the one-plane images of train_step_gray_cases.py.  Output (committed):
ref_train_step_gray_<ARCH>.npz, the same keys as ref_train_step_<ARCH>.npz.  Consumers: tests/test_gray_train_host.py,
tests/test_gpu_gray_train.py.
"""
import functools
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_train_step as base  # noqa: E402  (sets up the import paths; its main() is the protocol)
import train_step_gray_cases as gray_cases  # noqa: E402


def main():
    base.cases = gray_cases                                  # the case table, images and file names of the gray fixtures
    base.configs.build_modules = functools.partial(base.configs.build_modules, input_channels=gray_cases.INPUT_CHANNELS)
    base.main()


if __name__ == '__main__':
    main()
