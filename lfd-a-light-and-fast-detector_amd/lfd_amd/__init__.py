"""lfd_amd -- MI355X-native (gfx950) implementation of the LFD dense-prediction hot path.

Host-side mirror of the reference's operator interface (`LFDResNet`, `SimpleNeck`, `LFDHead`,
`LFD`, `FocalLoss`, `IoULoss`, `CrossEntropyLoss`, `nms`/`batched_nms`/`multiclass_nms`, and the
`nms_ext` / `sigmoid_focal_loss_ext` extension-module surfaces) over the C-ABI library
`liblfd_hip.so` (include/lfd_hip.h) whose kernels are hand-written HIP for CDNA4.
"""
__version__ = '0.1.0'

_DEPLOYMENT = ('INT8Calibrator', 'Int8Engine', 'build_int8_engine')      # lfd_amd/deployment.py, imported on first use
_CALIBRATION = ('calibration',)                                          # lfd_amd/calibration.py: the INT8 calibration rules


def __getattr__(name):
    if name in _DEPLOYMENT:
        from . import deployment
        return getattr(deployment, name)
    if name in _CALIBRATION:
        import importlib
        return importlib.import_module('.' + name, __name__)
    raise AttributeError('module %r has no attribute %r' % (__name__, name))
