"""INT8 deployment: the third precision the reference publishes next to FP32 and FP16 (lfd/deployment/tensorrt/build_engine.py:
INT8Calibrator + build_tensorrt_engine(..., precision_mode='int8', int8_calibrator=...)).

    calibrator = INT8Calibrator(frames, 'model.int8.json', batch_size=8)     # frames: float32 [N,C,H,W], already normalised
    eng = build_int8_engine(model, calibrator)                               # calibrates, or reads the cache
    cls, reg = eng(x)                                                         # as LFD.forward

The calibrator mirrors the reference's constructor and method names; what is calibrated, and how, is this project's own contract
(lfd_amd/engine_i8.py) -- TensorRT's entropy calibration is proprietary and is not reproduced.  The cache is UTF-8
JSON: {"format", "version", "state_sha256", "amax": {tensor name: largest |value| over the calibration batches}}; a cache
written for other weights (another sha) or another layer list is ignored and calibration runs again.

Calibration rules (lfd_amd/calibration.py): INT8Calibrator(..., algorithm='amax' | 'percentile' | 'entropy' | 'mse',
**the rule's parameters).  'amax' (the default) is the path above, unchanged.  The other rules clip: one pass over the batches
collects a magnitude histogram of every tensor on the device (csrc/calib_hist.hip), the thresholds are chosen from it on the host,
and the cache is version 2: {"format", "version", "state_sha256", "algorithm", "params", "amax", "threshold"}, used only when sha,
tensor names, algorithm and params all match.  A version-1 cache never satisfies a clipping calibrator, and the reverse."""
import hashlib
import json
import os

import numpy
import torch

from . import calibration, engine, engine_i8

CACHE_FORMAT = 'lfd_amd.int8_calibration'
CACHE_VERSION = 1
CACHE_VERSION_RULES = 2      # caches of the clipping rules ('percentile', 'entropy', 'mse')


def state_sha256(state_dict):
    """sha256 over the names and the bytes of a state_dict, in its order"""
    h = hashlib.sha256()
    for k in state_dict:
        h.update(k.encode())
        h.update(state_dict[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def encode_cache(sha, amax):
    return json.dumps(dict(format=CACHE_FORMAT, version=CACHE_VERSION, state_sha256=sha,
                           amax=dict((k, float(v)) for k, v in amax.items())), indent=1).encode('utf-8')


def decode_cache(blob, sha, names):
    """cache bytes -> {name: amax}, or None when the bytes are not a cache of this format for these weights and tensors"""
    try:
        d = json.loads(blob.decode('utf-8'))
    except (ValueError, AttributeError):
        return None
    if not isinstance(d, dict) or d.get('format') != CACHE_FORMAT or d.get('version') != CACHE_VERSION:
        return None
    amax = d.get('amax')
    if d.get('state_sha256') != sha or not isinstance(amax, dict) or sorted(amax) != sorted(names):
        return None
    try:
        return dict((k, float(amax[k])) for k in names)
    except (TypeError, ValueError):
        return None


def encode_cache_v2(sha, algorithm, params, amax, threshold):
    """version-2 cache bytes of a clipping rule: the rule, its full parameter dict, and per tensor the amax seen and the
    threshold chosen (floats as their shortest round-tripping decimal: decoding gives the same bits)"""
    return json.dumps(dict(format=CACHE_FORMAT, version=CACHE_VERSION_RULES, state_sha256=sha, algorithm=algorithm,
                           params=dict(params), amax=dict((k, float(v)) for k, v in amax.items()),
                           threshold=dict((k, float(v)) for k, v in threshold.items())), indent=1).encode('utf-8')


def decode_cache_v2(blob, sha, names, algorithm, params):
    """cache bytes -> ({name: amax}, {name: threshold}), or None when the bytes are not a version-2 cache for these weights,
    these tensors, this rule and these parameters"""
    try:
        d = json.loads(blob.decode('utf-8'))
    except (ValueError, AttributeError):
        return None
    if not isinstance(d, dict) or d.get('format') != CACHE_FORMAT or d.get('version') != CACHE_VERSION_RULES:
        return None
    if d.get('state_sha256') != sha or d.get('algorithm') != algorithm or d.get('params') != dict(params):
        return None
    amax, thr = d.get('amax'), d.get('threshold')
    if not isinstance(amax, dict) or not isinstance(thr, dict) or sorted(amax) != sorted(names) or sorted(thr) != sorted(names):
        return None
    try:
        return dict((k, float(amax[k])) for k in names), dict((k, float(thr[k])) for k in names)
    except (TypeError, ValueError):
        return None


class INT8Calibrator(object):
    """Calibration frames in batches, and the cache file.  data: float32 [N,C,H,W], each image already normalised (numpy array
    or torch tensor); frames beyond the last whole batch are not used, as in the reference.  algorithm and its parameters
    (lfd_amd/calibration.py: 'amax'; 'percentile': percentile; 'entropy': nbins, nlevels, start_bin, stride; 'mse': nbins,
    start_bin, stride) come after the reference's arguments; an unknown rule or a value out of range is a ValueError here."""

    def __init__(self, data, cache_file, batch_size=8, device=None, algorithm='amax', **params):
        self.algorithm = algorithm
        self.params = calibration.check_params(algorithm, params)
        self._cache_file = cache_file
        self._batch_size = int(batch_size)
        if isinstance(data, torch.Tensor):
            data = data.detach().cpu().numpy()
        assert data.ndim == 4 and data.dtype == numpy.float32
        assert self._batch_size >= 1
        self._data = numpy.array(data, dtype=numpy.float32, order='C')
        self._current_index = 0
        self._device = device

    def get_batch_size(self):
        return self._batch_size

    def get_batch(self, names=None, p_str=None):
        """the next batch as a device tensor [batch_size,C,H,W]; None when fewer than batch_size frames remain"""
        if self._current_index + self._batch_size > self._data.shape[0]:
            return None
        batch = self._data[self._current_index:self._current_index + self._batch_size]
        self._current_index += self._batch_size
        return torch.from_numpy(batch).to(self._device if self._device is not None else 'cuda')

    def reset(self):
        self._current_index = 0

    def read_calibration_cache(self):
        if os.path.exists(self._cache_file):
            with open(self._cache_file, 'rb') as f:
                return f.read()
        return None

    def write_calibration_cache(self, cache):
        with open(self._cache_file, 'wb') as f:
            f.write(cache)


class Int8Engine(object):
    """An LFD model's eval forward with int8 residual stages.  scales: {tensor name: (threshold, scale)}, the threshold being
    the amax under the default rule; calibrated: whether this build ran the calibration batches (False: the cache was used);
    calibration: {'algorithm', 'params', 'amax': {name: value}, 'threshold': {name: value}, 'clipped': {name: share of the
    calibration elements above the threshold}} ('clipped' is None where the thresholds came from a cache, which does not
    keep it)."""

    def __init__(self, model, plan, calibrated, calibration=None):
        self.model = model
        self.plan = plan
        self.calibrated = calibrated
        self.calibration = calibration
        self.use_graph = False

    @property
    def scales(self):
        return self.plan.scales

    @property
    def fused(self):
        """whether the stages run the fused launches of csrc/block_i8.hip and csrc/conv_i8.hip (build_int8_engine(..., fused=True)); the bits of every
        output are the same either way"""
        return self.plan.fused

    @property
    def route(self):
        """'layers' | 'fused' | 'full': how the stages are launched (build_int8_engine's fused = False | True | 'full')"""
        return self.plan.route

    @property
    def block128(self):
        """whether the 128-channel residual blocks run as one launch each (csrc/block128_i8.hip; build_int8_engine(...,
        block128=True)); the bits of every output are the same either way"""
        return self.plan.block128

    @property
    def stem_int8(self):
        """whether the stem launch writes the int8 map itself where it can (build_int8_engine(..., stem_int8=True)); per call
        it does for the frame formats in plan.stem_int8_formats, and the bits of every output are the same either way"""
        return self.plan.stem_int8

    def _check_fresh(self):
        m = self.model
        if engine._param_signature(m._backbone, m._neck, m._head) != self.plan.param_sig:
            raise RuntimeError('Int8Engine: the model\'s parameters or buffers changed after the engine was built (optimizer step, '
                               'load_state_dict, .to()): the quantised weights and the calibration no longer belong to them -- '
                               'rebuild with build_int8_engine')
        if m.training:
            raise RuntimeError('Int8Engine: the model is in training mode; the engine folds eval-mode BatchNorm (call model.eval())')

    def forward_resident(self, x, slot=0):
        """(cls [N,P,C'], reg [N,P,4]) fp32, level-concatenated, in engine-owned buffers (valid until the next forward of the same
        input shape and slot).  x: the frame formats of LFD.forward."""
        self._check_fresh()
        from . import _lib
        _lib.require_cuda(x, 'Int8Engine.forward')
        if not x.is_contiguous():
            x = x.contiguous()
        plan = self.plan
        fmt, n, h, w = engine._input_format(x, plan.input_channels)
        st = plan.state_for(n, h, w, slot)
        with torch.cuda.device(x.device):
            if self.use_graph:
                engine._run_graphed(plan, st, x, fmt)
            else:
                plan.run_all(x, fmt, st)
        for i, hw in enumerate(st.sizes):
            self.model._head_indexes_to_feature_map_sizes[i] = hw
        return st.cls, st.reg

    def forward(self, x):
        cls, reg = self.forward_resident(x)
        return cls.clone(), reg.clone()

    __call__ = forward

    def detect(self, x, meta, score_thr=None, iou_thr=None, class_agnostic=None, max_candidates=None, slot=0):
        """forward + the model's fused device post-processing (LFD.detect); meta [N,3] on the device"""
        return self.model.detect(self.forward_resident(x, slot), meta, score_thr, iou_thr, class_agnostic, max_candidates)

    def get_results(self, predict_outputs, *args):
        return self.model.get_results(predict_outputs, *args)


def build_int8_engine(model, int8_calibrator, fused=False, block128=False, stem_int8=False):
    """LFD model (eval mode, on the device) + INT8Calibrator -> Int8Engine.  Uses the calibrator's cache when it was written
    for these weights and this layer list; otherwise runs the calibration batches and writes it.  fused=True: the stages run
    the fused int8 launches (stage-entry pair, whole 64-channel block) where the layer list has them; layers, scales, cache
    and every output bit are those of the default layer-by-layer route, and a cache written by either serves the other.
    fused='full': additionally every 64-channel stage-entry block is one launch (csrc/entry_i8.hip), the first of them reading
    the fp16 stem map so that the quantise launch is gone; the same bits again for a finite stem map.  fused takes the bools
    False and True themselves and 'full'; any other value, 1, 0 and numpy.bool_ included, is a ValueError.
    block128=True (with fused=True or 'full'; a ValueError with fused=False): additionally every 128-channel residual block
    without a downsample is one launch (csrc/block128_i8.hip), pyramid taps included; the same bits and the same cache.
    stem_int8=True (with every value of fused; the bools themselves, anything else is a ValueError): the stem launch writes the
    int8 map the stages read (lfd_stem_conv_i8 for a 'fast' stem, every frame format; lfd_stem_faster_fused_i8 for a 'faster'
    stem, NHWC fp16 / uint8 frames), so the fp16 stem map and the quantise launch -- under 'full' the fp16 read of the first
    entry launch -- are gone; stems of 64 stored channels (48 real ones included) of RGB models only, plan.stem_int8_formats
    lists the frame formats, and a call in any other format runs the launches it runs without the option.  The same bits for
    a finite stem map, the same scales and the same cache."""
    assert int8_calibrator is not None, 'calibrator is not provided!'
    engine_i8.check_model(model)
    if model.training:
        raise RuntimeError('build_int8_engine: call model.eval() first (eval-mode BatchNorm is folded into the weights)')
    device = next(model.parameters()).device
    if device.type != 'cuda':
        raise RuntimeError('build_int8_engine: the model must be on the MI355X (got %s)' % device)
    with torch.no_grad():
        plan = engine_i8.Int8Plan(model._backbone, model._neck, model._head, device, fused=fused, block128=block128,
                                    stem_int8=stem_int8)
    sha = state_sha256(model.state_dict())
    blob = int8_calibrator.read_calibration_cache()
    seen = [0]

    def counted():
        while True:
            b = int8_calibrator.get_batch([])
            if b is None:
                return
            seen[0] += 1
            yield b.to(device)

    def check_seen():
        if seen[0] == 0:
            raise RuntimeError('build_int8_engine: the calibrator has no whole batch (fewer frames than batch_size, or already '
                               'consumed) and no usable cache')

    algorithm = getattr(int8_calibrator, 'algorithm', 'amax')
    if algorithm == 'amax':
        amax = decode_cache(blob, sha, plan.tensor_names) if blob is not None else None
        calibrated = amax is None
        if calibrated:
            amax = plan.calibrate(counted())
            check_seen()
            int8_calibrator.write_calibration_cache(encode_cache(sha, amax))
        plan.set_scales(amax)
        return Int8Engine(model, plan, calibrated, dict(algorithm='amax', params={}, amax=dict(amax), threshold=dict(amax),
                                                        clipped=dict((k, 0.0) for k in amax)))
    # a clipping rule: one histogram pass, thresholds on the host, a version-2 cache
    params = calibration.check_params(algorithm, getattr(int8_calibrator, 'params', None))
    got = decode_cache_v2(blob, sha, plan.tensor_names, algorithm, params) if blob is not None else None
    calibrated = got is None
    if calibrated:
        hists = plan.calibrate_histograms(counted())
        check_seen()
        res = calibration.thresholds(hists, algorithm, **params)
        amax, thr, clipped = res['amax'], res['threshold'], res['clipped']
        int8_calibrator.write_calibration_cache(encode_cache_v2(sha, algorithm, params, amax, thr))
    else:
        (amax, thr), clipped = got, None
    plan.set_scales(thr)
    return Int8Engine(model, plan, calibrated, dict(algorithm=algorithm, params=params, amax=amax, threshold=thr, clipped=clipped))
