"""INT8 calibration rules on the host (lfd_amd/calibration.py): every rule against the plain-loop float64 restatement
of tests/golden/calib_cases.py on seeded histograms (thresholds equal, not close), hand-derived cases, invariants, non-finite bins,
the version-2 cache codec, the calibrator's constructor, and the argument checks of lfd_abs_histogram_f16 (host-only calls)."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

import calib_cases as CC
from conftest import ROOT
from lfd_amd import INT8Calibrator, _lib, calibration, deployment

# the restatement's loops stay fast with coarser linear bins; the module takes them through the same parameters
SMALL = {'entropy': dict(nbins=256, nlevels=16, start_bin=16, stride=1), 'mse': dict(nbins=256, start_bin=16, stride=8)}


@pytest.fixture(scope='module')
def hists():
    return CC.seeded_histograms()


def _one_bin(value, count=1):
    h = np.zeros(CC.BINS, dtype=np.int64)
    h[int(np.float16(value).view(np.uint16))] = count
    return h


KINDS = ['half_normal', 'post_relu', 'spike', 'two_clusters']


def test_the_seeded_histograms_are_what_they_are_called(hists):
    assert sorted(hists) == sorted(KINDS)
    assert 0.45 < hists['post_relu'][0] / hists['post_relu'].sum() < 0.55
    assert calibration.amax_of(hists['spike']) == 240.0
    assert hists['two_clusters'][int(np.float16(10.0).view(np.uint16)):int(np.float16(40.0).view(np.uint16))].sum() == 0


def test_bin_values_are_the_fp16_values():
    v = calibration.bin_values()
    for b in (0, 1, 0x03ff, 0x0400, 0x3c00, 0x3c01, 0x7bff):
        assert v[b] == CC.val(b)
    assert v[0x7bff] == 65504.0 and np.isinf(v[0x7c00]) and np.isnan(v[0x7c01])
    assert bool((np.diff(v[:0x7c01]) > 0).all())


@pytest.mark.parametrize('kind', KINDS)
def test_amax_and_percentile_equal_the_restatement(hists, kind):
    h = hists[kind]
    assert calibration.threshold(h, 'amax')[0] == CC.amax_ref(h) == calibration.amax_of(h)
    for p in (50.0, 90.0, 99.0, 99.9, 99.99, 100.0):
        t, clipped = calibration.threshold(h, 'percentile', percentile=p)
        assert t == CC.percentile_ref(h, p), (kind, p)
        assert clipped == CC.clipped_ref(h, t)


@pytest.mark.parametrize('kind', KINDS)
def test_entropy_equals_the_restatement(hists, kind):
    h = hists[kind]
    for params in (SMALL['entropy'], dict(nbins=200, nlevels=12, start_bin=12, stride=3)):
        t, clipped = calibration.threshold(h, 'entropy', **params)
        assert t == CC.entropy_ref(h, **params), (kind, params)
        assert 0.0 < t <= CC.amax_ref(h) and clipped == CC.clipped_ref(h, t)


@pytest.mark.parametrize('kind', KINDS)
def test_mse_equals_the_restatement(hists, kind):
    h = hists[kind]
    for params in (SMALL['mse'], dict(nbins=100, start_bin=7, stride=5)):
        t, clipped = calibration.threshold(h, 'mse', **params)
        assert t == CC.mse_ref(h, **params), (kind, params)
        assert 0.0 < t <= CC.amax_ref(h) and clipped == CC.clipped_ref(h, t)


def test_clipping_on_the_spike_and_the_invariants_with_default_parameters(hists):
    # one element at 240 over 40000 of a half-normal of scale 0.5: the percentile rule leaves it out.  ('entropy' as defined
    # cannot: every candidate below the spike has an empty last bin under the outlier mass, KL = +inf, so T = A.)
    t, clipped = calibration.threshold(hists['spike'], 'percentile', percentile=99.9)
    assert t < 2.4 and clipped > 0
    assert calibration.threshold(hists['spike'], 'entropy') == (240.0, 0.0)
    # default parameters run on a full histogram and stay inside [0, A]
    for kind in KINDS:
        for alg in calibration.ALGORITHMS:
            t, clipped = calibration.threshold(hists[kind], alg)
            assert 0.0 <= t <= calibration.amax_of(hists[kind]) and 0.0 <= clipped < 1.0
            assert clipped == calibration.clipped_share(hists[kind], t)


def test_hand_derived_cases():
    # all mass in one bin: T is that value for every rule, nothing clipped
    for value in (0.37109375, 1.0, 1000.0, 65504.0, 5.960464477539063e-08):
        h = _one_bin(value, 1000)
        for alg in calibration.ALGORITHMS:
            assert calibration.threshold(h, alg) == (float(np.float16(value)), 0.0), (alg, value)
        assert calibration.threshold(h, 'entropy', **SMALL['entropy']) == (float(np.float16(value)), 0.0)
    # ... zeros beside it change nothing
    h = _one_bin(3.0, 10)
    h[0] = 10 ** 6
    for alg in calibration.ALGORITHMS:
        assert calibration.threshold(h, alg, **({'percentile': 100.0} if alg == 'percentile' else {})) == (3.0, 0.0)
    # 99 ones and 1 hundred
    h = _one_bin(1.0, 99) + _one_bin(100.0, 1)
    assert calibration.threshold(h, 'percentile', percentile=99)[0] == 1.0
    assert calibration.threshold(h, 'percentile', percentile=99) == (1.0, 0.01)
    assert calibration.threshold(h, 'percentile', percentile=99.5) == (100.0, 0.0)
    assert calibration.threshold(h, 'percentile', percentile=100) == (100.0, 0.0)
    assert calibration.threshold(h, 'amax') == (100.0, 0.0)
    # zeros count towards the percentile: 90 zeros, 10 at 2.0
    h = _one_bin(2.0, 10)
    h[0] = 90
    assert calibration.threshold(h, 'percentile', percentile=90) == (0.0, 0.1)
    assert calibration.threshold(h, 'percentile', percentile=90.5) == (2.0, 0.0)
    # mse by hand: 1000 at 1.0 and 1 at 127.0, candidates T = 127 i / 2048.  At T = 127 (s = 1) both are exact, err = 0; every
    # smaller T clips the one at 127 and pays (127 - T)^2 > 0
    h = _one_bin(1.0, 1000) + _one_bin(127.0, 1)
    assert calibration.threshold(h, 'mse') == (127.0, 0.0)
    # an empty histogram and an all-zero tensor: T = 0 for every rule (act_scale maps it to scale 1)
    for h in (np.zeros(CC.BINS, dtype=np.int64), _one_bin(0.0, 5)):
        for alg in calibration.ALGORITHMS:
            assert calibration.threshold(h, alg) == (0.0, 0.0)


def test_thresholds_reports_every_tensor(hists):
    r = calibration.thresholds(hists, 'percentile', percentile=99.0)
    assert sorted(r) == ['amax', 'clipped', 'threshold']
    for k in KINDS:
        assert r['amax'][k] == CC.amax_ref(hists[k]) and r['threshold'][k] == CC.percentile_ref(hists[k], 99.0)
        assert r['clipped'][k] == CC.clipped_ref(hists[k], r['threshold'][k]) and r['clipped'][k] <= 0.01


@pytest.mark.parametrize('pattern', [0x7c00, 0x7c01, 0x7fff])
def test_a_non_finite_bin_raises_and_names_the_tensor(hists, pattern):
    h = hists['half_normal'].copy()
    h[pattern] = 2
    for alg in calibration.ALGORITHMS:
        with pytest.raises(ValueError, match='stage1.block0.conv2'):
            calibration.threshold(h, alg, 'stage1.block0.conv2')
    with pytest.raises(ValueError, match="'bad'"):
        calibration.thresholds({'good': hists['spike'], 'bad': h}, 'mse')


def test_malformed_histograms_and_parameters_raise(hists):
    with pytest.raises(ValueError):
        calibration.threshold(np.zeros(100, dtype=np.int64), 'amax')
    with pytest.raises(ValueError):
        calibration.threshold(np.zeros(CC.BINS, dtype=np.float64), 'amax')
    for alg, params in (('minmax', {}), ('amax', dict(percentile=99.0)), ('percentile', dict(percentile=0.0)),
                        ('percentile', dict(percentile=100.5)), ('percentile', dict(percentile='99')), ('entropy', dict(nlevels=0)),
                        ('entropy', dict(nlevels=256, start_bin=128)), ('entropy', dict(start_bin=4096)), ('entropy', dict(stride=0)),
                        ('entropy', dict(nbins=1.5)), ('mse', dict(nlevels=128)), ('mse', dict(start_bin=0)), ('mse', dict(nbins=1))):
        with pytest.raises(ValueError):
            calibration.check_params(alg, params)
        with pytest.raises(ValueError):
            calibration.threshold(hists['spike'], alg, **params)
    assert calibration.check_params('entropy') == dict(nbins=2048, nlevels=128, start_bin=128, stride=1)
    assert calibration.check_params('mse', dict(stride=4)) == dict(nbins=2048, start_bin=128, stride=4)
    assert calibration.check_params('percentile', dict(percentile=99)) == dict(percentile=99.0)


# ---- the cache
NAMES = ['stem', 'stage0.block0.conv1', 'stage0.block0.conv2']


def _values(seed):
    rng = np.random.RandomState(seed)
    return dict((k, float(np.float64(rng.rand()) * 37.0 / 3.0)) for k in NAMES)


def test_the_default_rule_writes_the_version_1_bytes():
    amax = _values(0)
    blob = deployment.encode_cache('ab' * 32, amax)
    d = json.loads(blob.decode())
    assert sorted(d) == ['amax', 'format', 'state_sha256', 'version'] and d['version'] == 1
    assert blob == json.dumps(dict(format='lfd_amd.int8_calibration', version=1, state_sha256='ab' * 32, amax=amax), indent=1).encode()
    cal = INT8Calibrator(np.zeros((1, 3, 8, 8), np.float32), 'unused.json', 1)
    assert (cal.algorithm, cal.params) == ('amax', {})


def test_version_2_round_trips_its_floats_bit_for_bit():
    amax, thr = _values(1), _values(2)
    params = calibration.check_params('percentile', dict(percentile=99.99))
    blob = deployment.encode_cache_v2('cd' * 32, 'percentile', params, amax, thr)
    d = json.loads(blob.decode())
    assert sorted(d) == ['algorithm', 'amax', 'format', 'params', 'state_sha256', 'threshold', 'version']
    assert (d['format'], d['version'], d['algorithm']) == (deployment.CACHE_FORMAT, 2, 'percentile')
    got = deployment.decode_cache_v2(blob, 'cd' * 32, NAMES, 'percentile', params)
    assert got is not None
    for want, have in zip((amax, thr), got):
        assert list(have) == NAMES
        for k in NAMES:
            assert np.float64(have[k]).tobytes() == np.float64(want[k]).tobytes()
    # awkward floats
    odd = dict(zip(NAMES, (0.1 + 0.2, 5.960464477539063e-08, 65504.0)))
    got = deployment.decode_cache_v2(deployment.encode_cache_v2('s', 'mse', calibration.check_params('mse'), odd, odd), 's', NAMES,
                                     'mse', calibration.check_params('mse'))
    assert got == (odd, odd)


def test_every_mismatch_is_rejected():
    amax, thr = _values(1), _values(2)
    params = calibration.check_params('entropy')
    blob = deployment.encode_cache_v2('cd' * 32, 'entropy', params, amax, thr)
    ok = lambda **kw: deployment.decode_cache_v2(kw.get('blob', blob), kw.get('sha', 'cd' * 32), kw.get('names', NAMES),
                                                 kw.get('algorithm', 'entropy'), kw.get('params', params))
    assert ok() is not None
    assert ok(sha='ce' * 32) is None
    assert ok(names=NAMES[:-1]) is None and ok(names=NAMES + ['stage0.block1.conv1']) is None
    assert ok(algorithm='mse') is None and ok(algorithm='mse', params=calibration.check_params('mse')) is None
    assert ok(params=calibration.check_params('entropy', dict(stride=2))) is None
    assert ok(params=calibration.check_params('entropy', dict(nlevels=64))) is None
    for version in (1, 3, '2', None):
        d = json.loads(blob.decode())
        d['version'] = version
        assert ok(blob=json.dumps(d).encode()) is None
    d = json.loads(blob.decode())
    del d['threshold']
    assert ok(blob=json.dumps(d).encode()) is None
    assert ok(blob=b'not json') is None and ok(blob=b'[]') is None
    # the two versions never satisfy each other's decoder
    assert deployment.decode_cache(blob, 'cd' * 32, NAMES) is None
    v1 = deployment.encode_cache('cd' * 32, amax)
    assert deployment.decode_cache(v1, 'cd' * 32, NAMES) == amax
    for alg in ('percentile', 'entropy', 'mse'):
        assert deployment.decode_cache_v2(v1, 'cd' * 32, NAMES, alg, calibration.check_params(alg)) is None


# ---- the calibrator's constructor
def test_constructor_keeps_the_reference_arguments_and_checks_the_new_ones(tmp_path):
    data = np.zeros((5, 3, 8, 8), np.float32)
    cal = INT8Calibrator(data, str(tmp_path / 'c.json'), 2)                          # the reference's three, by position
    assert cal.get_batch_size() == 2 and (cal.algorithm, cal.params) == ('amax', {})
    cal = INT8Calibrator(data, str(tmp_path / 'c.json'), 2, None, 'percentile')
    assert cal.params == dict(percentile=99.99)
    cal = INT8Calibrator(data, str(tmp_path / 'c.json'), batch_size=1, algorithm='entropy', nlevels=64, stride=2)
    assert cal.params == dict(nbins=2048, nlevels=64, start_bin=128, stride=2)
    cal = INT8Calibrator(data, str(tmp_path / 'c.json'), algorithm='mse')
    assert cal.params == dict(nbins=2048, start_bin=128, stride=8) and cal.get_batch_size() == 8
    for kw in (dict(algorithm='kl'), dict(algorithm='percentile', percentile=0), dict(algorithm='percentile', percentile=101),
               dict(algorithm='amax', percentile=99.0), dict(algorithm='mse', nlevels=3), dict(algorithm='entropy', nlevels=4096),
               dict(percentile=99.0)):
        with pytest.raises(ValueError):
            INT8Calibrator(data, str(tmp_path / 'c.json'), 2, **kw)
    import lfd_amd
    assert lfd_amd.calibration is calibration and lfd_amd.INT8Calibrator is deployment.INT8Calibrator


# ---- the kernel's entry point: argument checks happen on the host, before anything touches a device
def test_histogram_entry_point_argument_checks_are_status_codes():
    l = _lib.lib()
    buf = (C.c_char * 256)()
    base = (C.addressof(buf) + 15) & ~15
    al, mis = C.c_void_p(base), C.c_void_p(base + 2)
    hist, hist_mis = C.c_void_p(base + 64), C.c_void_p(base + 68)
    f = l.lfd_abs_histogram_f16
    assert f(al, 0, 64, 48, hist, None) == 0                    # rows == 0: a no-op
    assert f(None, 0, 64, 64, hist, None) == 0
    assert bytes(buf) == b'\0' * 256
    assert f(al, 1, 64, 64, None, None) == -1                   # no histogram
    assert f(None, 1, 64, 64, hist, None) == -1                 # no map
    assert f(al, -1, 64, 64, hist, None) == -1                  # rows < 0
    assert f(al, 1, 60, 60, hist, None) == -1                   # c % 8
    assert f(al, 1, 0, 0, hist, None) == -1
    assert f(al, 1, 64, 0, hist, None) == -1                    # c_real < 1
    assert f(al, 1, 64, 65, hist, None) == -1                   # c_real > c
    assert f(mis, 1, 64, 64, hist, None) == -1                  # x not 16-byte aligned
    assert f(al, 1, 64, 64, hist_mis, None) == -1               # hist not 8-byte aligned
    assert f(al, (1 << 39) // 64 + 1, 64, 64, hist, None) == -4     # a workgroup's 32-bit bins could wrap: unsupported
    assert bytes(buf) == b'\0' * 256


def test_the_restated_geometry_is_the_headers():
    src = open(os.path.join(ROOT, 'include', 'lfd_hip.h')).read()
    assert int(re.search(r'#define LFD_CALIB_HIST_MAX_WORKGROUPS (\d+)', src).group(1)) == CC.MAX_WORKGROUPS
    assert int(re.search(r'#define LFD_CALIB_HIST_CHUNK_VECS (\d+)', src).group(1)) == CC.CHUNK_VECS
    for c in (8, 24):
        rows = CC.multi_chunk_rows(c)
        nvec = rows * c // 8
        assert nvec // CC.CHUNK_VECS >= 2 * CC.MAX_WORKGROUPS and nvec % CC.CHUNK_VECS and rows * c < 2 ** 25
