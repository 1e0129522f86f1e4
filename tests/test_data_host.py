"""Host side of the device batch assembly (lfd_amd/data.py, include/lfd_hip.h lfd_batch_assemble_f32): the region samplers
against the reference's own decisions (tests/golden/ref_region_sampler.npz), the normalisation tables, the flip rule, the
source windows against the resize contract (tests/golden/batch_oracle.py), the descriptor layout and the status codes.
No GPU."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import batch_oracle
from conftest import ROOT, load_golden
from lfd_amd import _lib, data


def _fixture_cases():
    z = load_golden('ref_region_sampler.npz')
    i0 = o0 = 0
    for k in range(len(z['kind'])):
        i1, o1 = int(z['in_offsets'][k]), int(z['out_offsets'][k])
        yield k, z, (i0, i1), (o0, o1)
        i0, o0 = i1, o1


def test_region_samplers_reproduce_the_reference_decisions():
    n = idle = neg = 0
    for k, z, (i0, i1), (o0, o1) in _fixture_cases():
        h, w = (int(v) for v in z['shape'][k])
        sample = {}
        if i1 > i0:
            sample['bboxes'] = [list(b) for b in z['in_boxes'][i0:i1]]
            sample['bbox_labels'] = [int(v) for v in z['in_labels'][i0:i1]]
        else:
            neg += 1
        random.seed(1000 + k)
        if z['kind'][k] == 1:
            plan = data.IdleRegionSampler()(sample, (h, w, 3))
            assert (sample['resize_scale'], sample['resized_height'], sample['resized_width']) == tuple(z['meta'][k])
            idle += 1
        else:
            lo, hi = (float(v) for v in z['range'][k])
            plan = data.RandomBBoxCropRegionSampler(int(z['crop_size'][k]), (lo, hi), float(z['prob'][k]))(sample, (h, w, 3))
        assert random.random() == z['post'][k], k        # the same number of draws
        assert plan.scale == z['scale'][k], k
        assert plan.dsize == tuple(z['dsize'][k]), k
        assert plan.crop == tuple(z['crop'][k]), k
        got_b = np.array(sample.get('bboxes', []), dtype=np.float64).reshape(-1, 4)
        assert np.array_equal(got_b, z['out_boxes'][o0:o1]), k
        assert np.array_equal(np.array(sample.get('bbox_labels', []), dtype=np.int64), z['out_labels'][o0:o1]), k
        assert ('bboxes' in sample) == (o1 > o0)
        n += 1
    assert n == 360 and idle == 40 and neg > 20


@pytest.mark.parametrize('preset', ['SIMPLE_NORMALIZE', 'STANDARD_NORMALIZE', 'CAFFE_IMAGENET_NORMALIZE'])
def test_lut_is_albumentations_float32_arithmetic(preset):
    cfg = getattr(data, preset)
    lut = data.DeviceAugmentation(normalize=cfg).lut()
    assert lut.shape == (3, 256) and lut.dtype == np.float32
    mean = np.array(cfg['mean'], dtype=np.float32)
    mean *= cfg['max_pixel_value']
    std = np.array(cfg['std'], dtype=np.float32)
    std *= cfg['max_pixel_value']
    den = np.reciprocal(std, dtype=np.float32)
    img = np.arange(256, dtype=np.uint8).reshape(16, 16, 1).repeat(3, 2).astype(np.float32)
    img -= mean
    img *= den
    for c in range(3):
        assert np.array_equal(lut[c], img[:, :, c].reshape(-1)), c
    gray = data.DeviceAugmentation(normalize=cfg, out_channels=1).lut()
    assert gray.shape == (1, 256) and np.array_equal(gray[0], lut[0])


def test_channel_maps_and_flip_rule():
    aug = data.DeviceAugmentation(flip_prob=0.5, bgr2rgb=True)
    assert aug.channel_map(3) == [2, 1, 0] and aug.channel_map(1) == [0, 0, 0]
    assert data.DeviceAugmentation().channel_map(3) == [0, 1, 2]
    with pytest.raises(ValueError):
        data.DeviceAugmentation(out_channels=1).channel_map(3)
    assert data.DeviceAugmentation.flip_boxes([[10, 5, 20, 7], [0, 0, 480, 480]], 480) == [[450, 5, 20, 7], [0, 0, 480, 480]]
    rng = random.Random(3)
    draws = [aug.draw_flip(rng) for _ in range(2000)]
    assert 800 < sum(draws) < 1200
    assert not any(data.DeviceAugmentation(flip_prob=0.0).draw_flip(rng) for _ in range(100))


def test_flipped_sample_boxes_follow_the_flipped_pixels():
    """a box's columns [x, x + w) of the crop land on [S - x - w, S - x) of the flipped crop"""
    S = 40
    crop = np.zeros((4, S), np.uint8)
    x, w = 7, 5
    crop[:, x:x + w] = 1
    flipped = crop[:, ::-1]
    nx = data.DeviceAugmentation.flip_boxes([[x, 0, w, 4]], S)[0][0]
    assert np.flatnonzero(flipped[0]).tolist() == list(range(nx, nx + w))


def _random_plans(rs, count):
    for _ in range(count):
        h, w = int(rs.randint(1, 90)), int(rs.randint(1, 90))
        s = float(rs.choice([rs.uniform(0.5, 1.5), 1.0, 0.5, 1.5]))
        try:
            p = data.RegionPlan(s, h, w, (0, 0, 1, 1))
        except ValueError:
            continue
        cw, ch = int(rs.randint(1, 70)), int(rs.randint(1, 70))
        cx, cy = int(rs.randint(-cw - 5, p.res_w + 5)), int(rs.randint(-ch - 5, p.res_h + 5))
        yield data.RegionPlan(s, h, w, (cx, cy, cw, ch))


def test_every_source_index_of_the_resize_lies_inside_the_window():
    rs = np.random.RandomState(5)
    n = 0
    for p in _random_plans(rs, 300):
        coef, (x0, y0, ww, wh) = data.plan_tables(p, p.crop[2], p.crop[3])
        cols, rows = batch_oracle.touched(p.src_h, p.src_w, p.scale, p.crop)
        assert all(x0 <= c < x0 + ww for c in cols) and all(y0 <= r < y0 + wh for r in rows), p
        if cols and rows:   # the window is the tightest box around what the resize reads
            assert (x0, x0 + ww - 1, y0, y0 + wh - 1) == (min(cols), max(cols), min(rows), max(rows)), p
        assert 0 <= x0 and x0 + ww <= p.src_w and 0 <= y0 and y0 + wh <= p.src_h
        n += 1
    assert n > 250


def test_tables_agree_with_the_contract():
    rs = np.random.RandomState(6)
    for p in _random_plans(rs, 60):
        W, H = p.crop[2], p.crop[3]
        coef, _ = data.plan_tables(p, W, H)
        cols, rows = batch_oracle.touched(p.src_h, p.src_w, p.scale, p.crop)
        if not cols:     # the crop misses the resized image: every weight is zero
            assert not coef[:, 2:].any()
            continue
        for xc in range(W):
            dx = p.crop[0] + xc
            if 0 <= dx < p.res_w:
                assert tuple(coef[xc]) == batch_oracle.taps(p.src_w, dx, p.scale, True), (p, xc)
            else:
                assert coef[xc, 2] == coef[xc, 3] == 0
        for yc in range(H):
            dy = p.crop[1] + yc
            if 0 <= dy < p.res_h:
                assert tuple(coef[W + yc]) == batch_oracle.taps(p.src_h, dy, p.scale, False), (p, yc)
            else:
                assert coef[W + yc, 2] == coef[W + yc, 3] == 0


def test_host_composition_equals_the_restated_contract():
    rs = np.random.RandomState(8)
    aug = data.DeviceAugmentation(flip_prob=0.5, normalize=data.STANDARD_NORMALIZE, bgr2rgb=True)
    plans = list(_random_plans(rs, 6))
    images = [rs.randint(0, 256, size=(p.src_h, p.src_w, 3)).astype(np.uint8) for p in plans]
    flips = [bool(rs.rand() < 0.5) for _ in plans]
    h, w = max(p.valid_h for p in plans), max(p.valid_w for p in plans)
    got = data.compose_host(images, plans, flips, aug, h, w)
    ref = batch_oracle.compose(images, [p.scale for p in plans], [p.crop for p in plans], flips, aug.lut(), [2, 1, 0], 3, h, w)
    assert np.array_equal(got, ref)


def test_empty_resize_raises():
    with pytest.raises(ValueError):
        data.RegionPlan(0.5, 1, 40, (0, 0, 8, 8))      # rint(0.5) == 0: cv2 asserts
    with pytest.raises(ValueError):
        data.RandomBBoxCropRegionSampler(16, (0.3, 0.3), 1.0)({}, (1, 1, 3))
    assert data.resized_size(3, 5, 0.5) == (2, 2)      # 1.5 -> 2, 2.5 -> 2: half to even


def test_tables_that_leave_the_window_are_refused():
    p = data.RegionPlan(1.0, 10, 10, (0, 0, 4, 4))
    coef, window = data.plan_tables(p, 4, 4)
    coef[1, 1] = 9
    with pytest.raises(RuntimeError):
        data.check_tables(coef, window, 4, p)


def test_batch_desc_mirror_matches_gcc(tmp_path):
    fields = [f for f, _ in _lib.BatchDesc._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lfd_hip.h"', 'int main(void) {',
             'printf("size %zu\\n", sizeof(lfd_batch_desc_t));']
    lines += ['printf("%s %%zu\\n", offsetof(lfd_batch_desc_t, %s));' % (f, f) for f in fields]
    lines += ['return 0; }']
    src = tmp_path / 'desc.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'desc'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True, capture_output=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    assert int(got['size']) == C.sizeof(_lib.BatchDesc) == data.DESC_BYTES
    for f in fields:
        assert int(got[f]) == getattr(_lib.BatchDesc, f).offset, f


_STATUS_SCRIPT = r"""
import ctypes as C
import sys
sys.path.insert(0, sys.argv[1])
import torch
assert torch.cuda.device_count() == 0, 'a device is visible: the status-code calls are not run'
from lfd_amd import _lib
l = _lib.lib()
P = C.c_void_p
a = [P(0x10000), P(0x20000), P(0x30000), P(0x40000), P(0x50000)]
out = P(0x60000)


def call(args=a, n=2, c_src=3, c_out=3, h=8, w=8, o=out):
    return l.lfd_batch_assemble_f32(*args, n, c_src, c_out, h, w, o, None)
for i in range(5):
    bad = list(a)
    bad[i] = P(0)
    assert call(args=bad) == -1, i
assert call(o=P(0)) == -1
for i, off in ((1, 4), (2, 8), (3, 4), (4, 4)):      # desc, map: 8 bytes; coef, lut: 16 bytes
    bad = list(a)
    bad[i] = P(a[i].value + off)
    assert call(args=bad) == -1, i
assert call(o=P(0x60004)) == -1
for c in (0, 2, 4):
    assert call(c_src=c) == -1 and call(c_out=c) == -1
assert call(n=0) == -1 and call(h=0) == -1 and call(w=-3) == -1
assert call(n=1 << 14, c_out=3, h=256, w=256) == -4        # 2^31.6 elements
assert call(n=1, c_out=1, h=1 << 15, w=1 << 16) == -4       # exactly 2^31
print('status codes ok')
"""


def test_invalid_arguments_are_status_codes():
    """The argument checks run on the host and refuse before any launch.  The calls carry fake (aligned, unmapped) addresses,
    so they run in a child process that sees no device: were a check ever loosened, the launch would fail with a status
    (no device), never touch a GPU."""
    env = dict(os.environ, HIP_VISIBLE_DEVICES='-1', CUDA_VISIBLE_DEVICES='-1')
    r = subprocess.run([sys.executable, '-c', _STATUS_SCRIPT, os.path.dirname(os.path.dirname(_lib.__file__))], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and 'status codes ok' in r.stdout, r.stdout + r.stderr
