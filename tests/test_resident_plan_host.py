"""The resident loader's draw contract on the host (tests/golden/resident_plan_oracle.py): the Philox known
answers, the oracle's decisions replayed through the existing RandomBBoxCropRegionSampler with a scripted rng (which ties
the new contract to code pinned to the reference by ref_region_sampler.npz), the statistics of the draws, and the ABI of
lfd_plan_bbox_crop_batch (struct layouts, argument checks -- no device call)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import resident_cases as RC
import resident_plan_oracle as oracle
from conftest import ROOT
from lfd_amd import _lib, data

KNOWN = [
    ('00000000 00000000 00000000 00000000', '00000000 00000000', '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ('ffffffff ffffffff ffffffff ffffffff', 'ffffffff ffffffff', '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ('243f6a88 85a308d3 13198a2e 03707344', 'a4093822 299f31d0', 'd16cfe09 94fdcceb 5001e420 24126ea1'),
]


@pytest.mark.parametrize('counter,key,out', KNOWN)
def test_philox4x32_10_known_answers(counter, key, out):
    words = lambda s: [int(v, 16) for v in s.split()]     # noqa: E731
    assert oracle.philox4x32_10(words(counter), words(key)) == words(out)


def test_uniform_and_pick_are_the_documented_constructions():
    assert oracle.uniform(0, 0) == 0.0
    assert oracle.uniform(0xffffffff, 0xffffffff) == 1.0 - 2.0 ** -53
    assert oracle.uniform(1 << 5, 0) == 2.0 ** -27 and oracle.uniform(0, 1 << 6) == 2.0 ** -53
    assert oracle.pick(0, 7) == 0 and oracle.pick(0xffffffff, 7) == 6 and oracle.pick(1 << 31, 7) == 3
    assert oracle.words(5 | (9 << 32), 2, 3, 4)[:4] == oracle.philox4x32_10((4, 3, 2, 0), (5, 9))
    assert oracle.words(5 | (9 << 32), 2, 3, 4)[4:] == oracle.philox4x32_10((4, 3, 2, 1), (5, 9))


class Scripted(object):
    """an rng that returns the oracle's decisions in the reference's conditional draw order: random() for the probability,
    random() for the scale only when resizing, choice() only when there are boxes, randint() twice, random() for the flip"""

    def __init__(self, d):
        self.d = d
        self.randoms = [d.p] + ([d.u_scale] if d.resized else []) + [d.u_flip]
        self.ints = [(d.x_range, d.rand_x), (d.y_range, d.rand_y)]
        self.chose = False

    def random(self):
        return self.randoms.pop(0)

    def choice(self, seq):
        assert self.d.target is not None and not self.chose
        self.chose = True
        return seq[self.d.target]

    def randint(self, a, b):
        (lo, hi), v = self.ints.pop(0)
        assert (a, b) == (lo, hi) and a <= v <= b
        return v

    def exhausted(self):
        return not self.randoms and not self.ints and (self.chose or self.d.target is None)


def test_oracle_decisions_replayed_through_the_region_sampler_give_the_oracle_plan():
    ds = RC.dataset()
    sampler = data.RandomBBoxCropRegionSampler(RC.CROP, RC.RESIZE_RANGE, RC.RESIZE_PROB)
    aug = data.DeviceAugmentation(flip_prob=RC.FLIP_PROB)
    seen = dict(resized=0, flipped=0, negative=0, dropped_all=0, no_boxes=0)
    for e in range(RC.EPOCHS):
        for b, row in enumerate(RC.ROWS):
            for slot, m in enumerate(row):
                s = ds[m]
                shape = s['image'].shape
                ps = oracle.plan_sample(s.get('bboxes', []), s.get('bbox_labels', []), shape, RC.SEED, e, b, slot, RC.CROP,
                                        RC.RESIZE_RANGE, RC.RESIZE_PROB, RC.FLIP_PROB)
                d = ps['decision']
                st = {k: s[k] for k in ('bboxes', 'bbox_labels') if k in s}
                rng = Scripted(d)
                plan = sampler(st, shape, rng)
                flip = aug.draw_flip(rng)
                assert rng.exhausted(), (e, b, slot)
                if flip and 'bboxes' in st:
                    st['bboxes'] = data.DeviceAugmentation.flip_boxes(st['bboxes'], plan.valid_w)
                op = ps['plan']
                assert flip == ps['flip']
                assert (plan.scale, plan.src_h, plan.src_w, plan.res_h, plan.res_w, plan.crop) == \
                    (op.scale, op.src_h, op.src_w, op.res_h, op.res_w, op.crop), (e, b, slot)
                boxes = np.array(st.get('bboxes', []), dtype=np.float32).reshape(-1, 4)
                labels = np.array(st.get('bbox_labels', []), dtype=np.int64).reshape(-1)
                assert np.array_equal(boxes, ps['boxes']) and np.array_equal(labels, ps['labels']), (e, b, slot)
                coef, window = data.plan_tables(plan, RC.CROP, RC.CROP)
                assert np.array_equal(coef, ps['coef']) and tuple(window) == tuple(ps['window']), (e, b, slot)
                seen['resized'] += d.resized
                seen['flipped'] += flip
                seen['negative'] += d.x_range[0] < 0 or d.y_range[0] < 0
                seen['dropped_all'] += len(s.get('bboxes', [])) > 0 and len(boxes) == 0
                seen['no_boxes'] += d.target is None
    # the cases the dataset was built for do occur among the planned samples
    assert all(v > 0 for k, v in seen.items() if k != 'dropped_all'), seen


def test_draw_statistics_and_ranges_over_20000_samples():
    """seed 0, 20 000 draws: deterministic, so it cannot flake"""
    boxes = [[30.0, 40.0, 25.0, 35.0], [100.5, 20.0, 90.0, 12.0], [5.0, 60.0, 10.0, 120.0]]
    n, cs, rp, fp = 20000, 64, 0.3, 0.6
    resized = flipped = 0
    targets = [0, 0, 0]
    for i in range(n):
        d = oracle.decide(boxes, (160, 240), 0, i // 5000, (i // 100) % 50, i % 100, cs, (0.5, 1.5), rp, fp)
        resized += d.resized
        flipped += d.flip
        targets[d.target] += 1
        assert 0.0 <= d.p < 1.0 and 0.0 <= d.u_flip < 1.0
        assert (0.5 <= d.scale < 1.5) if d.resized else d.scale == 1.0
        tgt = oracle.scale_boxes(boxes, d.scale)[d.target]
        for c, size, (lo, hi), v in ((d.crop_x, tgt[2], d.x_range, d.rand_x), (d.crop_y, tgt[3], d.y_range, d.rand_y)):
            assert (lo, hi) == (min(0, cs - size), max(0, cs - size)) and lo <= v <= hi
        assert d.crop_x == tgt[0] - d.rand_x and d.crop_y == tgt[1] - d.rand_y
    for count, p in ((resized, rp), (flipped, fp)) + tuple((t, 1.0 / 3) for t in targets):
        assert abs(count - n * p) <= 5 * math.sqrt(n * p * (1 - p)), (count, p)


def test_an_empty_resize_is_a_blank_sample_not_an_error():
    ps = oracle.plan_sample([[0.0, 0.0, 1.0, 1.0]], [0], (1, 5), 3, 0, 0, 0, 16, (0.01, 0.02), 1.0, 0.5)
    assert ps['plan'] is None and len(ps['boxes']) == 0 and not ps['coef'].any() and ps['window'] == (0, 0, 1, 1)
    out = oracle.plan_batch([{'bboxes': [[0.0, 0.0, 1.0, 1.0]], 'bbox_labels': [0]}], [(1, 5)], [0], 3, [0, 0], 3, 0, 0, 16,
                            (0.01, 0.02), 1.0, 0.5, 4, 8)
    assert out['status'].tolist() == [oracle.EMPTY_RESIZE, 0, 0, 2] and out['offsets'].tolist() == [0, 0, 0]
    assert out['desc']['valid_w'].tolist() == [0, 0]


def test_plan_structs_mirror_the_header_and_arguments_are_checked_on_the_host(tmp_path):
    pairs = {'lfd_plan_desc_t': _lib.PlanDesc, 'lfd_plan_bufs_t': _lib.PlanBufs}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "lfd_hip.h"', 'int main(void) {']
    for cname, mirror in pairs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in mirror._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    lines += ['return 0; }']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.run(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True, capture_output=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines())
    for cname, mirror in pairs.items():
        assert int(got[cname]) == C.sizeof(mirror), cname
        for fname, _ in mirror._fields_:
            assert int(got['%s.%s' % (cname, fname)]) == getattr(mirror, fname).offset, (cname, fname)
    # argument checks happen before anything touches a device
    l = _lib.lib()
    assert l.lfd_plan_bbox_crop_batch(None, None, None) == -1
    buf = (C.c_char * 256)()
    al = (C.addressof(buf) + 15) & ~15
    d, b = _lib.PlanDesc(), _lib.PlanBufs()
    for name, _ in _lib.PlanBufs._fields_:
        setattr(b, name, al)
    d.n, d.num_images, d.crop_size, d.c_src, d.max_boxes_per_image, d.max_boxes = 1, 1, 16, 3, 4, 4
    d.resize_lo, d.resize_hi = 0.5, 1.5

    def status(**kw):
        d2, b2 = _lib.PlanDesc.from_buffer_copy(d), _lib.PlanBufs.from_buffer_copy(b)
        for k, v in kw.items():
            setattr(b2 if hasattr(b2, k) else d2, k, v)
        return l.lfd_plan_bbox_crop_batch(C.byref(d2), C.byref(b2), None)
    assert status(n=0) == -1 and status(crop_size=0) == -1 and status(c_src=2) == -1 and status(max_boxes=0) == -1
    assert status(max_boxes_per_image=0) == -1 and status(resize_hi=float('inf')) == -1 and status(resize_lo=float('nan')) == -1
    assert status(status=None) == -1 and status(indices=None) == -1
    assert status(coef=al + 4) == -1 and status(boxes=al + 8) == -1 and status(desc=al + 4) == -1
    assert status(n=4097) == -4                              # LFD_PLAN_MAX_BATCH
    assert status(n=64, crop_size=4096) == -4                # an assembled output of 2^31 elements or more
    with pytest.raises(TypeError):
        data.ResidentDataLoader(None, None, data.IdleRegionSampler(), None, seed=0)
