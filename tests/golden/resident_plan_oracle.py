"""The resident loader's draw contract and the whole per-sample plan restated in plain Python / numpy: what
csrc/batch_plan.hip (lfd_plan_bbox_crop_batch) must produce, integer for integer and float32 bit for bit.

Philox4x32-10 and the fixed-position draws are written out here; everything after the draws calls the helpers
lfd_amd/data.py already defines (resized_size, RegionPlan, plan_tables, DeviceAugmentation.flip_boxes).  The box arithmetic
of RandomBBoxCropRegionSampler.__call__ is restated (the sampler makes its own draws); tests/test_resident_plan_host.py replays
the decisions through the sampler itself with a scripted rng and compares.
"""
import math

import numpy as np

from lfd_amd import data

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xffffffff

EMPTY_RESIZE, IMAGE_OVERFLOW, BATCH_OVERFLOW, BAD_SAMPLE = 1, 2, 4, 8


def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words -> 4 words (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11)"""
    c0, c1, c2, c3 = [int(v) & MASK for v in counter]
    k0, k1 = [int(v) & MASK for v in key]
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK, (p0 >> 32) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return [c0, c1, c2, c3]


def uniform(a, b):
    """Python's random() construction: 53 bits"""
    return ((a >> 5) * 67108864.0 + (b >> 6)) * (1.0 / 9007199254740992.0)


def pick(r, n):
    return (r * n) >> 32


def words(seed, epoch, batch, slot):
    key = (seed & MASK, (seed >> 32) & MASK)
    return philox4x32_10((slot, batch, epoch, 0), key) + philox4x32_10((slot, batch, epoch, 1), key)


class Decision(object):
    """what the eight words decide for one sample, before any box arithmetic that does not feed a draw"""
    __slots__ = ('p', 'resized', 'u_scale', 'scale', 'target', 'rand_x', 'rand_y', 'u_flip', 'flip', 'crop_x', 'crop_y',
                 'empty', 'x_range', 'y_range')


def decide(bboxes, shape, seed, epoch, batch, slot, crop_size, resize_range, resize_prob, flip_prob):
    r = words(seed, epoch, batch, slot)
    d = Decision()
    d.p = uniform(r[0], r[1])
    d.resized = d.p < resize_prob
    d.u_scale = uniform(r[2], r[3])
    d.scale = d.u_scale * (resize_range[1] - resize_range[0]) + resize_range[0] if d.resized else 1.0
    d.u_flip = uniform(r[7], r[7])
    d.flip = d.u_flip < flip_prob
    try:
        res_h, res_w = data.resized_size(shape[0], shape[1], d.scale)
        d.empty = False
    except ValueError:
        d.empty = True
        d.target = d.rand_x = d.rand_y = d.crop_x = d.crop_y = d.x_range = d.y_range = None
        return d
    scaled = scale_boxes(bboxes, d.scale)
    if len(scaled) > 0:
        d.target = pick(r[4], len(scaled))
        tgt = scaled[d.target]
    else:
        d.target = None
        tgt = [0, 0, res_w, res_h]
    wr, hr = crop_size - tgt[2], crop_size - tgt[3]
    d.x_range, d.y_range = (min(0, wr), max(0, wr)), (min(0, hr), max(0, hr))
    d.rand_x = min(0, wr) + pick(r[5], abs(wr) + 1)
    d.rand_y = min(0, hr) + pick(r[6], abs(hr) + 1)
    d.crop_x, d.crop_y = tgt[0] - d.rand_x, tgt[1] - d.rand_y
    return d


def scale_boxes(bboxes, scale):
    return [[int(b[0] * scale), int(b[1] * scale), math.ceil(b[2] * scale), math.ceil(b[3] * scale)] for b in bboxes]


def plan_sample(bboxes, labels, shape, seed, epoch, batch, slot, crop_size, resize_range, resize_prob, flip_prob):
    """-> dict(decision, plan (RegionPlan or None), flip, boxes float32 [g, 4], labels int64 [g], coef int32 [2 * cs, 4],
    window).  An empty resize gives plan None: all zero, no boxes, flip False, zero tables, window (0, 0, 1, 1)."""
    cs = crop_size
    d = decide(bboxes, shape, seed, epoch, batch, slot, cs, resize_range, resize_prob, flip_prob)
    if d.empty:
        return dict(decision=d, plan=None, flip=False, boxes=np.zeros((0, 4), np.float32), labels=np.zeros((0,), np.int64),
                    coef=np.zeros((2 * cs, 4), np.int32), window=(0, 0, 1, 1))
    new_boxes, new_labels = [], []
    for i, b in enumerate(scale_boxes(bboxes, d.scale)):
        nx, ny = max(0, b[0] - d.crop_x), max(0, b[1] - d.crop_y)
        nw = min(cs, b[0] + b[2] - d.crop_x) - nx - 1
        nh = min(cs, b[1] + b[3] - d.crop_y) - ny - 1
        if nw <= 1 or nx >= cs or nh <= 1 or ny >= cs:
            continue
        new_boxes.append([nx, ny, nw, nh])
        new_labels.append(labels[i])
    plan = data.RegionPlan(d.scale, shape[0], shape[1], (d.crop_x, d.crop_y, cs, cs))
    if d.flip:
        new_boxes = data.DeviceAugmentation.flip_boxes(new_boxes, plan.valid_w)
    coef, window = data.plan_tables(plan, cs, cs)
    return dict(decision=d, plan=plan, flip=bool(d.flip), boxes=np.array(new_boxes, dtype=np.float32).reshape(-1, 4),
                labels=np.array(new_labels, dtype=np.int64).reshape(-1), coef=coef, window=window)


DESC_FIELDS = ('src_offset', 'src_pitch', 'win_x0', 'win_y0', 'win_w', 'win_h', 'valid_w', 'valid_h', 'flip')


def plan_batch(samples, shapes, img_offsets, c_src, index_row, seed, epoch, batch, crop_size, resize_range, resize_prob,
               flip_prob, max_boxes_per_image, max_boxes):
    """The whole batch: samples[m] the dataset's sample dicts ('bboxes' / 'bbox_labels' optional), shapes[m] = (h, w),
    img_offsets[m] the arena byte offset of image m.  -> dict: 'samples' (plan_sample per slot), 'desc' {field: int64 [n]},
    'coef' int32 [n, 2 * cs, 4], 'boxes' float32 [K, 4], 'labels' int64 [K], 'offsets' int32 [n + 1], 'status' int32 [4],
    'annotations' (the kept prefix per slot)."""
    n, cs = len(index_row), crop_size
    per, counts, lost_image, blank, bits = [], [], 0, 0, 0
    desc = {k: np.zeros(n, np.int64) for k in DESC_FIELDS}
    coef = np.zeros((n, 2 * cs, 4), np.int32)
    for i, m in enumerate(index_row):
        s = samples[m]
        ps = plan_sample(s.get('bboxes', []), s.get('bbox_labels', []), shapes[m], seed, epoch, batch, i, cs, resize_range,
                         resize_prob, flip_prob)
        per.append(ps)
        x0, y0, ww, wh = ps['window']
        pitch = shapes[m][1] * c_src
        valid = 0 if ps['plan'] is None else cs
        for k, v in zip(DESC_FIELDS, (int(img_offsets[m]) + y0 * pitch + x0 * c_src, pitch, x0, y0, ww, wh, valid, valid,
                                      int(ps['flip']))):
            desc[k][i] = v
        coef[i] = ps['coef']
        if ps['plan'] is None:
            blank += 1
            bits |= EMPTY_RESIZE
        g = len(ps['boxes'])
        counts.append(min(g, max_boxes_per_image))
        lost_image += g - counts[-1]
    if lost_image:
        bits |= IMAGE_OVERFLOW
    offsets, lost_batch, run = [0], 0, 0
    for c in counts:
        take = min(c, max_boxes - run)
        lost_batch += c - take
        run += take
        offsets.append(run)
    if lost_batch:
        bits |= BATCH_OVERFLOW
    ann = [(ps['boxes'][:offsets[i + 1] - offsets[i]], ps['labels'][:offsets[i + 1] - offsets[i]]) for i, ps in enumerate(per)]
    return dict(samples=per, desc=desc, coef=coef,
                boxes=np.concatenate([a for a, _ in ann], 0).reshape(-1, 4), labels=np.concatenate([l for _, l in ann], 0),
                offsets=np.array(offsets, np.int32), status=np.array([bits, lost_image, lost_batch, blank], np.int32),
                annotations=ann)
