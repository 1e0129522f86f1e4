"""tests/golden/make_golden_region_sampler.py -- regenerates ref_region_sampler.npz: what the REAL reference region samplers
(lfd/data_pipeline/sampler/region_sampler.py, loaded by file path) decide for seeded inputs.

    python tests/golden/make_golden_region_sampler.py [reference root]

cv2 is replaced by a stub whose resize returns zeros of cv2's output size for dsize (0, 0) (round half to even of
W * fx, H * fy), and crop_from_image is replaced to record the crop region, so no pixel is computed.  Per case: the sampler
settings, the image size, the input boxes and labels, and -- under random.seed(case seed) -- the resize scale, dsize,
crop region, output boxes and labels, Idle's three meta keys, and the next random() after the call (the draw count).
The inputs come from numpy's RandomState, so the global `random` state is the sampler's alone.
"""
import importlib.util
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from oracle import ref_import  # noqa: E402  (where the reference checkout lives: REF_ROOT)
CROP_SIZES = (480, 512, 640)
PROBS = (0.0, 0.5, 1.0)
NUM_CASES = 360


def load_reference_sampler(ref_root):
    stub = types.ModuleType('cv2')

    def resize(image, dsize, fx=None, fy=None):
        assert tuple(dsize) == (0, 0)
        h, w = int(np.rint(image.shape[0] * fy)), int(np.rint(image.shape[1] * fx))
        assert h > 0 and w > 0
        return np.zeros((h, w) + image.shape[2:], dtype=image.dtype)
    stub.resize = resize
    sys.modules['cv2'] = stub
    path = os.path.join(ref_root, 'lfd', 'data_pipeline', 'sampler', 'region_sampler.py')
    spec = importlib.util.spec_from_file_location('ref_region_sampler', path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_case(k):
    """-> (kind, crop, prob, lo, hi, (h, w), boxes [g,4] float64, labels [g]) from RandomState(k)"""
    rs = np.random.RandomState(k)
    kind = 1 if k % 9 == 8 else 0                      # 1: IdleRegionSampler
    crop = CROP_SIZES[k % 3]
    prob = PROBS[(k // 3) % 3]
    lo, hi = (0.5, 1.5) if k % 5 else (0.3, 2.0)
    size_mode = rs.randint(4)
    if size_mode == 0:       # smaller than the crop
        h, w = rs.randint(8, crop // 2), rs.randint(8, crop // 2)
    elif size_mode == 1:
        h, w = rs.randint(crop // 2, crop * 2), rs.randint(crop // 2, crop * 2)
    else:                     # WIDER-like
        h, w = rs.randint(300, 1400), rs.randint(600, 1100)
    g = 0 if rs.rand() < 0.2 else rs.randint(1, 12)   # negatives
    boxes = np.zeros((g, 4))
    for i in range(g):
        big = rs.rand() < 0.15                             # larger than the crop
        bw = rs.randint(crop, 2 * crop) if big else rs.choice([rs.randint(1, 6), rs.randint(6, 200)])
        bh = rs.randint(crop, 2 * crop) if big else rs.choice([rs.randint(1, 6), rs.randint(6, 200)])
        bx, by = rs.randint(-10, max(1, w - 1)), rs.randint(-10, max(1, h - 1))
        boxes[i] = (bx, by, bw, bh)
        if rs.rand() < 0.3:
            boxes[i] += rs.rand(4) * 0.99                 # float annotations
    labels = rs.randint(0, 3, size=g)
    return kind, crop, prob, lo, hi, (h, w), boxes, labels


def run_reference(mod, case, seed):
    kind, crop, prob, lo, hi, (h, w), boxes, labels = case
    rec = {}
    real_crop = mod.crop_from_image

    def crop_from_image(image, region):   # (the real one fails on a crop that misses the image; no pixel is needed here)
        rec['crop'] = tuple(int(v) for v in region)
        rec['dsize'] = (image.shape[1], image.shape[0])
        return np.zeros((region[3], region[2]) + image.shape[2:], dtype=image.dtype)
    mod.crop_from_image = crop_from_image
    sample = {'image': np.zeros((h, w, 3), np.uint8)}
    if len(boxes):
        sample['bboxes'] = [list(b) for b in boxes]
        sample['bbox_labels'] = [int(v) for v in labels]
    random.seed(seed)
    if kind == 1:
        out = mod.IdleRegionSampler()(sample)
        rec['crop'] = (0, 0, w, h)
        rec['dsize'] = (w, h)
        rec['scale'] = out['resize_scale']
        rec['meta'] = (out['resize_scale'], out['resized_height'], out['resized_width'])
    else:
        orig_resize = sys.modules['cv2'].resize

        def resize(image, dsize, fx=None, fy=None):
            rec['scale'] = fx
            return orig_resize(image, dsize, fx, fy)
        mod.cv2.resize = resize
        out = mod.RandomBBoxCropRegionSampler(crop, (lo, hi), prob)(sample)
        mod.cv2.resize = orig_resize
        rec['meta'] = (0.0, 0, 0)
    rec['post'] = random.random()
    rec['boxes'] = np.array(out.get('bboxes', []), dtype=np.float64).reshape(-1, 4)
    rec['labels'] = np.array(out.get('bbox_labels', []), dtype=np.int64)
    mod.crop_from_image = real_crop
    return rec


def main():
    ref_root = sys.argv[1] if len(sys.argv) > 1 else ref_import.REF_ROOT
    mod = load_reference_sampler(ref_root)
    cols = {k: [] for k in ('kind', 'crop_size', 'prob', 'range', 'shape', 'in_offsets', 'scale', 'dsize', 'crop', 'meta',
                            'post', 'out_offsets')}
    in_boxes, in_labels, out_boxes, out_labels = [], [], [], []
    ni = no = 0
    for k in range(NUM_CASES):
        case = make_case(k)
        rec = run_reference(mod, case, 1000 + k)
        kind, crop, prob, lo, hi, shape, boxes, labels = case
        cols['kind'].append(kind); cols['crop_size'].append(crop); cols['prob'].append(prob); cols['range'].append((lo, hi))
        cols['shape'].append(shape)
        in_boxes.append(boxes); in_labels.append(labels)
        ni += len(boxes); cols['in_offsets'].append(ni)
        cols['scale'].append(rec['scale']); cols['dsize'].append(rec['dsize']); cols['crop'].append(rec['crop'])
        cols['meta'].append(rec['meta']); cols['post'].append(rec['post'])
        out_boxes.append(rec['boxes']); out_labels.append(rec['labels'])
        no += len(rec['boxes']); cols['out_offsets'].append(no)
    arrays = {k: np.array(v) for k, v in cols.items()}
    arrays['in_boxes'] = np.concatenate(in_boxes).reshape(-1, 4)
    arrays['in_labels'] = np.concatenate(in_labels).astype(np.int64)
    arrays['out_boxes'] = np.concatenate(out_boxes).reshape(-1, 4)
    arrays['out_labels'] = np.concatenate(out_labels).astype(np.int64)
    path = os.path.join(HERE, 'ref_region_sampler.npz')
    np.savez_compressed(path, **arrays)
    print('wrote', path, NUM_CASES, 'cases,', ni, 'input boxes,', no, 'output boxes,',
          int((arrays['kind'] == 1).sum()), 'idle')


if __name__ == '__main__':
    main()
