"""The synthetic dataset and settings the resident-loader tests share (tests/test_resident_plan_host.py on the host,
tests/test_gpu_resident_loader.py on the device): 12 images, 37x53 up to 200x300, built to include two gray images, two
images without boxes, one image with 70 boxes, boxes wider or taller than the crop, boxes partly outside the image and one
image smaller than the crop; one box lies outside its image, so that a crop can miss the image altogether."""
import numpy as np

CROP, BATCH = 64, 8
RESIZE_RANGE, RESIZE_PROB, FLIP_PROB = (0.5, 1.5), 0.5, 0.5
SEED = 5     # a seed under which every case above occurs in the 6 planned batches (the tests assert that it does)
EPOCHS = 2
# every image appears; the 70-box image (index 5) twice in the second batch, so that the batch capacity overflows too
ROWS = [[0, 1, 2, 3, 4, 5, 6, 7], [8, 5, 10, 11, 5, 3, 9, 10], [11, 4, 2, 9, 7, 6, 1, 8]]
SHAPES = [(37, 53), (200, 300), (120, 90), (64, 64), (150, 211), (200, 300), (99, 173), (83, 300), (200, 61), (131, 77),
          (65, 250), (177, 149)]
GRAY = (2, 9)
NO_BOXES = (3, 8)
MANY = 5


class Sampler(object):
    """a fixed list of index batches (the reference's dataset samplers have the same interface)"""

    def __init__(self, batches):
        self.batches = batches

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)

    def get_batch_size(self):
        return len(self.batches[0])


def dataset():
    rs = np.random.RandomState(77)
    out = []
    for i, (h, w) in enumerate(SHAPES):
        im = rs.randint(0, 256, size=(h, w) if i in GRAY else (h, w, 3)).astype(np.uint8)
        s = {'image': im, 'id': i, 'name': 'img%02d' % i}
        if i in NO_BOXES:
            out.append(s)
            continue
        if i == MANY:       # 70 small boxes packed into a 90 x 90 corner: one crop keeps dozens
            xy = rs.uniform(60, 150, size=(70, 2))
            wh = rs.uniform(5, 14, size=(70, 2))
            boxes = np.concatenate([xy, wh], 1)
        else:
            g = int(rs.randint(2, 7))
            xy = rs.uniform(0, [w * 0.7, h * 0.7], size=(g, 2))
            wh = rs.uniform(6, 40, size=(g, 2))
            boxes = np.concatenate([xy, wh], 1)
        boxes = [[float(v) for v in b] for b in boxes]
        if i == 1:
            boxes[0] = [20.5, 30.25, 160.0, 22.0]        # wider than the crop at every scale
            boxes[1] = [100.0, 10.0, 18.5, 150.75]       # taller than the crop at every scale
        if i == 4:
            boxes[0] = [-12.5, 40.0, 50.0, 30.0]         # partly left of the image
            boxes[1] = [190.0, 130.0, 60.0, 45.5]        # beyond the right / bottom edge
            boxes = boxes[:2] + [[330.0, 40.0, 30.0, 30.0]]  # outside the image: as the target, the crop misses the image
        if i == 6:
            boxes = [[int(v) for v in b] for b in boxes]  # integer annotations, as most datasets hold them
        s['bboxes'] = boxes
        s['bbox_labels'] = [int(v) for v in rs.randint(0, 3, size=len(boxes))]
        out.append(s)
    return out
