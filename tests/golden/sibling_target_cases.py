"""tests/golden/sibling_target_cases.py -- the edge-case batch and case tables of the sibling target assignment, shared by
the fixture generator (make_golden_sibling_targets.py, runs the reference) and the tests that read ref_sibling_targets.npz
(CPU suite: host mirrors; GPU suite: lfd_assign_targets_fcos_f32 / lfd_assign_targets_v2_f32).  Nothing here touches the
reference.

Three levels of 12x16, 6x8 and 3x4 points at strides 8, 16, 32 (a 96x128 image, P = 252), n = 3 images:
  image 0   no boxes
  image 1   box 0  (16, 8, 33, 25)   right / top edges ON points: x + w - 1 = 48 and y = 8 are grid coordinates, so the
                                     distance there is exactly 0 -- outside for FCOS (> 0), inside for LFDv2 (>= 0, score 0);
                                     longer side 33: LFDv2's right gray band of level 0 ((35 - 33) / (35 - 32))
            box 1  (40, 40, 20, 30)  class 0 \\ equal areas (600) over the points (48|56, 48|56): FCOS takes the lower index;
            box 2  (35, 45, 30, 20)  class 1 /  longer side 30: inside level 0, left gray band of level 1 ((30 - 28) / 4)
            box 3  (32, 8, 50, 20)   at the point (64, 16) -- a point of level 0 AND of level 1 -- the largest distance is
                                     exactly 32 = the upper bound of level 0 and the lower bound of level 1 (both inclusive)
            box 4  (44, 44, 9, 9)    class 2 \\ both centres at (48, 48): the point lies in two core zones, both scores are 1
            box 5  (40, 40, 17, 17)  class 2 /  (same class: LFDv2's per-class maximum; score tie -> lowest index)
            box 6  (42, 38, 26, 28)  class 0: a second box of box 1's class over the same points
            box 7  (100, 72, 9, 5)   class 1: the point (104, 72) lies ON its top edge and in its core zone -- LFDv2's
                                     `>= 0` hit test gives it score 1 there, a strict test would give 0
  image 2   box 0  (22, 18, 50, 40)  class 2, box 1 (30, 25, 30, 24) class 0 nested inside it (both valid at (40, 32)),
            boxes 2..69              68 seeded boxes: G = 70 is more than one LDS chunk of the kernels
gt_offsets = (0, 0, 8, 78): uneven.  The last FCOS level's upper bound is 1e8."""
import numpy as np

SIZES = [(12, 16), (6, 8), (3, 4)]
STRIDES = [8, 16, 32]
NUM_CLASSES = 3
N_IMAGES = 3
FCOS_RANGES = ((0, 32), (32, 64), (64, 1e8))
V2_RANGES = ((4, 32), (32, 64), (64, 128))
GRAY_FACTORS = (0.9, 1.1)

# (range_assign_mode, regression loss module): 'shorter' / 'sqrt' need a union (IoU-type) loss (lfdv2.py:176-178)
V2_CASES = [('longer', 'IoULoss'), ('shorter', 'IoULoss'), ('sqrt', 'IoULoss'), ('dist', 'IoULoss'),
            ('longer', 'SmoothL1Loss'), ('dist', 'SmoothL1Loss')]


def annotations():
    """-> list of (boxes float32 [G,4] xywh, labels int64 [G]) per image"""
    img1 = np.array([[16, 8, 33, 25], [40, 40, 20, 30], [35, 45, 30, 20], [32, 8, 50, 20], [44, 44, 9, 9], [40, 40, 17, 17],
                     [42, 38, 26, 28], [100, 72, 9, 5]], np.float32)
    lab1 = np.array([1, 0, 1, 2, 2, 2, 0, 1], np.int64)
    rs = np.random.default_rng(31)
    wh = np.exp(rs.uniform(np.log(5), np.log(90), (68, 2)))
    xy = rs.uniform(0, [128, 96], (68, 2)) - wh / 2
    # quarter-pixel coordinates: exact in fp32, and some edges land on grid points
    rnd = (np.round(np.concatenate([xy, wh], 1) * 4) / 4).astype(np.float32)
    img2 = np.concatenate([np.array([[22, 18, 50, 40], [30, 25, 30, 24]], np.float32), rnd])
    lab2 = np.concatenate([np.array([2, 0], np.int64), rs.integers(0, NUM_CLASSES, 68).astype(np.int64)])
    return [(np.zeros((0, 4), np.float32), np.zeros((0,), np.int64)), (img1, lab1), (img2, lab2)]


def total_points():
    return sum(h * w for h, w in SIZES)


def points():
    """[P, 2] (x, y) int64, level-major, row-major"""
    out = []
    for (h, w), s in zip(SIZES, STRIDES):
        ys, xs = np.meshgrid(np.arange(h) * s, np.arange(w) * s, indexing='ij')
        out.append(np.stack([xs.reshape(-1), ys.reshape(-1)], -1))
    return np.concatenate(out).astype(np.int64)
