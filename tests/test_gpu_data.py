"""Device batch assembly (csrc/batch_assemble.hip through lfd_amd/data.py) on the MI355X: the kernel against the contract
restated in numpy (tests/golden/batch_oracle.py) bit for bit, the store path against the staging path, the seeded loader
against its worker count and against the host-composed batch, and training fed from the loader."""
import random

import numpy as np
import pytest
import torch

import batch_oracle
from lfd_amd import configs, data, optim, train

pytestmark = pytest.mark.gpu


def _check(images, plans, flips, aug, cmap_rgb=(0, 1, 2)):
    got = data.assemble_batch(images, plans, flips, aug, 'cuda').cpu().numpy()
    h, w = max(p.valid_h for p in plans), max(p.valid_w for p in plans)
    ref = batch_oracle.compose(images, [p.scale for p in plans], [p.crop for p in plans], flips, aug.lut(), list(cmap_rgb),
                               aug.out_channels, h, w)
    assert got.shape == ref.shape
    bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
    assert bad.size == 0, (len(bad), bad[:5])


def _img(rs, h, w, c=3):
    return rs.randint(0, 256, size=(h, w, c) if c else (h, w)).astype(np.uint8)


def test_kernel_random_scales_and_crops_off_every_edge():
    rs = np.random.RandomState(0)
    S = 64
    plans, images, flips = [], [], []
    offs = [(-20, -20), (40, -10), (-10, 40), (50, 50), (-100, -100), (10, 10)]   # off each edge, a crop larger than the image
    for i in range(12):
        h, w = int(rs.randint(20, 120)), int(rs.randint(20, 120))
        s = float(rs.uniform(0.5, 1.5))
        rh, rw = data.resized_size(h, w, s)
        ox, oy = offs[i % len(offs)]
        cx = ox if ox < 0 else rw - S + ox if i % 2 else int(rs.randint(0, max(1, rw - S)))
        cy = oy if oy < 0 else rh - S + oy
        plans.append(data.RegionPlan(s, h, w, (cx, cy, S, S)))
        images.append(_img(rs, h, w))
        flips.append(bool(i % 3 == 0))
    plans.append(data.RegionPlan(0.7, 20, 20, (-80, -90, S, S)))     # a crop that misses the image: uint8 0 -> lut[0]
    images.append(_img(rs, 20, 20))
    flips.append(False)
    _check(images, plans, flips, data.DeviceAugmentation(flip_prob=0.5, normalize=data.SIMPLE_NORMALIZE))
    _check(images, plans, flips, data.DeviceAugmentation(normalize=data.STANDARD_NORMALIZE, bgr2rgb=True), (2, 1, 0))


@pytest.mark.parametrize('scale', [1.0, 0.5, 1.5])
def test_kernel_fixed_scales_and_tiny_sources(scale):
    rs = np.random.RandomState(1)
    shapes = [(1, 1), (2, 3), (3, 2), (7, 9), (33, 17), (64, 48)]
    plans, images = [], []
    for h, w in shapes:
        try:
            rh, rw = data.resized_size(h, w, scale)
        except ValueError:
            continue
        plans.append(data.RegionPlan(scale, h, w, (-2, -1, 24, 20)))
        images.append(_img(rs, h, w))
    flips = [bool(i % 2) for i in range(len(plans))]
    _check(images, plans, flips, data.DeviceAugmentation(normalize=data.CAFFE_IMAGENET_NORMALIZE))
    if scale == 1.0:   # identity: the crop of the source itself
        out = data.assemble_batch([images[-1]], [data.RegionPlan(1.0, 64, 48, (0, 0, 48, 64))], [False],
                                  data.DeviceAugmentation(normalize=None), 'cuda').cpu().numpy()
        assert np.array_equal(out[0], images[-1].transpose(2, 0, 1).astype(np.float32))


def test_kernel_gray_sources_one_and_three_output_channels():
    rs = np.random.RandomState(2)
    plans = [data.RegionPlan(float(s), 50, 70, (-5, 3, 40, 40)) for s in (0.6, 1.0, 1.37)]
    images = [_img(rs, 50, 70, 0) for _ in plans]
    flips = [False, True, True]
    _check(images, plans, flips, data.DeviceAugmentation(out_channels=1))
    _check(images, plans, flips, data.DeviceAugmentation(out_channels=3, bgr2rgb=True))
    mixed = [images[0], _img(rs, 50, 70), images[2]]       # a gray image in a colour batch is tiled
    _check(mixed, plans, flips, data.DeviceAugmentation(out_channels=3))


def test_kernel_idle_batches_of_mixed_sizes_pad_with_zero():
    rs = np.random.RandomState(3)
    sampler = data.IdleRegionSampler()
    shapes = [(37, 53), (61, 29), (12, 77), (61, 77)]
    for sub in (shapes[:3], shapes):             # w_out 77 (scalar stores), then 77 again with a full-size image
        plans = [sampler({}, (h, w, 3)) for h, w in sub]
        images = [_img(rs, h, w) for h, w in sub]
        _check(images, plans, [False] * len(sub), data.DeviceAugmentation())
        _check(images, plans, [True] * len(sub), data.DeviceAugmentation())
    plans = [sampler({}, (h, w, 3)) for h, w in [(40, 64), (23, 31)]]    # w_out 64: 16-byte stores, padding in a vector
    _check([_img(rs, 40, 64), _img(rs, 23, 31)], plans, [False, True], data.DeviceAugmentation())
    out = data.assemble_batch([_img(rs, 40, 64), _img(rs, 23, 31)], plans, [False, False],
                              data.DeviceAugmentation(), 'cuda').cpu().numpy()
    assert not out[1, :, 23:].any() and not out[1, :, :, 31:].any()      # 0.0, not lut[0] = -1.0


class _Sampler(object):
    """a fixed list of index batches (the reference's dataset samplers have the same interface)"""

    def __init__(self, batches):
        self.batches = batches

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)

    def get_batch_size(self):
        return len(self.batches[0])


def _dataset(n, seed, gray=False):
    rs = np.random.RandomState(seed)
    out = []
    for i in range(n):
        h, w = int(rs.randint(60, 260)), int(rs.randint(80, 300))
        im = _img(rs, h, w, 0 if gray else 3)
        g = int(rs.randint(0, 5))
        wh = rs.randint(8, 60, size=(g, 2))
        xy = rs.randint(0, 40, size=(g, 2))
        s = {'image': im, 'id': i}
        if g:
            s['bboxes'] = [list(map(int, v)) for v in np.concatenate([xy, wh], 1)]
            s['bbox_labels'] = [0] * g
        out.append(s)
    return out


def _batches(n, bs, seed):
    idx = np.random.RandomState(seed).permutation(n)
    return [list(map(int, idx[i:i + bs])) for i in range(0, n - bs + 1, bs)]


def _collect(loader):
    return [(x.cpu().numpy().copy(), ann, meta) for x, ann, meta in loader]


def _same(a, b):
    assert len(a) == len(b)
    for (xa, aa, ma), (xb, ab, mb) in zip(a, b):
        assert np.array_equal(xa.view(np.uint32), xb.view(np.uint32))
        assert ma == mb
        for (ba, la), (bb, lb) in zip(aa, ab):
            assert np.array_equal(ba, bb) and np.array_equal(la, lb)


def test_store_path_equals_staging_path():
    ds = _dataset(12, 4)
    ds[3]['image'] = ds[3]['image'][:, :, 0]           # a gray image among colour ones
    store = data.DeviceImageStore(ds, 'cuda', max_bytes=1 << 24)
    assert store.channels == 3 and store.nbytes == sum(s['image'].shape[0] * s['image'].shape[1] * 3 for s in ds)
    rs = np.random.RandomState(5)
    sampler = data.RandomBBoxCropRegionSampler(96, (0.5, 1.5), 0.5)
    idx = [3, 0, 7, 11, 5]
    plans = [sampler(dict(ds[i]), ds[i]['image'].shape, random.Random(int(rs.randint(1 << 30)))) for i in idx]
    flips = [bool(k % 2) for k in range(len(idx))]
    aug = data.DeviceAugmentation(normalize=data.STANDARD_NORMALIZE, bgr2rgb=True)
    a = data.assemble_batch([ds[i]['image'] for i in idx], plans, flips, aug, 'cuda')
    b = data.assemble_batch(None, plans, flips, aug, 'cuda', store=store, indices=idx)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    mk = lambda st: data.DeviceDataLoader(ds, _Sampler(_batches(12, 4, 1)), sampler, aug, 'cuda', num_workers=2, seed=9,
                                          store=st)
    la, lb = mk(None), mk(store)
    _same(_collect(la), _collect(lb))
    assert lb.last_h2d_bytes < la.last_h2d_bytes
    with pytest.raises(RuntimeError):
        data.DeviceImageStore(ds, 'cuda', max_bytes=1000)


def test_seeded_loader_does_not_depend_on_the_worker_count_and_equals_the_host_batch():
    ds = _dataset(24, 6)
    batches = _batches(24, 4, 2)
    aug = data.DeviceAugmentation(flip_prob=0.5, normalize=data.SIMPLE_NORMALIZE)
    sampler = data.RandomBBoxCropRegionSampler(128, (0.5, 1.5), 0.5)
    l1 = data.DeviceDataLoader(ds, _Sampler(batches), sampler, aug, 'cuda', num_workers=1, seed=11)
    l4 = data.DeviceDataLoader(ds, _Sampler(batches), sampler, aug, 'cuda', num_workers=4, seed=11)
    r1, r4 = _collect(l1), _collect(l4)
    _same(r1, r4)
    assert len(r1) == len(l1) == 6 and r1[0][0].shape == (4, 3, 128, 128)
    for b, (x, ann, meta) in enumerate(r1):
        hx, hann, hmeta = l1.host_batch(batches[b], 0, b)
        assert np.array_equal(x.view(np.uint32), hx.view(np.uint32)), b
        assert meta == hmeta == [{'id': i} for i in batches[b]]
        for (ba, la), (bb, lb) in zip(ann, hann):
            assert ba.dtype == np.float32 and la.dtype == np.int64
            assert np.array_equal(ba, bb) and np.array_equal(la, lb)
    second = _collect(l1)                                    # epoch 1 draws differently
    assert not all(np.array_equal(a[0], b[0]) for a, b in zip(r1, second))
    idle = data.DeviceDataLoader(ds, _Sampler(batches[:2]), data.IdleRegionSampler(), data.DeviceAugmentation(), 'cuda',
                                 num_workers=2, seed=3)
    for b, (x, ann, meta) in enumerate(idle):
        hx, _, hmeta = idle.host_batch(batches[b], 0, b)
        assert np.array_equal(x.cpu().numpy(), hx) and meta == hmeta
        assert meta[0]['resize_scale'] == 1.0 and 'resized_height' in meta[0]


@pytest.mark.parametrize('gray', [False, True])
def test_training_fed_from_the_loader_equals_training_on_the_host_batch(gray):
    """WIDERFACE_LFD_S (and its gray twin): train_step and GraphedTrainStep fed the loader's device batches give the same loss
    values, bit for bit, as the same steps fed the host-composed batches.  The loop keeps one batch drawn ahead (the
    documented lifetime: a batch stays valid on the drawing stream until two more have been drawn)."""
    ds = _dataset(24, 7, gray)
    batches = _batches(24, 4, 3)
    aug = data.DeviceAugmentation(flip_prob=0.5, out_channels=1 if gray else 3)
    loader = data.DeviceDataLoader(ds, _Sampler(batches), data.RandomBBoxCropRegionSampler(160, (0.5, 1.5), 0.5), aug,
                                   'cuda', num_workers=3, seed=21)
    torch.manual_seed(5)
    kw = dict(input_channels=1) if gray else {}
    models = [configs.build_model('WIDERFACE_LFD_S', **kw).cuda().train() for _ in range(4)]
    for m in models[1:]:
        m.load_state_dict(models[0].state_dict())
    opts = [optim.SGD(m.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4) for m in models]
    clip = dict(max_norm=10, norm_type=2)
    ga = train.GraphedTrainStep(models[2], opts[2], clip, max_boxes=64)
    gb = train.GraphedTrainStep(models[3], opts[3], clip, max_boxes=64)
    it = iter(loader)
    nxt = next(it)
    for b in range(len(batches)):
        x, ann, _ = nxt
        nxt = next(it, None)                                 # draw ahead before the step reads x
        hx = torch.from_numpy(loader.host_batch(batches[b], 0, b)[0]).cuda()
        lva, _ = train.train_step(models[0], opts[0], x, ann, clip, True)
        lvb, _ = train.train_step(models[1], opts[1], hx, ann, clip, True)
        assert lva == lvb, (b, lva, lvb)
        lga, _ = ga(x, ann, True)
        lgb, _ = gb(hx, ann, True)
        assert lga == lgb, (b, lga, lgb)
    assert nxt is None and len(ga.graphs) == 1


def test_kernel_idle_batches_wider_than_one_column_tile():
    """w_out > 1024: several column tiles per image row (x0 > 0), with scalar (1030) and 16-byte (1028) stores"""
    rs = np.random.RandomState(9)
    sampler = data.IdleRegionSampler()
    for shapes in ([(7, 1030), (5, 611), (9, 1029)], [(6, 1028), (4, 1027), (3, 2052)]):
        plans = [sampler({}, (h, w, 3)) for h, w in shapes]
        images = [_img(rs, h, w) for h, w in shapes]
        _check(images, plans, [False] * len(shapes), data.DeviceAugmentation())
        _check(images, plans, [True, False, True], data.DeviceAugmentation(normalize=data.STANDARD_NORMALIZE, bgr2rgb=True),
               (2, 1, 0))


def test_a_batch_held_across_an_epoch_boundary_stays_valid():
    """An odd number of batches per epoch: the last batch of an epoch and the first of the next must not share an output
    buffer.  Drawing one batch ahead across the boundary, the held batch still equals its host-composed twin."""
    ds = _dataset(12, 12)
    batches = _batches(12, 4, 5)
    assert len(batches) == 3
    loader = data.DeviceDataLoader(ds, _Sampler(batches), data.RandomBBoxCropRegionSampler(64, (0.5, 1.5), 0.5),
                                   data.DeviceAugmentation(flip_prob=0.5), 'cuda', num_workers=2, seed=4)

    def stream(epochs):
        for e in range(epochs):
            for b, item in enumerate(loader):
                yield e, b, item
    it = stream(3)
    held = next(it)
    checked = 0
    for nxt in it:
        e, b, (x, ann, meta) = held                       # `nxt` has been drawn: its kernel is enqueued
        assert np.array_equal(x.cpu().numpy(), loader.host_batch(batches[b], e, b)[0]), (e, b)
        checked += 1
        held = nxt
    assert checked == 8
