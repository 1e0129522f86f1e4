"""The resident loader on the MI355X (csrc/batch_plan.hip through lfd_amd.data.ResidentDataLoader): the planning kernels
against the contract restated in Python (tests/golden/resident_plan_oracle.py) integer for integer and float32 bit for bit,
the assembled images against the host composition of the oracle's plans, the capacities, the independence of a batch from
what was drawn before, and training fed with DeviceAnnotations against training fed with their host copy."""
import numpy as np
import pytest
import torch

import resident_cases as RC
import resident_plan_oracle as oracle
from lfd_amd import configs, data, optim, train

pytestmark = pytest.mark.gpu

GUARD = 256      # bytes of 0xA5 in front of and behind every guarded buffer


def _sampler():
    return data.RandomBBoxCropRegionSampler(RC.CROP, RC.RESIZE_RANGE, RC.RESIZE_PROB)


def _aug():
    return data.DeviceAugmentation(flip_prob=RC.FLIP_PROB, normalize=data.SIMPLE_NORMALIZE)


def _loader(rds, seed=RC.SEED, **kw):
    return data.ResidentDataLoader(rds, RC.Sampler(RC.ROWS), _sampler(), _aug(), seed=seed, **kw)


def _snapshot(loader, x, ann):
    plan = loader.last_plan
    return dict(x=x.cpu().numpy().copy(), desc=plan.desc_host(), coef=plan.coef.cpu().numpy().copy(),
                boxes=ann.boxes.cpu().numpy().copy(), labels=ann.labels.cpu().numpy().copy(),
                offsets=ann.offsets.cpu().numpy().copy(), status=ann.status(), host=ann.to_host())


@pytest.fixture(scope='module')
def world():
    """the dataset, its resident twin, the oracle's plans and everything the loader produced for 3 batches x 2 epochs"""
    ds = RC.dataset()
    rds = data.ResidentDataset(ds, 'cuda', max_bytes=1 << 24)
    shapes = [s['image'].shape[:2] for s in ds]
    loader = _loader(rds)
    got, metas = {}, {}
    for e in range(RC.EPOCHS):
        for b, (x, ann, meta) in enumerate(loader):
            assert loader.last_h2d_bytes == 0 and len(ann) == RC.BATCH
            got[e, b], metas[e, b] = _snapshot(loader, x, ann), meta
    ref = {(e, b): oracle.plan_batch(ds, shapes, rds.store.offsets, rds.channels, row, RC.SEED, e, b, RC.CROP, RC.RESIZE_RANGE,
                                     RC.RESIZE_PROB, RC.FLIP_PROB, 4096, 4096)
           for e in range(RC.EPOCHS) for b, row in enumerate(RC.ROWS)}
    return dict(ds=ds, rds=rds, shapes=shapes, got=got, ref=ref, metas=metas)


def _assert_plan_equal(g, r, what):
    for i, d in enumerate(g['desc']):
        for k in oracle.DESC_FIELDS:
            assert getattr(d, k) == int(r['desc'][k][i]), (what, i, k, getattr(d, k), int(r['desc'][k][i]))
    assert np.array_equal(g['coef'], r['coef']), what
    assert np.array_equal(g['offsets'], r['offsets']), (what, g['offsets'], r['offsets'])
    k = int(r['offsets'][-1])
    assert np.array_equal(g['boxes'][:k].view(np.uint32), r['boxes'].view(np.uint32)), what
    assert np.array_equal(g['labels'][:k], r['labels']), what
    s = g['status']
    assert [s['bits'], s['dropped_per_image'], s['dropped_batch'], s['blank_images']] == r['status'].tolist(), (what, s)
    assert len(g['host']) == len(r['annotations'])
    for (gb, gl), (rb, rl) in zip(g['host'], r['annotations']):
        assert gb.dtype == np.float32 and gl.dtype == np.int64 and gb.shape == rb.shape
        assert np.array_equal(gb, rb) and np.array_equal(gl, rl), what


def test_resident_dataset_tables(world):
    ds, rds = world['ds'], world['rds']
    assert len(rds) == 12 and rds.channels == 3
    assert rds.img_h.cpu().tolist() == [s[0] for s in world['shapes']] and rds.img_w.cpu().tolist() == [s[1] for s in world['shapes']]
    assert rds.img_offset.dtype == torch.int64 and rds.img_offset.cpu().tolist() == rds.store.offsets.tolist()
    counts = [len(s.get('bboxes', [])) for s in ds]
    assert rds.box_offset.dtype == torch.int32 and rds.box_offset.cpu().tolist() == [0] + list(np.cumsum(counts))
    flat = [b for s in ds for b in s.get('bboxes', [])]
    assert rds.box.dtype == torch.float64 and rds.box.cpu().tolist() == [[float(v) for v in b] for b in flat]
    assert rds.label.cpu().tolist() == [l for s in ds for l in s.get('bbox_labels', [])]
    assert rds.metas[3] == {'id': 3, 'name': 'img03'}


def test_descriptors_tables_boxes_and_status_equal_the_oracle(world):
    cases = dict(flip=0, miss=0, many=0)
    for key, r in world['ref'].items():
        _assert_plan_equal(world['got'][key], r, key)
        assert world['metas'][key] == [{'id': m, 'name': 'img%02d' % m} for m in RC.ROWS[key[1]]]
        cases['flip'] += int(r['desc']['flip'].sum())
        cases['miss'] += sum(ps['window'] == (0, 0, 1, 1) for ps in r['samples'])
        cases['many'] += sum(len(ps['boxes']) > 16 for ps in r['samples'])
    assert cases['flip'] > 0 and cases['miss'] > 0 and cases['many'] > 0, cases
    assert world['got'][0, 0]['status']['bits'] == 0


def test_image_batch_equals_the_host_composition_of_the_oracle_plans(world):
    aug = _aug()
    for (e, b), r in world['ref'].items():
        images = [world['ds'][m]['image'] for m in RC.ROWS[b]]
        plans = [ps['plan'] for ps in r['samples']]
        flips = [ps['flip'] for ps in r['samples']]
        ref = data.compose_host(images, plans, flips, aug, RC.CROP, RC.CROP)
        got = world['got'][e, b]['x']
        assert got.shape == ref.shape == (RC.BATCH, 3, RC.CROP, RC.CROP)
        bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
        assert bad.size == 0, ((e, b), len(bad), bad[:5])


def _guarded(t):
    """a tensor of t's shape and dtype in the middle of a 0xA5-filled allocation -> (tensor, the whole allocation)"""
    nbytes = t.numel() * t.element_size()
    whole = torch.full((nbytes + 2 * GUARD,), 0xA5, dtype=torch.uint8, device=t.device)
    return whole[GUARD:GUARD + nbytes].view(t.dtype).view(t.shape), whole


def test_capacities_keep_the_documented_prefix_and_write_nothing_beyond(world):
    """max_boxes_per_image = 16 and max_boxes = 40: every sample keeps its first 16 boxes, the batch its first 40; offsets
    and status say so; the bytes around every output buffer keep their guard pattern"""
    rds, n, mbpi, mb = world['rds'], RC.BATCH, 16, 40
    over = dict(image=0, batch=0)
    for e in range(RC.EPOCHS):
        for b, row in enumerate(RC.ROWS):
            plan, ann = data.PlanBuffers(n, RC.CROP, mbpi, 'cuda'), data.DeviceAnnotations(n, mb, 'cuda')
            wholes = []
            for obj, names in ((plan, ('desc', 'coef', 'stage_box', 'stage_label', 'stage_count')), (ann, ('buffer', 'status_words'))):
                for name in names:
                    t, whole = _guarded(getattr(obj, name))
                    setattr(obj, name, t)
                    wholes.append((name, whole, t.numel() * t.element_size()))
            ann.boxes = ann.buffer[:16 * mb].view(torch.float32).view(mb, 4)
            ann.labels = ann.buffer[16 * mb:24 * mb].view(torch.int64)
            ann.offsets = ann.buffer[24 * mb:].view(torch.int32)
            idx = torch.tensor(row, dtype=torch.int32, device='cuda')
            data.plan_bbox_crop_batch(rds, idx, RC.SEED, e, b, RC.CROP, RC.RESIZE_RANGE, RC.RESIZE_PROB, RC.FLIP_PROB, plan, ann)
            torch.cuda.synchronize()
            for name, whole, nbytes in wholes:
                w = whole.cpu().numpy()
                assert (w[:GUARD] == 0xA5).all() and (w[GUARD + nbytes:] == 0xA5).all(), ((e, b), name)
            r = oracle.plan_batch(world['ds'], world['shapes'], rds.store.offsets, rds.channels, row, RC.SEED, e, b, RC.CROP,
                                  RC.RESIZE_RANGE, RC.RESIZE_PROB, RC.FLIP_PROB, mbpi, mb)
            full = world['ref'][e, b]
            g = dict(desc=plan.desc_host(), coef=plan.coef.cpu().numpy(), boxes=ann.boxes.cpu().numpy(),
                     labels=ann.labels.cpu().numpy(), offsets=ann.offsets.cpu().numpy(), status=ann.status(), host=ann.to_host())
            _assert_plan_equal(g, r, ('capacity', e, b))
            # the documented prefix, stated without the oracle's own clipping: the first min(g, 16) boxes of every sample, then
            # the first 40 of the batch
            kept = [a[:mbpi] for a, _ in full['annotations']]
            flat = np.concatenate(kept, 0)[:mb]
            offs = np.minimum(np.concatenate([[0], np.cumsum([len(k) for k in kept])]), mb)
            assert np.array_equal(g['offsets'], offs) and np.array_equal(g['boxes'][:len(flat)], flat)
            st = g['status']
            assert st['dropped_per_image'] == sum(max(0, len(a) - mbpi) for a, _ in full['annotations'])
            assert st['dropped_batch'] == sum(len(k) for k in kept) - len(flat)
            assert st['bits'] == (2 if st['dropped_per_image'] else 0) | (4 if st['dropped_batch'] else 0)
            over['image'] += st['dropped_per_image'] > 0
            over['batch'] += st['dropped_batch'] > 0
    assert over['image'] > 0 and over['batch'] > 0, over


def test_an_empty_resize_and_an_index_out_of_range_give_blank_samples_and_status_bits():
    ds = [{'image': np.full((1, 5, 3), 200, np.uint8), 'bboxes': [[0.0, 0.0, 3.0, 1.0]], 'bbox_labels': [1]},
          {'image': np.full((40, 50, 3), 100, np.uint8), 'bboxes': [[5.0, 6.0, 20.0, 21.0]], 'bbox_labels': [2]}]
    rds = data.ResidentDataset(ds, 'cuda', max_bytes=1 << 20)
    rows = [[0, 1, 0, 1]]
    loader = data.ResidentDataLoader(rds, RC.Sampler(rows), data.RandomBBoxCropRegionSampler(16, (0.03, 0.04), 1.0),
                                     data.DeviceAugmentation(flip_prob=0.5), seed=3, max_boxes=8)
    (x, ann, _), = list(loader)
    r = oracle.plan_batch(ds, [(1, 5), (40, 50)], rds.store.offsets, 3, rows[0], 3, 0, 0, 16, (0.03, 0.04), 1.0, 0.5, 8, 8)
    assert r['status'][0] == oracle.EMPTY_RESIZE and r['status'][3] == 2        # the 1 x 5 image vanishes, the other does not
    _assert_plan_equal(_snapshot(loader, x, ann), r, 'empty')
    xh = x.cpu().numpy()
    assert not xh[0].any() and not xh[2].any() and xh[1].any()
    # an index beyond the dataset: planned as a blank sample, flagged, nothing read
    plan, ann = data.PlanBuffers(4, 16, 8, 'cuda'), data.DeviceAnnotations(4, 8, 'cuda')
    idx = torch.tensor([1, 2, -1, 1], dtype=torch.int32, device='cuda')
    data.plan_bbox_crop_batch(rds, idx, 3, 0, 0, 16, (1.0, 1.0), 0.0, 0.0, plan, ann)
    st, desc = ann.status(), plan.desc_host()
    assert st['bits'] == 8 and st['blank_images'] == 2
    assert [d.valid_w for d in desc] == [16, 0, 0, 16] and ann.offsets.cpu().tolist() == [0, 1, 1, 1, 2]


def test_a_batch_depends_on_seed_epoch_and_index_only(world):
    rds = world['rds']
    fresh = _loader(rds)
    for e, b in ((1, 2), (0, 1), (1, 2)):        # out of order, on a loader that has drawn nothing else, and twice
        idx = torch.tensor(RC.ROWS[b], dtype=torch.int32, device='cuda')
        x, ann = fresh.draw(idx, e, b)
        g = _snapshot(fresh, x, ann)
        w = world['got'][e, b]
        assert np.array_equal(g['x'].view(np.uint32), w['x'].view(np.uint32)), (e, b)
        _assert_plan_equal(g, world['ref'][e, b], ('fresh', e, b))
    other = _loader(rds, seed=RC.SEED + 1)
    x, ann, _ = next(iter(other))
    assert not np.array_equal(x.cpu().numpy(), world['got'][0, 0]['x'])
    with pytest.raises(TypeError):
        data.ResidentDataLoader(rds, RC.Sampler(RC.ROWS), data.IdleRegionSampler(), _aug(), seed=1)
    with pytest.raises(ValueError):
        data.ResidentDataLoader(rds, RC.Sampler(RC.ROWS), _sampler(), _aug(), seed=None)


def test_training_fed_device_annotations_equals_training_fed_their_host_copy(world):
    """WIDERFACE_LFD_XS at 96 x 96 (tests/test_gpu_train.py trains it at 96 x 128 and 64 x 96): two GraphedTrainStep iterations
    fed DeviceAnnotations, with equal and with larger capacity, and fed .to_host() give bit-equal loss values, gradient norms
    and parameters; LFD.get_loss takes both forms; the host route refuses DeviceAnnotations"""
    rds, crop, bs = world['rds'], 96, 4
    rows = [r[:bs] for r in RC.ROWS[:2]]
    loader = data.ResidentDataLoader(rds, RC.Sampler(rows), data.RandomBBoxCropRegionSampler(crop, RC.RESIZE_RANGE, RC.RESIZE_PROB),
                                     _aug(), seed=3, max_boxes=64)
    torch.manual_seed(11)
    models = [configs.build_model('WIDERFACE_LFD_XS').cuda().train() for _ in range(4)]
    for m in models[1:]:
        m.load_state_dict(models[0].state_dict())
    probe = models.pop()       # get_loss only: its forward moves the norm statistics, so it is not one of the trained twins
    opts = [optim.SGD(m.parameters(), lr=0.02, momentum=0.9, weight_decay=1e-4) for m in models]
    clip = dict(max_norm=10, norm_type=2)
    steps = [train.GraphedTrainStep(m, o, clip, max_boxes=mb) for m, o, mb in zip(models, opts, (64, 64, 128))]
    boxes_seen = 0
    for x, ann, _ in loader:
        host = ann.to_host()
        boxes_seen += sum(len(b) for b, _ in host)
        with torch.no_grad():
            pred = probe(x)
        la = probe.get_loss(pred, ann)['loss_values']
        lh = probe.get_loss(pred, host)['loss_values']
        assert la == lh, (la, lh)
        with pytest.raises(RuntimeError):
            probe.get_loss((pred[0].cpu(), pred[1].cpu()), ann)
        (l0, n0), (l1, n1), (l2, n2) = steps[0](x, ann, True), steps[1](x, host, True), steps[2](x, ann, True)
        assert l0 == l1 == l2, (l0, l1, l2)
        assert float(n0) == float(n1) == float(n2)
    assert boxes_seen > 0
    for m in models[1:]:
        for p, q in zip(models[0].parameters(), m.parameters()):
            assert torch.equal(p, q)
        for p, q in zip(models[0].buffers(), m.buffers()):
            assert torch.equal(p, q)
    small = train.GraphedTrainStep(models[0], opts[0], clip, max_boxes=32)
    with pytest.raises(RuntimeError):
        small(x, ann, True)
