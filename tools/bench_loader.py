"""Device batch assembly timing (lfd_amd.data.DeviceDataLoader, csrc/batch_assemble.hip) at the WIDERFACE_LFD_S training
setting: bs 64, RandomBBoxCropRegionSampler(480, (0.5, 1.5), 0.5), flip p 0.5, simple_normalize, on seeded synthetic
decoded images of WIDER FACE-like sizes (1024 wide, 400-1400 high, 1-20 boxes).  Prints one JSON line per mode:
  loader        : the loader alone (staging path: windows copied through pinned memory), batches/s
  loader_store  : the loader alone over a DeviceImageStore (descriptors + tables only), batches/s
  fed           : GraphedTrainStep fed by the loader, ms per iteration
  fixed         : the same GraphedTrainStep on one fixed device batch (the ceiling), ms per iteration
  resident      : ResidentDataLoader alone (the plan made on the device, csrc/batch_plan.hip; no per-batch copy), batches/s
  fed_resident  : GraphedTrainStep fed by ResidentDataLoader (DeviceAnnotations), ms per iteration
Each loader mode also reports the host-to-device bytes per batch.  Kernel time: run `--modes loader` under
`rocprofv3 --kernel-trace --stats` in a run of its own.  Not the headline metric (bench.py is); recorded in DESIGN.md."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'lfd-a-light-and-fast-detector_amd'))
from lfd_amd import configs, data, optim, train  # noqa: E402


class Sampler(object):
    """RandomDatasetSampler's interface: shuffled index batches (ignore_last)"""

    def __init__(self, n, batch, seed):
        self.n, self.batch, self.rs = n, batch, np.random.RandomState(seed)

    def __iter__(self):
        idx = self.rs.permutation(self.n)
        return iter([list(map(int, idx[i:i + self.batch])) for i in range(0, self.n - self.batch + 1, self.batch)])

    def __len__(self):
        return self.n // self.batch

    def get_batch_size(self):
        return self.batch


def synthetic_dataset(n, seed):
    rng = np.random.default_rng(seed)
    ds = []
    for i in range(n):
        h, w = int(rng.integers(400, 1400)), 1024
        im = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
        g = int(rng.integers(1, 21))
        wh = np.exp(rng.uniform(np.log(6), np.log(300), (g, 2))).astype(int) + 1
        xy = (rng.uniform(0, 1, (g, 2)) * (np.array([w, h]) - wh).clip(1)).astype(int)
        ds.append({'image': im, 'bboxes': np.concatenate([xy, wh], 1).tolist(), 'bbox_labels': [0] * g, 'id': i})
    return ds


def loader_for(ds, args, store=None):
    return data.DeviceDataLoader(ds, Sampler(len(ds), args.batch, 0), data.RandomBBoxCropRegionSampler(args.crop, (0.5, 1.5), 0.5),
                                 data.DeviceAugmentation(flip_prob=0.5, normalize=data.SIMPLE_NORMALIZE), 'cuda',
                                 num_workers=args.workers, seed=1, store=store)


def resident_loader_for(ds, args, holder):
    if 'resident' not in holder:
        holder['resident'] = data.ResidentDataset(ds, 'cuda', max_bytes=64 << 30)
    return data.ResidentDataLoader(holder['resident'], Sampler(len(ds), args.batch, 0),
                                   data.RandomBBoxCropRegionSampler(args.crop, (0.5, 1.5), 0.5),
                                   data.DeviceAugmentation(flip_prob=0.5, normalize=data.SIMPLE_NORMALIZE), seed=1,
                                   max_boxes=args.batch * 24)


def batches(loader, count):
    """an endless stream of batches over repeated epochs"""
    while True:
        for b in loader:
            yield b
            count -= 1
            if count <= 0:
                return


def time_loader(loader, args):
    it = batches(loader, args.warmup + args.steps)
    for _ in range(args.warmup):
        next(it)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    h2d = 0
    for _ in range(args.steps):
        next(it)
        h2d += loader.last_h2d_bytes
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.steps
    return dt, h2d / args.steps


def run(mode, args, ds, store_holder):
    out = dict(mode=mode, batch=args.batch, crop=args.crop, workers=args.workers, images=len(ds))
    if mode in ('loader', 'loader_store'):
        store = None
        if mode == 'loader_store':
            if 'store' not in store_holder:
                store_holder['store'] = data.DeviceImageStore(ds, 'cuda', max_bytes=64 << 30)
            store = store_holder['store']
        dt, h2d = time_loader(loader_for(ds, args, store), args)
        out.update(batches_per_s=round(1.0 / dt, 2), ms_per_batch=round(dt * 1e3, 3), h2d_bytes_per_batch=int(h2d),
                   output_bytes_per_batch=args.batch * 3 * args.crop * args.crop * 4)
    elif mode == 'resident':
        dt, h2d = time_loader(resident_loader_for(ds, args, store_holder), args)
        out.update(batches_per_s=round(1.0 / dt, 2), ms_per_batch=round(dt * 1e3, 3), h2d_bytes_per_batch=int(h2d),
                   output_bytes_per_batch=args.batch * 3 * args.crop * args.crop * 4)
    else:
        torch.manual_seed(0)
        m = configs.build_model('WIDERFACE_LFD_S').cuda().train()
        opt = optim.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
        step = train.GraphedTrainStep(m, opt, dict(max_norm=10, norm_type=2), max_boxes=args.batch * 24)
        feeder = resident_loader_for(ds, args, store_holder) if mode == 'fed_resident' else loader_for(ds, args)
        it = batches(feeder, args.warmup + args.steps + 1)
        x0, ann0, _ = next(it)
        fixed_x = x0.clone()
        if mode == 'fixed':
            feed = lambda: (step.x if step.x is not None else fixed_x, ann0)     # noqa: E731
        else:
            feed = lambda: next(it)[:2]                                           # noqa: E731
        for _ in range(args.warmup):
            lv, _ = step(*feed(), True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            lv, _ = step(*feed(), True)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.steps
        out.update(ms_per_step=round(dt * 1e3, 3), images_per_s=round(args.batch / dt, 1), loss=lv['loss'])
        if mode == 'fed_resident':
            out.update(plan_status=feeder._ring[0][1].status())
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=64)
    ap.add_argument('--crop', type=int, default=480)
    ap.add_argument('--images', type=int, default=256)
    ap.add_argument('--workers', type=int, default=8)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=4)
    ap.add_argument('--modes', default='loader,loader_store,fed,fixed')
    a = ap.parse_args()
    dataset = synthetic_dataset(a.images, 0)
    holder = {}
    for md in a.modes.split(','):
        run(md, a, dataset, holder)
