"""Training batches assembled on the GPU: crop, resize, flip, normalise (csrc/batch_assemble.hip).

The reference loader (lfd/data_pipeline/data_loader/data_loader.py) resizes every decoded image with cv2 on CPU threads, crops
it, runs albumentations' flip + Normalize to fp32 and copies the zero-padded fp32 NCHW batch to the device.  Here the host
only plans: the region samplers make the reference's `random` draws and return where to crop instead of an image, worker
threads copy the source window each crop reads into pinned memory, and one kernel launch builds the fp32 batch on the device.

    loader = DeviceDataLoader(dataset, dataset_sampler, RandomBBoxCropRegionSampler(480, (0.5, 1.5), 0.5),
                              DeviceAugmentation(flip_prob=0.5, normalize=SIMPLE_NORMALIZE), device='cuda:0')
    for image_batch, annotation_batch, meta_batch in loader:     # image_batch: device fp32 [N, 3, 480, 480]
        step(image_batch, annotation_batch)

ResidentDataset + ResidentDataLoader (below) go one step further: with the decoded images and the annotations resident in
HBM the plan itself -- draws, boxes, descriptors, tables -- is made on the device (csrc/batch_plan.hip), under the loader's own
draw contract, and the annotations arrive as DeviceAnnotations.

The resize is cv2's INTER_LINEAR for 8-bit images, the fixed-point scalar path of OpenCV 4.x resize.cpp, as a formula
(`column_coefs` / `row_coefs`); agreement with cv2 itself is not verified.
"""
import io
import math
import random
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import _lib

__all__ = ['RandomBBoxCropRegionSampler', 'IdleRegionSampler', 'RegionPlan', 'DeviceAugmentation', 'DeviceDataLoader',
           'DeviceImageStore', 'SIMPLE_NORMALIZE', 'STANDARD_NORMALIZE', 'CAFFE_IMAGENET_NORMALIZE', 'resized_size',
           'column_coefs', 'row_coefs', 'plan_tables', 'compose_host', 'pil_decode', 'assemble', 'assemble_batch',
           'stage_batch', 'ResidentDataset', 'ResidentDataLoader', 'DeviceAnnotations', 'plan_bbox_crop_batch']

# lfd/data_pipeline/dataset/sample.py:5
RESERVED_KEYS = ('image_bytes', 'image_type', 'image_path', 'image', 'bboxes', 'bbox_labels')

# lfd/data_pipeline/augmentation/augmentation_pipeline.py:17-36 (albumentations.Normalize arguments)
CAFFE_IMAGENET_NORMALIZE = dict(mean=(102.9801, 115.9465, 122.7717), std=(1.0, 1.0, 1.0), max_pixel_value=1.0)
STANDARD_NORMALIZE = dict(mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225), max_pixel_value=255.0)
SIMPLE_NORMALIZE = dict(mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), max_pixel_value=255.0)

COEF_SCALE = 2048   # INTER_RESIZE_COEF_SCALE


# ---------------------------------------------------------------------------------------------------------- resize contract
def resized_size(h, w, scale):
    """cv2.resize(image, (0, 0), fx=scale, fy=scale) output size (res_h, res_w): round half to even of w * scale, h * scale"""
    rh, rw = int(np.rint(h * float(scale))), int(np.rint(w * float(scale)))
    if rh <= 0 or rw <= 0:
        raise ValueError('resize of a %dx%d image by %r gives an empty image (cv2.resize asserts)' % (w, h, scale))
    return rh, rw


def _fractions(dst, scale):
    f = ((np.asarray(dst, dtype=np.float64) + 0.5) * (1.0 / float(scale)) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    return s, (f - s.astype(np.float32)).astype(np.float32)


def _weights(f):
    a0 = np.rint((np.float32(1.0) - f) * np.float32(COEF_SCALE)).astype(np.int32)
    a1 = np.rint(f * np.float32(COEF_SCALE)).astype(np.int32)
    return a0, a1


def column_coefs(src_w, dx, scale):
    """-> (sx0, sx1, a0, a1) for resized columns dx: the two source columns and their 11-bit weights (fraction clamped at the
    borders, as cv2 does for columns)"""
    sx, f = _fractions(dx, scale)
    lo = sx < 0
    f[lo], sx[lo] = 0, 0
    hi = sx >= src_w - 1
    f[hi], sx[hi] = 0, src_w - 1
    a0, a1 = _weights(f)
    return sx, np.minimum(sx + 1, src_w - 1), a0, a1


def row_coefs(src_h, dy, scale):
    """-> (r0, r1, b0, b1) for resized rows dy: the fraction is NOT clamped at the borders, only the row indices are"""
    sy, f = _fractions(dy, scale)
    b0, b1 = _weights(f)
    return np.clip(sy, 0, src_h - 1), np.clip(sy + 1, 0, src_h - 1), b0, b1


class RegionPlan(object):
    """What a region sampler decided for one image: resize by `scale` (to res_h x res_w), take the crop (x, y, w, h) of the
    resized image (uint8 0 outside it), and place it at the top-left of the batch slot with extent valid_w x valid_h."""
    __slots__ = ('scale', 'src_h', 'src_w', 'res_h', 'res_w', 'crop', 'valid_w', 'valid_h')

    def __init__(self, scale, src_h, src_w, crop):
        self.scale = float(scale)
        self.src_h, self.src_w = int(src_h), int(src_w)
        self.res_h, self.res_w = resized_size(src_h, src_w, scale)
        self.crop = tuple(int(v) for v in crop)
        self.valid_w, self.valid_h = self.crop[2], self.crop[3]

    @property
    def dsize(self):
        return self.res_w, self.res_h

    def __repr__(self):
        return 'RegionPlan(scale=%r, src=%dx%d, res=%dx%d, crop=%r)' % (self.scale, self.src_w, self.src_h, self.res_w,
                                                                       self.res_h, self.crop)


# ---------------------------------------------------------------------------------------------------------- region samplers
class RandomBBoxCropRegionSampler(object):
    """lfd/data_pipeline/sampler/region_sampler.py:75-144 without the pixels: the same `random` draws in the same order
    (random() for the probability, random() for the scale, choice, randint, randint) and the same box arithmetic; the sample's
    'bboxes' / 'bbox_labels' are rewritten as the reference does, and the crop is returned as a RegionPlan."""

    def __init__(self, crop_size, resize_range=(0.5, 1.5), resize_prob=1.0):
        assert isinstance(crop_size, int)
        assert isinstance(resize_range, (tuple, list))
        assert 0 <= resize_prob <= 1.
        self._crop_size = crop_size
        self._resize_range = resize_range
        self._resize_prob = resize_prob

    def __call__(self, sample, image_shape, rng=random):
        if rng.random() < self._resize_prob:
            resize_scale = rng.random() * (self._resize_range[1] - self._resize_range[0]) + self._resize_range[0]
        else:
            resize_scale = 1.0
        res_h, res_w = resized_size(image_shape[0], image_shape[1], resize_scale)

        bboxes = sample['bboxes'] if 'bboxes' in sample else []
        labels = sample['bbox_labels'] if 'bbox_labels' in sample else []
        scaled_bboxes = [[int(b[0] * resize_scale), int(b[1] * resize_scale), math.ceil(b[2] * resize_scale),
                          math.ceil(b[3] * resize_scale)] for b in bboxes]
        target_bbox = rng.choice(scaled_bboxes) if len(scaled_bboxes) > 0 else [0, 0, res_w, res_h]
        cs = self._crop_size
        w_range, h_range = cs - target_bbox[2], cs - target_bbox[3]
        crop_x = target_bbox[0] - rng.randint(min(0, w_range), max(0, w_range))
        crop_y = target_bbox[1] - rng.randint(min(0, h_range), max(0, h_range))

        new_bboxes, new_labels = [], []
        for i, b in enumerate(scaled_bboxes):
            new_x, new_y = max(0, b[0] - crop_x), max(0, b[1] - crop_y)
            new_w = min(cs, b[0] + b[2] - crop_x) - new_x - 1
            new_h = min(cs, b[1] + b[3] - crop_y) - new_y - 1
            if new_w <= 1 or new_x >= cs or new_h <= 1 or new_y >= cs:
                continue
            new_bboxes.append([new_x, new_y, new_w, new_h])
            new_labels.append(labels[i])
        if len(new_bboxes) > 0:
            sample['bboxes'], sample['bbox_labels'] = new_bboxes, new_labels
        elif 'bboxes' in sample:
            del sample['bboxes'], sample['bbox_labels']
        return RegionPlan(resize_scale, image_shape[0], image_shape[1], (crop_x, crop_y, cs, cs))


class IdleRegionSampler(object):
    """lfd/data_pipeline/sampler/region_sampler.py:261-277: the whole image at scale 1; sets the three meta keys"""

    def __call__(self, sample, image_shape, rng=random):
        sample['resize_scale'] = 1.
        sample['resized_height'] = int(image_shape[0])
        sample['resized_width'] = int(image_shape[1])
        return RegionPlan(1.0, image_shape[0], image_shape[1], (0, 0, image_shape[1], image_shape[0]))


# ---------------------------------------------------------------------------------------------------------- augmentation
class DeviceAugmentation(object):
    """The augmentation the shipped configurations use, as the batch kernel applies it: an optional horizontal flip, an
    optional BGR -> RGB channel swap and albumentations.Normalize as a 256-entry fp32 table per output channel.

    The flip is ONE rng.random() < flip_prob per sample, drawn after the region sampler's draws for that sample, and the
    boxes of a flipped sample become x' = S - x - w (S: the width of the sampler's output).  This is the loader's own rule:
    the order in which albumentations draws is version-specific and is not reproduced.  out_channels = 1 builds batches
    for gray models (the first mean / std entry; a 1-channel source only); out_channels = 3 tiles a gray source."""

    def __init__(self, flip_prob=0.0, normalize=SIMPLE_NORMALIZE, bgr2rgb=False, out_channels=3):
        if out_channels not in (1, 3):
            raise ValueError('out_channels must be 1 or 3')
        if not 0.0 <= flip_prob <= 1.0:
            raise ValueError('flip_prob must lie in [0, 1]')
        self.flip_prob, self.normalize, self.bgr2rgb, self.out_channels = float(flip_prob), normalize, bool(bgr2rgb), out_channels

    def lut(self):
        """fp32 [out_channels, 256]: albumentations' float32 arithmetic, (v - mean * max_pixel) * reciprocal(std * max_pixel)"""
        v = np.arange(256, dtype=np.float32)
        if self.normalize is None:
            return np.repeat(v[None], self.out_channels, 0)
        mean = np.array(self.normalize['mean'], dtype=np.float32)[:self.out_channels]
        std = np.array(self.normalize['std'], dtype=np.float32)[:self.out_channels]
        mp = np.float32(self.normalize.get('max_pixel_value', 255.0))
        mean = mean * mp
        recip = np.reciprocal(std * mp, dtype=np.float32)
        return ((v[None, :] - mean[:, None]) * recip[:, None]).astype(np.float32)

    def channel_map(self, c_src):
        """source channel of every output channel"""
        if self.out_channels == 1:
            if c_src != 1:
                raise ValueError('DeviceAugmentation(out_channels=1) needs 1-channel images, got %d channels' % c_src)
            return [0]
        if c_src == 1:
            return [0, 0, 0]
        return [2, 1, 0] if self.bgr2rgb else [0, 1, 2]

    def draw_flip(self, rng=random):
        return rng.random() < self.flip_prob

    @staticmethod
    def flip_boxes(bboxes, width):
        return [[width - b[0] - b[2], b[1], b[2], b[3]] for b in bboxes]


def pil_decode(data):
    """Decodes encoded image bytes with PIL into what cv2 / turbojpeg return: uint8 BGR H x W x 3, or H x W for gray.  PIL's
    JPEG decoder is not bit-identical to libjpeg-turbo's default settings, so pixels may differ from the reference's."""
    from PIL import Image
    im = Image.open(io.BytesIO(data))
    if im.mode in ('L', 'I;16', 'I', 'F'):
        return np.asarray(im.convert('L'))
    return np.ascontiguousarray(np.asarray(im.convert('RGB'))[:, :, ::-1])


# ---------------------------------------------------------------------------------------------------------- tables
def plan_tables(plan, w_out, h_out):
    """-> (coef int32 [w_out + h_out, 4], window (x0, y0, w, h)).  Columns are crop columns (before the flip); a column or row
    outside the resized image, or beyond the valid extent, has zero weights and points at the window origin."""
    cx, cy, _, _ = plan.crop
    coef = np.zeros((w_out + h_out, 4), dtype=np.int32)
    xc = np.arange(min(plan.valid_w, w_out))
    dx = cx + xc
    cin = (dx >= 0) & (dx < plan.res_w)
    yc = np.arange(min(plan.valid_h, h_out))
    dy = cy + yc
    rin = (dy >= 0) & (dy < plan.res_h)
    if cin.any() and rin.any():
        sx0, sx1, a0, a1 = column_coefs(plan.src_w, dx[cin], plan.scale)
        r0, r1, b0, b1 = row_coefs(plan.src_h, dy[rin], plan.scale)
        wx0, wx1 = int(min(sx0.min(), sx1.min())), int(max(sx0.max(), sx1.max()))
        wy0, wy1 = int(min(r0.min(), r1.min())), int(max(r0.max(), r1.max()))
        coef[:, 0:2] = np.array([wx0, wx0])
        coef[w_out:, 0:2] = np.array([wy0, wy0])
        coef[xc[cin]] = np.stack([sx0, sx1, a0, a1], 1)
        coef[w_out + yc[rin]] = np.stack([r0, r1, b0, b1], 1)
        window = (wx0, wy0, wx1 - wx0 + 1, wy1 - wy0 + 1)
    else:   # the crop misses the image: every value is uint8 0
        window = (0, 0, 1, 1)
    check_tables(coef, window, w_out, plan)
    return coef, window


def check_tables(coef, window, w_out, plan):
    """every source index of the tables lies inside the window, and the window inside the source image"""
    x0, y0, ww, wh = window
    if not (0 <= x0 and 0 <= y0 and ww >= 1 and wh >= 1 and x0 + ww <= plan.src_w and y0 + wh <= plan.src_h):
        raise RuntimeError('batch assembly: window %r outside the %dx%d source' % (window, plan.src_w, plan.src_h))
    cols, rows = coef[:w_out, :2], coef[w_out:, :2]
    if cols.size and (cols.min() < x0 or cols.max() >= x0 + ww):
        raise RuntimeError('batch assembly: a column index outside the window %r' % (window,))
    if rows.size and (rows.min() < y0 or rows.max() >= y0 + wh):
        raise RuntimeError('batch assembly: a row index outside the window %r' % (window,))


def _as_hwc(image):
    image = np.asarray(image)
    if image.dtype != np.uint8:
        raise TypeError('batch assembly takes uint8 images, got %s' % image.dtype)
    if image.ndim == 2:
        return image[:, :, None]
    if image.ndim != 3 or image.shape[2] not in (1, 3):
        raise ValueError('batch assembly takes H x W, H x W x 1 or H x W x 3 images, got %s' % (image.shape,))
    return image


def compose_host(images, plans, flips, aug, h_out, w_out):
    """The same batch built on the host the way the reference composes it: resize the whole image, crop_from_image, tile a gray
    image, flip, normalise, pad top-left with 0.0.  -> fp32 [n, C_out, h_out, w_out] (numpy)."""
    lut = aug.lut()
    out = np.zeros((len(images), aug.out_channels, h_out, w_out), dtype=np.float32)
    for i, (im, p, fl) in enumerate(zip(images, plans, flips)):
        im = _as_hwc(im).astype(np.int64)
        sx0, sx1, a0, a1 = column_coefs(p.src_w, np.arange(p.res_w), p.scale)
        r0, r1, b0, b1 = row_coefs(p.src_h, np.arange(p.res_h), p.scale)
        hr = im[:, sx0] * a0[None, :, None] + im[:, sx1] * a1[None, :, None]
        res = np.clip((hr[r0] * b0[:, None, None] + hr[r1] * b1[:, None, None] + (1 << 21)) >> 22, 0, 255)
        cx, cy, cw, ch = p.crop
        crop = np.zeros((ch, cw, im.shape[2]), dtype=np.int64)
        ys, xs = cy + np.arange(ch), cx + np.arange(cw)
        ym, xm = (ys >= 0) & (ys < p.res_h), (xs >= 0) & (xs < p.res_w)
        crop[np.ix_(ym, xm)] = res[np.ix_(ys[ym], xs[xm])]     # (crop_from_image, also where the crop misses the image)
        if fl:
            crop = crop[:, ::-1]
        cmap = aug.channel_map(im.shape[2])
        for c in range(aug.out_channels):
            out[i, c, :ch, :cw] = lut[c][crop[:, :, cmap[c]]]
    return out


# ---------------------------------------------------------------------------------------------------------- the launch
def assemble(src, desc, coef, lut, cmap, n, c_src, c_out, h_out, w_out, out):
    """lfd_batch_assemble_f32 on torch.cuda.current_stream() (all device tensors)"""
    for t in (src, desc, coef, lut, cmap, out):
        _lib.require_cuda(t, 'batch assembly')
    _lib.check(_lib.lib().lfd_batch_assemble_f32(_lib.ptr(src), _lib.ptr(desc), _lib.ptr(coef), _lib.ptr(lut), _lib.ptr(cmap),
                                                 n, c_src, c_out, h_out, w_out, _lib.ptr(out), _lib.stream_ptr()),
               'lfd_batch_assemble_f32')


def stage_batch(images, plans, flips, alloc, store=None, indices=None):
    """Lays out one batch for lfd_batch_assemble_f32 in the uint8 buffer alloc(total) returns:
    [descriptors | tables (16-byte aligned) | source windows].  With a DeviceImageStore (images None, `indices` the dataset
    indices) the descriptors point into the store's arena and no window is copied.  -> the launch parameters (dict)."""
    n = len(plans)
    h_out, w_out = max(p.valid_h for p in plans), max(p.valid_w for p in plans)
    if store is not None:
        c_src = store.channels
    else:
        c_src = 3 if any(im.shape[2] == 3 for im in images) else 1
    tables = [plan_tables(p, w_out, h_out) for p in plans]
    coef_off = DESC_BYTES * n
    coef_off += (-coef_off) % 16
    win_off = coef_off + n * (w_out + h_out) * 16
    win_bytes = [0 if store is not None else wnd[2] * wnd[3] * c_src for _, wnd in tables]
    total = win_off + int(sum(win_bytes))
    hv = alloc(total)
    desc = (_lib.BatchDesc * n)()
    o = win_off
    tb = (w_out + h_out) * 16
    for i, ((coef, (x0, y0, ww, wh)), p) in enumerate(zip(tables, plans)):
        d = desc[i]
        d.win_x0, d.win_y0, d.win_w, d.win_h = x0, y0, ww, wh
        d.valid_w, d.valid_h, d.flip = p.valid_w, p.valid_h, int(flips[i])
        hv[coef_off + i * tb:coef_off + (i + 1) * tb] = coef.view(np.uint8).reshape(-1)
        if store is not None:
            pitch = p.src_w * c_src
            d.src_offset = int(store.offsets[indices[i]]) + y0 * pitch + x0 * c_src
            d.src_pitch = pitch
        else:
            win = images[i][y0:y0 + wh, x0:x0 + ww]
            if win.shape[2] != c_src:
                win = np.repeat(win, c_src, 2)
            hv[o:o + win_bytes[i]].reshape(wh, ww, c_src)[...] = win
            d.src_offset, d.src_pitch = o - win_off, ww * c_src
            o += win_bytes[i]
    hv[:DESC_BYTES * n] = np.frombuffer(desc, dtype=np.uint8)
    return dict(n=n, h=h_out, w=w_out, c_src=c_src, total=total, coef_off=coef_off, win_off=win_off)


def launch_staged(dev, job, aug, lut, cmap, out, store=None):
    """lfd_batch_assemble_f32 over a staged batch already on the device (`dev`: the staging bytes)"""
    if job['c_src'] == 3 and aug.out_channels == 1:
        raise ValueError('DeviceAugmentation(out_channels=1) cannot take 3-channel images')
    src = dev[job['win_off']:] if store is None else store.arena
    assemble(src, dev[:job['coef_off']], dev[job['coef_off']:job['win_off']], lut, cmap, job['n'], job['c_src'],
             aug.out_channels, job['h'], job['w'], out)


def assemble_batch(images, plans, flips, aug, device, store=None, indices=None):
    """One batch, synchronously on the current stream (no pipelining): -> device fp32 [n, C_out, h, w].  images: uint8
    H x W (x C) arrays (None with a store), plans: RegionPlans, flips: bools."""
    import torch
    holder = {}

    def alloc(total):
        holder['buf'] = np.zeros(total, dtype=np.uint8)
        return holder['buf']
    ims = None if store is not None else [_as_hwc(im) for im in images]
    job = stage_batch(ims, plans, flips, alloc, store, indices)
    dev = torch.from_numpy(holder['buf']).to(device)
    lut = torch.from_numpy(np.ascontiguousarray(aug.lut().reshape(-1))).to(device)
    cmap = torch.tensor(aug.channel_map(job['c_src']), dtype=torch.int32, device=device)
    out = torch.empty(job['n'], aug.out_channels, job['h'], job['w'], dtype=torch.float32, device=device)
    launch_staged(dev, job, aug, lut, cmap, out, store)
    return out


DESC_BYTES = 48


class DeviceImageStore(object):
    """Every image of `dataset` decoded once into one device uint8 arena; batches then upload only descriptors and tables.
    Gray images are stored tiled to 3 channels when the dataset holds any colour image (the kernel reads one channel count
    per launch; the tiled image gives the same batch).  Encoded images are decoded twice while the store is built (once for
    the shapes).  Raises before allocating when the arena would exceed `max_bytes`."""

    def __init__(self, dataset, device, max_bytes, decode=None):
        import torch
        decode = decode or pil_decode
        shapes = []
        for i in range(len(dataset)):
            shapes.append(_as_hwc(_decode_sample(dataset[i], decode)).shape)
        self.channels = 3 if any(s[2] == 3 for s in shapes) else 1
        sizes = [s[0] * s[1] * self.channels for s in shapes]
        total = int(sum(sizes))
        if total > max_bytes:
            raise RuntimeError('DeviceImageStore: %d decoded bytes exceed max_bytes=%d' % (total, max_bytes))
        self.offsets = np.concatenate([[0], np.cumsum(sizes)[:-1]]).astype(np.int64) if sizes else np.zeros(0, np.int64)
        self.shapes = [(s[0], s[1]) for s in shapes]
        self.arena = torch.empty(max(total, 1), dtype=torch.uint8, device=device)
        for i in range(len(dataset)):
            im = _as_hwc(_decode_sample(dataset[i], decode))
            if im.shape[2] != self.channels:
                im = np.repeat(im, self.channels, 2)
            o = int(self.offsets[i])
            self.arena[o:o + sizes[i]].copy_(torch.from_numpy(np.ascontiguousarray(im).reshape(-1)))
        torch.cuda.synchronize(self.arena.device)
        self.nbytes = total

    def shape(self, index):
        return self.shapes[index]


def _decode_sample(sample, decode):
    """lfd/data_pipeline/data_loader/data_loader.py:47-66 with `decode` in place of turbojpeg / cv2.imdecode"""
    if 'image' in sample:
        return sample['image']
    if 'image_bytes' in sample:
        return decode(sample['image_bytes'])
    if 'image_path' in sample:
        with open(sample['image_path'], 'rb') as fin:
            return decode(fin.read())
    raise ValueError('sample does not have "image", "image_bytes" or "image_path"!')


class _Slot(object):
    """one pinned staging buffer and its device twin"""

    def __init__(self):
        self.host, self.dev = None, None
        self.copied = None       # event: the H2D copy that read `host` has completed
        self.consumed = None     # event: the kernel that read `dev` has completed


class DeviceDataLoader(object):
    """The reference DataLoader's contract (iterates (image_batch, annotation_batch, meta_batch), len() = iterations per
    epoch, .batch_size), with image_batch a device fp32 NCHW tensor built by csrc/batch_assemble.hip.

    dataset: indexable, yielding the reference's Sample dicts (decoded 'image' arrays are used as they are; 'image_bytes' /
    'image_path' go through `decode`, default `pil_decode`).  dataset_sampler: any of the reference's dataset samplers.
    region_sampler: RandomBBoxCropRegionSampler or IdleRegionSampler (this module).  augmentation: a DeviceAugmentation.

    Randomness: seed=None draws from the global `random`, like the reference (results then depend on thread timing);
    seed=int draws batch b of epoch e from random.Random('seed:e:b'), so batches do not depend on num_workers.

    Pipeline: num_workers threads plan batches and copy each image's source window into a ring of num_workers + 1 pinned
    buffers; per batch ONE host-to-device copy (descriptors, tables, windows) runs on a side stream, and the kernel, launched
    on the caller's current stream when the batch is drawn, waits for it on an event.  With a DeviceImageStore the copy
    holds descriptors and tables only.

    Lifetime: batches come from a ring of `out_buffers` device buffers (default 2), taken in draw order over the loader's
    whole life (epoch boundaries included).  The kernel writing the batch drawn two draws later is enqueued on the current
    stream when that batch is drawn, behind whatever the caller enqueued on that stream before; so a batch stays valid for
    work on the drawing stream until two more batches have been drawn (GraphedTrainStep copies it into `step.x` on that
    stream first).  Work on another stream, or a batch kept longer, needs a copy.  One epoch iterates at a time: starting a
    new iteration closes the previous one."""

    def __init__(self, dataset, dataset_sampler, region_sampler, augmentation, device, num_workers=4, seed=None, store=None,
                 decode=None, out_buffers=2):
        import torch
        if not isinstance(region_sampler, (RandomBBoxCropRegionSampler, IdleRegionSampler)):
            raise TypeError('DeviceDataLoader: RandomBBoxCropRegionSampler or IdleRegionSampler (lfd_amd.data)')
        if num_workers < 1 or out_buffers < 1:
            raise ValueError('num_workers and out_buffers must be >= 1')
        self._dataset, self._dataset_sampler = dataset, dataset_sampler
        self._region_sampler, self._aug = region_sampler, augmentation or DeviceAugmentation()
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('DeviceDataLoader builds batches on the MI355X; got device %s' % self.device)
        self._num_workers, self._seed, self._store = int(num_workers), seed, store
        self._decode = decode or pil_decode
        self._epoch = 0
        self._lut = torch.from_numpy(np.ascontiguousarray(self._aug.lut().reshape(-1))).to(self.device)
        self._maps = {}
        for c_src in (1, 3):
            try:
                self._maps[c_src] = torch.tensor(self._aug.channel_map(c_src), dtype=torch.int32, device=self.device)
            except ValueError:
                pass
        self._side = torch.cuda.Stream(device=self.device)
        self._slots = [_Slot() for _ in range(self._num_workers + 1)]
        self._out = [None] * int(out_buffers)
        self._drawn = 0          # batches drawn over the loader's life: picks the output buffer
        self._active = None      # the epoch being iterated
        self.last_h2d_bytes = 0

    def __len__(self):
        return len(self._dataset_sampler)

    @property
    def batch_size(self):
        return self._dataset_sampler.get_batch_size()

    # ---------------------------------------------------------------- planning (worker threads)
    def _rng(self, epoch, batch_index):
        return random if self._seed is None else random.Random('%d:%d:%d' % (self._seed, epoch, batch_index))

    def plan(self, index_batch, rng, store=None):
        """-> (images, plans, flips, annotations, metas); images are decoded arrays, or None when `store` (a
        DeviceImageStore) gives the shapes"""
        images, plans, flips, annotations, metas = [], [], [], [], []
        for idx in index_batch:
            sample = self._dataset[idx]
            st = {}
            if 'bboxes' in sample:
                st['bboxes'], st['bbox_labels'] = sample['bboxes'], sample['bbox_labels']
            for k in set(sample.keys()) - set(RESERVED_KEYS):
                st[k] = sample[k]
            if store is not None:
                image, shape = None, store.shape(idx)
            else:
                image = _as_hwc(_decode_sample(sample, self._decode))
                shape = image.shape
            p = self._region_sampler(st, shape, rng)
            fl = self._aug.draw_flip(rng)
            if fl and 'bboxes' in st:
                st['bboxes'] = DeviceAugmentation.flip_boxes(st['bboxes'], p.valid_w)
            images.append(image)
            plans.append(p)
            flips.append(fl)
            if 'bboxes' in st:
                annotations.append((np.array(st['bboxes'], dtype=np.float32).reshape(-1, 4),
                                    np.array(st['bbox_labels'], dtype=np.int64)))
            else:
                annotations.append((np.empty((0, 4), dtype=np.float32), np.empty((0,), dtype=np.int64)))
            meta_keys = set(st.keys()) - set(RESERVED_KEYS)
            metas.append({k: st[k] for k in meta_keys} if meta_keys else None)
        return images, plans, flips, annotations, metas

    def _stage(self, slot, index_batch, rng):
        """plan a batch and fill the slot's pinned buffer (stage_batch)"""
        import torch
        images, plans, flips, annotations, metas = self.plan(index_batch, rng, self._store)

        def alloc(total):
            if slot.copied is not None:
                slot.copied.synchronize()       # the previous copy out of this buffer has completed
            if slot.host is None or slot.host.numel() < total:
                slot.host = torch.empty(int(total * 1.25) + 4096, dtype=torch.uint8).pin_memory()
            return slot.host.numpy()
        job = stage_batch(images, plans, flips, alloc, self._store, index_batch)
        job.update(annotations=annotations, metas=metas)
        return job

    # ---------------------------------------------------------------- launch (drawing thread)
    def _launch(self, slot, job):
        import torch
        cur = torch.cuda.current_stream(self.device)
        total = job['total']
        if slot.dev is None or slot.dev.numel() < total:
            torch.cuda.synchronize(self.device)         # (rare) the old buffer may still be read
            slot.dev = torch.empty(slot.host.numel(), dtype=torch.uint8, device=self.device)
        with torch.cuda.stream(self._side):
            if slot.consumed is not None:
                self._side.wait_event(slot.consumed)
            slot.dev[:total].copy_(slot.host[:total], non_blocking=True)
            slot.copied = torch.cuda.Event()
            slot.copied.record(self._side)
        cur.wait_event(slot.copied)
        n, h, w, c_out = job['n'], job['h'], job['w'], self._aug.out_channels
        k = self._drawn % len(self._out)
        numel = n * c_out * h * w
        if self._out[k] is None or self._out[k].numel() < numel:
            self._out[k] = torch.empty(numel, dtype=torch.float32, device=self.device)
        out = self._out[k][:numel].view(n, c_out, h, w)
        if job['c_src'] not in self._maps:
            raise ValueError('DeviceAugmentation(out_channels=%d) cannot take %d-channel images' % (c_out, job['c_src']))
        launch_staged(slot.dev, job, self._aug, self._lut, self._maps[job['c_src']], out, self._store)
        slot.consumed = torch.cuda.Event()
        slot.consumed.record(cur)
        self.last_h2d_bytes = total
        self._drawn += 1
        return out

    def __iter__(self):
        if self._active is not None:
            self._active.close()            # its workers finish before this epoch's use the staging buffers
        self._active = self._epoch_batches(self._epoch)
        self._epoch += 1
        return self._active

    def _epoch_batches(self, epoch):
        batches = list(self._dataset_sampler)
        depth = len(self._slots) - 1        # batch b + depth reuses the slot of batch b - 1, whose copy is issued
        pool = ThreadPoolExecutor(max_workers=self._num_workers)
        futures = {}
        try:
            for b in range(min(depth, len(batches))):
                futures[b] = pool.submit(self._stage, self._slots[b % len(self._slots)], batches[b], self._rng(epoch, b))
            for b in range(len(batches)):
                job = futures.pop(b).result()
                out = self._launch(self._slots[b % len(self._slots)], job)
                nb = b + depth
                if nb < len(batches):
                    futures[nb] = pool.submit(self._stage, self._slots[nb % len(self._slots)], batches[nb],
                                              self._rng(epoch, nb))
                yield out, job['annotations'], job['metas']
        finally:
            for f in futures.values():
                f.cancel()
            pool.shutdown(wait=True)

    def host_batch(self, index_batch, epoch, batch_index):
        """the batch the seeded loader draws for (epoch, batch_index), composed on the host (compose_host): -> (fp32 NCHW numpy,
        annotations, metas).  Needs seed=int; decodes the dataset's images (also when the loader reads a store)."""
        if self._seed is None:
            raise RuntimeError('host_batch needs a seeded loader')
        images, plans, flips, annotations, metas = self.plan(index_batch, self._rng(epoch, batch_index))
        h, w = max(p.valid_h for p in plans), max(p.valid_w for p in plans)
        return compose_host(images, plans, flips, self._aug, h, w), annotations, metas


# ---------------------------------------------------------------------------------------------------------- resident loader
class ResidentDataset(object):
    """A DeviceImageStore plus the dataset's annotations as device tables, so that a whole batch can be planned by
    csrc/batch_plan.hip: img_offset int64 [M], img_h / img_w int32 [M], box float64 [sumB, 4] (the samples' 'bboxes' x, y, w, h,
    exactly the Python floats), label int64 [sumB], box_offset int32 [M + 1].  Samples without 'bboxes' own no boxes.  The
    non-reserved sample keys (the metas) stay on the host: `metas[index]` is a dict, or None."""

    def __init__(self, dataset, device, max_bytes, decode=None):
        import torch
        self.store = DeviceImageStore(dataset, device, max_bytes, decode)
        self.device = self.store.arena.device
        boxes, labels, offs, self.metas = [], [], [0], []
        for i in range(len(dataset)):
            sample = dataset[i]
            if 'bboxes' in sample:
                b = [[float(v) for v in row[:4]] for row in sample['bboxes']]
                l = [int(v) for v in sample['bbox_labels']]
                if len(b) != len(l):
                    raise ValueError('sample %d: %d bboxes, %d bbox_labels' % (i, len(b), len(l)))
                boxes += b
                labels += l
            offs.append(len(boxes))
            keys = set(sample.keys()) - set(RESERVED_KEYS)
            self.metas.append({k: sample[k] for k in keys} if keys else None)
        if offs[-1] >= 1 << 31:
            raise RuntimeError('ResidentDataset: %d boxes do not fit int32 offsets' % offs[-1])
        self.num_images, self.num_boxes = len(self.metas), offs[-1]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.device)     # noqa: E731
        self.img_offset = up(np.asarray(self.store.offsets, dtype=np.int64).reshape(-1))
        self.img_h = up(np.array([s[0] for s in self.store.shapes], dtype=np.int32))
        self.img_w = up(np.array([s[1] for s in self.store.shapes], dtype=np.int32))
        self.box = up(np.array(boxes, dtype=np.float64).reshape(-1, 4) if boxes else np.zeros((1, 4), np.float64))
        self.label = up(np.array(labels, dtype=np.int64) if labels else np.zeros((1,), np.int64))
        self.box_offset = up(np.array(offs, dtype=np.int32))
        torch.cuda.synchronize(self.device)

    def __len__(self):
        return self.num_images

    @property
    def channels(self):
        return self.store.channels


class DeviceAnnotations(object):
    """One batch's annotations on the device, in GraphedTrainStep's single-buffer layout:
    `buffer` uint8 = [boxes f32 [max_boxes, 4] | labels i64 [max_boxes] | offsets i32 [n + 1]], with the three views.  Image i
    owns boxes offsets[i] .. offsets[i + 1] (x, y, w, h); rows beyond offsets[n] are unspecified.  len() is the batch size.
    Lives as long as the image batch it was drawn with (the loader's ring)."""

    def __init__(self, n, max_boxes, device):
        import torch
        self.n, self.max_boxes = int(n), int(max_boxes)
        mb = self.max_boxes
        self.buffer = torch.zeros(24 * mb + 4 * (self.n + 1), dtype=torch.uint8, device=device)
        self.boxes = self.buffer[:16 * mb].view(torch.float32).view(mb, 4)
        self.labels = self.buffer[16 * mb:24 * mb].view(torch.int64)
        self.offsets = self.buffer[24 * mb:].view(torch.int32)
        self.status_words = torch.zeros(4, dtype=torch.int32, device=device)

    def __len__(self):
        return self.n

    def to_host(self):
        """-> the reference's annotation_batch: a list of (float32 [g, 4], int64 [g]) per image (copies; synchronises)"""
        offs = self.offsets.cpu().numpy()
        k = int(offs[-1])
        boxes, labels = self.boxes[:k].cpu().numpy(), self.labels[:k].cpu().numpy()
        return [(boxes[offs[i]:offs[i + 1]].copy(), labels[offs[i]:offs[i + 1]].copy()) for i in range(self.n)]

    def status(self):
        """-> dict(bits, dropped_per_image, dropped_batch, blank_images): what the planning kernel could not keep (synchronises).
        bits: 1 a resize to an empty image, 2 / 4 boxes beyond max_boxes_per_image / max_boxes, 8 a sample out of range."""
        w = [int(v) for v in self.status_words.cpu().numpy()]
        return dict(bits=w[0], dropped_per_image=w[1], dropped_batch=w[2], blank_images=w[3])


class PlanBuffers(object):
    """what lfd_plan_bbox_crop_batch writes for lfd_batch_assemble_f32 and its per-sample staging (one ring slot)"""

    def __init__(self, n, crop_size, max_boxes_per_image, device):
        import torch
        self.n, self.crop_size, self.max_boxes_per_image = int(n), int(crop_size), int(max_boxes_per_image)
        self.desc = torch.zeros(DESC_BYTES * self.n, dtype=torch.uint8, device=device)
        self.coef = torch.zeros((self.n, 2 * self.crop_size, 4), dtype=torch.int32, device=device)
        self.stage_box = torch.zeros((self.n, self.max_boxes_per_image, 4), dtype=torch.float32, device=device)
        self.stage_label = torch.zeros((self.n, self.max_boxes_per_image), dtype=torch.int64, device=device)
        self.stage_count = torch.zeros((self.n, 4), dtype=torch.int32, device=device)

    def desc_host(self):
        """-> the descriptors as a list of lfd_amd._lib.BatchDesc (copies; synchronises)"""
        raw = self.desc.cpu().numpy().tobytes()
        return [_lib.BatchDesc.from_buffer_copy(raw, i * DESC_BYTES) for i in range(self.n)]


def plan_bbox_crop_batch(rds, indices, seed, epoch, batch, crop_size, resize_range, resize_prob, flip_prob, plan, ann,
                         max_boxes_per_image=None):
    """lfd_plan_bbox_crop_batch on torch.cuda.current_stream(): plans the batch whose dataset indices are the device int32 row
    `indices` over the ResidentDataset `rds` into `plan` (PlanBuffers) and `ann` (DeviceAnnotations)."""
    import ctypes as C
    n = int(indices.numel())
    mbpi = plan.max_boxes_per_image if max_boxes_per_image is None else int(max_boxes_per_image)
    if n != plan.n or n != ann.n or crop_size != plan.crop_size or not 1 <= mbpi <= plan.max_boxes_per_image:
        raise ValueError('plan_bbox_crop_batch: buffers for another batch size, crop size or capacity')
    if indices.dtype != _torch().int32 or not indices.is_contiguous():
        raise TypeError('plan_bbox_crop_batch: indices must be a contiguous int32 row')
    if not 0 <= int(seed) < 1 << 64 or not 0 <= int(epoch) < 1 << 32 or not 0 <= int(batch) < 1 << 32:
        raise ValueError('plan_bbox_crop_batch: seed in [0, 2^64), epoch and batch in [0, 2^32)')
    for t in (indices, plan.desc, ann.buffer, rds.box):
        _lib.require_cuda(t, 'batch planning')
    d = _lib.PlanDesc()
    d.seed, d.epoch, d.batch = int(seed), int(epoch), int(batch)
    d.resize_lo, d.resize_hi = float(resize_range[0]), float(resize_range[1])
    d.resize_prob, d.flip_prob = float(resize_prob), float(flip_prob)
    d.arena_bytes = int(rds.store.nbytes)
    d.n, d.num_images, d.total_boxes = n, rds.num_images, rds.num_boxes
    d.crop_size, d.c_src = int(crop_size), rds.channels
    d.max_boxes_per_image, d.max_boxes = mbpi, ann.max_boxes
    b = _lib.PlanBufs()
    for k, t in (('img_offset', rds.img_offset), ('img_h', rds.img_h), ('img_w', rds.img_w), ('box', rds.box),
                 ('label', rds.label), ('box_offset', rds.box_offset), ('indices', indices), ('desc', plan.desc),
                 ('coef', plan.coef), ('stage_box', plan.stage_box), ('stage_label', plan.stage_label),
                 ('stage_count', plan.stage_count), ('boxes', ann.boxes), ('labels', ann.labels), ('offsets', ann.offsets),
                 ('status', ann.status_words)):
        setattr(b, k, t.data_ptr())
    _lib.check(_lib.lib().lfd_plan_bbox_crop_batch(C.byref(d), C.byref(b), _lib.stream_ptr()), 'lfd_plan_bbox_crop_batch')


def _torch():
    import torch
    return torch


class ResidentDataLoader(object):
    """DeviceDataLoader's contract over a ResidentDataset, with the whole per-batch plan made on the device
    (csrc/batch_plan.hip): per batch the host launches lfd_plan_bbox_crop_batch and lfd_batch_assemble_f32 on the caller's
    current stream, copies nothing (`last_h2d_bytes` is 0) and runs no worker threads.  Once per epoch `list(dataset_sampler)`
    is uploaded as int32 [iterations, N].

    Yields (image_batch, annotation_batch, meta_batch): image_batch fp32 [N, C_out, crop, crop] on the device,
    annotation_batch a DeviceAnnotations (GraphedTrainStep, train_step and LFD.get_loss take it as it is; `.to_host()` gives
    the reference's list), meta_batch the host list of the samples' metas.

    region_sampler: this module's RandomBBoxCropRegionSampler, read for crop_size, resize_range and resize_prob only.  The
    draws are NOT the reference's Mersenne Twister stream but the loader's own contract: Philox4x32-10 keyed by
    `seed`, counter (slot, batch, epoch, j), words at fixed positions; batch (epoch, b) depends on nothing else.  Validation
    batches (IdleRegionSampler) stay with DeviceDataLoader.

    Lifetime: as DeviceDataLoader's -- image batches, annotations and `last_plan` come from rings of `out_buffers` slots taken in
    draw order; a batch stays valid for work on the drawing stream until `out_buffers` more batches have been drawn."""

    def __init__(self, resident_dataset, dataset_sampler, region_sampler, augmentation, seed, max_boxes=4096,
                 max_boxes_per_image=None, out_buffers=2):
        import torch
        if not isinstance(region_sampler, RandomBBoxCropRegionSampler):
            raise TypeError('ResidentDataLoader plans RandomBBoxCropRegionSampler (lfd_amd.data) on the device; '
                            'other region samplers, IdleRegionSampler included, go through DeviceDataLoader')
        if not isinstance(resident_dataset, ResidentDataset):
            raise TypeError('ResidentDataLoader: a ResidentDataset (lfd_amd.data)')
        if seed is None or not 0 <= int(seed) < 1 << 64:
            raise ValueError('ResidentDataLoader: seed must be an int in [0, 2^64)')
        if out_buffers < 1 or max_boxes < 1 or (max_boxes_per_image is not None and max_boxes_per_image < 1):
            raise ValueError('out_buffers, max_boxes and max_boxes_per_image must be >= 1')
        self._rds, self._dataset_sampler = resident_dataset, dataset_sampler
        self._aug = augmentation or DeviceAugmentation()
        self._crop = int(region_sampler._crop_size)
        self._resize_range = (float(region_sampler._resize_range[0]), float(region_sampler._resize_range[1]))
        self._resize_prob = float(region_sampler._resize_prob)
        self._seed = int(seed)
        self.max_boxes = int(max_boxes)
        self.max_boxes_per_image = int(max_boxes if max_boxes_per_image is None else max_boxes_per_image)
        self.device = resident_dataset.device
        self._lut = torch.from_numpy(np.ascontiguousarray(self._aug.lut().reshape(-1))).to(self.device)
        self._map = torch.tensor(self._aug.channel_map(resident_dataset.channels), dtype=torch.int32, device=self.device)
        self._out = [None] * int(out_buffers)
        self._ring = [None] * int(out_buffers)      # (PlanBuffers, DeviceAnnotations) per slot
        self._drawn, self._epoch, self._active = 0, 0, None
        self.last_h2d_bytes = 0
        self.last_plan = None

    def __len__(self):
        return len(self._dataset_sampler)

    @property
    def batch_size(self):
        return self._dataset_sampler.get_batch_size()

    def draw(self, indices, epoch, batch_index):
        """plans and assembles the batch (epoch, batch_index) over the device int32 row `indices` into the next ring slot:
        -> (image_batch, DeviceAnnotations)"""
        import torch
        n, cs, c_out = int(indices.numel()), self._crop, self._aug.out_channels
        k = self._drawn % len(self._out)
        if self._ring[k] is None or self._ring[k][0].n != n:
            self._ring[k] = (PlanBuffers(n, cs, self.max_boxes_per_image, self.device),
                             DeviceAnnotations(n, self.max_boxes, self.device))
            self._out[k] = torch.empty(n * c_out * cs * cs, dtype=torch.float32, device=self.device)
        plan, ann = self._ring[k]
        out = self._out[k].view(n, c_out, cs, cs)
        with torch.cuda.device(self.device):
            plan_bbox_crop_batch(self._rds, indices, self._seed, epoch, batch_index, cs, self._resize_range, self._resize_prob,
                                 self._aug.flip_prob, plan, ann)
            assemble(self._rds.store.arena, plan.desc, plan.coef, self._lut, self._map, n, self._rds.channels, c_out, cs, cs, out)
        self._drawn += 1
        self.last_plan, self.last_h2d_bytes = plan, 0
        return out, ann

    def __iter__(self):
        if self._active is not None:
            self._active.close()
        self._active = self._epoch_batches(self._epoch)
        self._epoch += 1
        return self._active

    def _epoch_batches(self, epoch):
        import torch
        rows = [list(map(int, r)) for r in self._dataset_sampler]
        if not rows:
            return
        if any(len(r) != len(rows[0]) for r in rows):
            raise ValueError('ResidentDataLoader: every batch of an epoch must have the same size')
        table = torch.from_numpy(np.array(rows, dtype=np.int32)).to(self.device)      # the epoch's one upload
        metas = self._rds.metas
        for b, row in enumerate(rows):
            out, ann = self.draw(table[b], epoch, b)
            yield out, ann, [metas[i] for i in row]
