"""The batch-assembly contract restated in plain numpy, one resized column / row at a time, for tests/test_data_host.py and
tests/test_gpu_data.py (independent of lfd_amd.data's vectorised tables).

cv2.resize(image, (0, 0), fx=s, fy=s, INTER_LINEAR) on uint8, OpenCV 4.x fixed-point scalar path:
  res = rint_half_even(W * s) x rint_half_even(H * s);
  column dx: f = float32((dx + 0.5) * (1 / s) - 0.5), sx = floor(f), f -= sx; sx < 0 -> (sx, f) = (0, 0);
             sx >= W - 1 -> (sx, f) = (W - 1, 0); a0 = rint(float32(1 - f) * 2048), a1 = rint(f * 2048);
             Hrow[dx] = S[sx] * a0 + S[min(sx + 1, W - 1)] * a1;
  row dy:    the same f, sy, b0, b1 with the fraction NOT clamped; rows clip(sy, 0, H - 1), clip(sy + 1, 0, H - 1);
  v = clamp((Hrow_r0 * b0 + Hrow_r1 * b1 + 2^21) >> 22, 0, 255).
Then crop (uint8 0 outside the resized image), gray -> 3 channels by tiling, horizontal flip, out = lut[c][v] per output
channel (channel map), and 0.0 beyond the image's extent in the batch.
"""
import math

import numpy as np


def rint(x):
    return int(np.rint(x))


def taps(n_src, d, s, clamp_fraction):
    f = np.float32((d + 0.5) * (1.0 / s) - 0.5)
    i = int(math.floor(f))
    f = np.float32(f - np.float32(i))
    if clamp_fraction:
        if i < 0:
            f, i = np.float32(0), 0
        if i >= n_src - 1:
            f, i = np.float32(0), n_src - 1
        i0, i1 = i, min(i + 1, n_src - 1)
    else:
        i0, i1 = min(max(i, 0), n_src - 1), min(max(i + 1, 0), n_src - 1)
    w0 = rint(np.float32(np.float32(1.0) - f) * np.float32(2048))
    w1 = rint(np.float32(f * np.float32(2048)))
    return i0, i1, w0, w1


def resize(image, s):
    """uint8 H x W x C -> uint8 res_h x res_w x C; also returns the set of source columns / rows read"""
    h, w = image.shape[:2]
    rh, rw = rint(h * s), rint(w * s)
    if rh <= 0 or rw <= 0:
        raise ValueError('empty resize')
    src = image.astype(np.int64)
    hrow = np.zeros((h, rw, image.shape[2]), dtype=np.int64)
    for dx in range(rw):
        x0, x1, a0, a1 = taps(w, dx, s, True)
        hrow[:, dx] = src[:, x0] * a0 + src[:, x1] * a1
    out = np.zeros((rh, rw, image.shape[2]), dtype=np.uint8)
    for dy in range(rh):
        y0, y1, b0, b1 = taps(h, dy, s, False)
        out[dy] = np.clip((hrow[y0] * b0 + hrow[y1] * b1 + (1 << 21)) >> 22, 0, 255)
    return out


def touched(h, w, s, crop):
    """-> (columns, rows) of the source that the crop's pixels read"""
    cx, cy, cw, ch = crop
    rh, rw = rint(h * s), rint(w * s)
    cols, rows = set(), set()
    for dx in range(max(cx, 0), min(cx + cw, rw)):
        cols.update(taps(w, dx, s, True)[:2])
    for dy in range(max(cy, 0), min(cy + ch, rh)):
        rows.update(taps(h, dy, s, False)[:2])
    if not cols or not rows:      # the crop misses the resized image: no pixel is read
        return set(), set()
    return cols, rows


def compose(images, scales, crops, flips, lut, cmap_rgb, out_channels, h_out, w_out):
    """images: uint8 H x W x C (C 1 or 3); crops (x, y, w, h) of the resized image (w, h = the image's extent in the batch);
    lut: fp32 [out_channels, 256]; cmap_rgb: channel map for 3-channel sources -> fp32 [n, out_channels, h_out, w_out]"""
    out = np.zeros((len(images), out_channels, h_out, w_out), dtype=np.float32)
    for i, (im, s, (cx, cy, cw, ch), fl) in enumerate(zip(images, scales, crops, flips)):
        if im.ndim == 2:
            im = im[:, :, None]
        res = resize(im, s)
        rh, rw = res.shape[:2]
        crop = np.zeros((ch, cw, im.shape[2]), dtype=np.uint8)
        ys, xs = cy + np.arange(ch), cx + np.arange(cw)
        ym, xm = (ys >= 0) & (ys < rh), (xs >= 0) & (xs < rw)
        crop[np.ix_(ym, xm)] = res[np.ix_(ys[ym], xs[xm])]
        if crop.shape[2] == 1 and out_channels == 3:
            crop = np.repeat(crop, 3, 2)
            cmap = [0, 1, 2]
        else:
            cmap = cmap_rgb if crop.shape[2] == 3 else [0]
        if fl:
            crop = crop[:, ::-1]
        for c in range(out_channels):
            out[i, c, :ch, :cw] = lut[c][crop[:, :, cmap[c]]]
    return out
