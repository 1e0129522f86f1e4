"""tests/golden/head_out_parent_bits.npz: the bits of dbias / dscale that the head-output glue (csrc/head_out.hip, through the
ops.head_out_* wrappers) left on the MI355X on the commit BEFORE the 64- and 128-row files became one row-width-templated
file.  tests/test_gpu_head_out_bits.py regenerates the inputs below and compares with torch.equal: the per-thread accumulation
order, the LDS sum order, the block count and the fp64 final of the gradient kernels are part of the contract (the tolerance of
the other glue tests, rtol 1e-6, would not notice a changed summation order).

Run on the GPU with the tree at the commit whose bits are to be pinned:  python tests/golden/make_golden_head_out_bits.py
(the precedent is wf_s_train_iteration_entry_points.json, also recorded on a parent commit).

Inputs come from numpy.random.default_rng on the CPU, so they do not depend on the commit or the torch version: y ~ 2 N(0,1)
cast to fp16, gradients 1e-3 N(0,1) fp32, Scale 1.37, dbias starts at 0.5, dscale at 0.25, loss scale 1024.  out and dy are not
stored: they are single roundings of fp32 products and the test compares them with the plain restatement.

Cases, n = 2, point0 = 7, P = hw + 11 (layouts: (channels, first row, with Scale and dscale)):
  hw 1; 33 (pixels x pieces is no multiple of the 256-thread block); 600 (several blocks of partials); and one hw beyond the
  block cap -- 16400 at 64 rows (32800 pixels > 1024 * 256 / 8), 8200 at 128 rows (16400 pixels > 1024 * 256 / 16) -- which
  takes the grid-stride loop into a second trip with all 1024 blocks.
One three-level case per width (hw 35, 12, 1 at point0 0, 35, 47, P = 48) through the per-level `_concat` calls and through the
one-launch `_levels` call, recorded separately."""
import os
import sys

import numpy as np

N, P0, S, SCALE = 2, 7, 1024.0, 1.37
LAYOUTS = {64: [('shipped_1+4', [(1, 0, False), (4, 1, True)]),          # no float4 group anywhere
                ('45+4', [(45, 0, False), (4, 45, True)]),
                ('60+4', [(60, 0, False), (4, 60, True)]),                # float4 groups in both segments, last row 63
                ('reg_4', [(4, 0, True)]),                                # the regression conv of separate towers
                ('single_64', [(64, 0, False)])],
           128: [('coco_80+4', [(80, 0, False), (4, 80, True)]),         # = LAYOUTS of tests/test_gpu_wide_head.py
                 ('124+4', [(124, 0, False), (4, 124, True)]),
                 ('61+4', [(61, 0, False), (4, 61, True)]),
                 ('single_128', [(128, 0, False)]),
                 ('single_4', [(4, 0, False)])]}
HWS = {64: (1, 33, 600, 16400), 128: (1, 33, 600, 8200)}
LEVEL_HWS, LEVEL_STARTS, LEVEL_P = (35, 12, 1), (0, 35, 47), 48
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'head_out_parent_bits.npz')


def single_cases():
    """-> [(rows, layout index, layout name, layout, hw)]"""
    return [(rows, li, name, layout, hw) for rows in (64, 128) for li, (name, layout) in enumerate(LAYOUTS[rows]) for hw in HWS[rows]]


def level_cases():
    """-> [(rows, layout name, layout)]: the first layout of each width (the shipped 1 + 4, COCO's 80 + 4)"""
    return [(rows,) + LAYOUTS[rows][0] for rows in (64, 128)]


def key(rows, name, what):
    return '%d/%s/%s' % (rows, name, what)


def _plain(shape, dtype, fill=None):
    import torch
    return torch.empty(shape, dtype=dtype, device='cuda') if fill is None else torch.full(shape, fill, dtype=dtype, device='cuda')


def _inputs(seed, rows, layout, ypoints, gpoints):
    """host inputs: y [N, ypoints, rows] fp16 and one gradient [N, gpoints, channels] fp32 per segment"""
    rng = np.random.default_rng(seed)
    y = (rng.standard_normal((N, ypoints, rows), dtype=np.float32) * 2).astype(np.float16)
    grads = [rng.standard_normal((N, gpoints, ch), dtype=np.float32) * np.float32(1e-3) for ch, _, _ in layout]
    return y, grads


def _segs(layout, grads, P, alloc, dscale=True):
    import torch
    segs = []
    for (ch, r0, sc), g in zip(layout, grads):
        segs.append(dict(channels=ch, row0=r0, scale=torch.tensor(SCALE, device='cuda') if sc else None,
                         out=alloc((N, P, ch), torch.float32, -7.0), dbias=alloc((ch,), torch.float32, 0.5),
                         dscale=alloc((), torch.float32, 0.25) if sc and dscale else None, grad=torch.from_numpy(g).cuda()))
    return segs


def run_single(rows, li, layout, hw, alloc=_plain):
    """one level through ops.head_out_split / ops.head_out_grad -> dict(y, segs, dy)"""
    import torch
    from lfd_amd import ops
    P = hw + 11
    yh, grads = _inputs([rows, li, hw], rows, layout, hw, P)
    y = alloc((N, 1, hw, rows), torch.float16)
    y.copy_(torch.from_numpy(yh).view(N, 1, hw, rows))
    segs = _segs(layout, grads, P, alloc)
    ops.head_out_split(y, segs, [sg['out'] for sg in segs], P0)
    dy = ops.head_out_grad(y, segs, [sg['grad'] for sg in segs], P0, S)
    torch.cuda.synchronize()
    return dict(y=y.view(N, hw, rows), segs=segs, dy=dy.view(N, hw, rows))


def run_levels(rows, layout, batched, alloc=_plain):
    """three levels of one level-concatenated conv output through the `_levels` call (batched) or the per-level `_concat` calls
    -> dict(y, segs (the shared outs / dbias / grads), dscales [level][segment], dy)"""
    import torch
    from lfd_amd import ops
    yh, grads = _inputs([rows, 99], rows, layout, LEVEL_P, LEVEL_P)
    y = alloc((N, LEVEL_P, rows), torch.float16)
    y.copy_(torch.from_numpy(yh))
    segs = _segs(layout, grads, LEVEL_P, alloc, dscale=False)
    dy = alloc((N, LEVEL_P, rows), torch.float16, 3.0)
    dscales, lv_f, lv_b = [], [], []
    for hw, p0 in zip(LEVEL_HWS, LEVEL_STARTS):
        ds = [alloc((), torch.float32, 0.25) if sg['scale'] is not None else None for sg in segs]
        lsegs = [dict(sg, dscale=d) for sg, d in zip(segs, ds)]
        dscales.append(ds)
        lv_f.append((hw, p0, lsegs, [sg['out'] for sg in segs]))
        lv_b.append((hw, p0, lsegs, [sg['grad'] for sg in segs]))
    if batched:
        ops.head_out_split_levels(y, lv_f)
        ops.head_out_grad_levels(y, lv_b, S, dy)
    else:
        for hw, p0, lsegs, o in lv_f:
            ops.head_out_split_concat(y, hw, lsegs, o, p0)
        for hw, p0, lsegs, g in lv_b:
            ops.head_out_grad_concat(y, hw, lsegs, g, p0, S, dy)
    torch.cuda.synchronize()
    return dict(y=y, segs=segs, dscales=dscales, dy=dy)


def packed(res):
    """the recorded floats of a run: every segment's dbias, then every Scale gradient (levels outermost)"""
    import torch
    ds = [d for lv in res.get('dscales', [[sg['dscale'] for sg in res['segs']]]) for d in lv if d is not None]
    return torch.cat([sg['dbias'].reshape(-1) for sg in res['segs']] + [d.reshape(1) for d in ds]).cpu().numpy()


if __name__ == '__main__':
    root = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.join(root, 'lfd-a-light-and-fast-detector_amd'))
    out = {}
    for rows, li, name, layout, hw in single_cases():
        out[key(rows, name, 'hw%d' % hw)] = packed(run_single(rows, li, layout, hw))
    for rows, name, layout in level_cases():
        out[key(rows, name, 'concat')] = packed(run_levels(rows, layout, False))
        out[key(rows, name, 'levels')] = packed(run_levels(rows, layout, True))
    assert all(np.isfinite(v).all() and v.dtype == np.float32 for v in out.values())
    dst = sys.argv[1] if len(sys.argv) > 1 else FIXTURE
    np.savez(dst, **out)
    print('wrote %s: %d cases, %d floats' % (dst, len(out), sum(v.size for v in out.values())))
