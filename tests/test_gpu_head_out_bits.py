"""csrc/head_out.hip, one row-width-templated file for 64 and 128 output rows, leaves the BITS the two files before it left:
dbias and dscale of every case of tests/golden/make_golden_head_out_bits.py (recorded on the MI355X on the commit before the
files became one, tests/golden/head_out_parent_bits.npz) are compared with torch.equal -- a changed accumulation order, LDS sum
order, block count or final stage would show, which the rtol 1e-6 of the other glue tests would not.  out and dy are single
roundings of fp32 products and are compared with the plain restatement (float(y) * scale, half(grad * scale * loss scale), zero
outside the segments), also with torch.equal.

Every tensor the kernels write -- out, dy, dbias, dscale, the workspace -- and y sit between 256 guard bytes of 0xA5 (the _guarded
pattern of tests/test_gpu_wide_head.py).  The calls go through the ops.head_out_* wrappers, as the recording did; the workspace
(ops.train_workspace) and the dy that ops.head_out_grad allocates are replaced with guarded ones of exactly the size the
library asks for: 1024 blocks x 2 x rows floats per level.

The hw beyond the block cap (16400 at 64 rows, 8200 at 128) takes the grid-stride loops into a second trip with all 1024 blocks,
which no other test reaches: a wrong stride or piece index would show there."""
import numpy as np
import pytest
import torch

import make_golden_head_out_bits as G
from conftest import load_golden
from lfd_amd import ops

pytestmark = pytest.mark.gpu

GUARD = 256


@pytest.fixture(scope='module')
def parent_bits():
    return load_golden('head_out_parent_bits.npz')


class _Guarded(object):
    """allocator of the golden module's runs: every tensor between two runs of GUARD bytes of 0xA5"""

    def __init__(self):
        self.made = []

    def __call__(self, shape, dtype, fill=None):
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        whole = torch.full((nbytes + -nbytes % 16 + 2 * GUARD,), 0xA5, dtype=torch.uint8, device='cuda')
        t = whole[GUARD:GUARD + nbytes].view(dtype).view(shape)
        if fill is not None:
            t.fill_(fill)
        self.made.append((whole, nbytes))
        return t

    def owns(self, t):
        return any(t.data_ptr() == w.data_ptr() + GUARD for w, _ in self.made)

    def intact(self):
        return all(bool((w[:GUARD] == 0xA5).all()) and bool((w[GUARD + b:] == 0xA5).all()) for w, b in self.made)


def _guard_the_wrappers_buffers(monkeypatch, alloc, rows, nlevels, guard_dy=False):
    """the workspace of exactly nlevels x 1024 x 2 x rows floats, and (per-level form) the dy ops.head_out_grad allocates with
    torch.empty_like(y): only for the guarded y of this run, every other empty_like is torch's"""
    ws = alloc((nlevels * 1024 * 2 * rows * 4,), torch.uint8)
    monkeypatch.setattr(ops, 'train_workspace', lambda device: ws)
    if guard_dy:
        real = torch.empty_like
        monkeypatch.setattr(torch, 'empty_like', lambda t, *a, **k: alloc(t.shape, t.dtype, 3.0) if t.dtype == torch.float16 and
                            alloc.owns(t) else real(t, *a, **k))


def _check_restatement(y, segs, dy, points):
    """out / dy of the points [lo, hi) that the call covered against the plain torch ops, and nothing written elsewhere"""
    lo, hi = points
    ref_dy = torch.zeros_like(dy)
    for sg in segs:
        rows = slice(sg['row0'], sg['row0'] + sg['channels'])
        ref, d = y[..., rows].float(), sg['grad'][:, lo:hi]
        if sg['scale'] is not None:
            ref, d = ref * sg['scale'], d * sg['scale']
        assert torch.equal(sg['out'][:, lo:hi], ref)
        assert bool((sg['out'][:, :lo] == -7).all()) and bool((sg['out'][:, hi:] == -7).all())
        ref_dy[..., rows] = (d * G.S).half()
    assert torch.equal(dy, ref_dy)


CASES = G.single_cases()


@pytest.mark.parametrize('rows,li,name,layout,hw', CASES, ids=['%d-%s-hw%d' % (c[0], c[2], c[4]) for c in CASES])
def test_one_level_leaves_the_parents_bits(rows, li, name, layout, hw, parent_bits, monkeypatch):
    alloc = _Guarded()
    _guard_the_wrappers_buffers(monkeypatch, alloc, rows, 1, guard_dy=True)
    res = G.run_single(rows, li, layout, hw, alloc)
    monkeypatch.undo()
    got, want = G.packed(res), parent_bits[G.key(rows, name, 'hw%d' % hw)]
    print(rows, name, hw, 'floats that differ from the recorded ones: %d of %d, max abs difference %.3g'
          % (int((got != want).sum()), got.size, float(np.abs(got.astype(np.float64) - want).max())))
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    assert torch.equal(torch.from_numpy(got), torch.from_numpy(want))
    assert not np.any(got[:sum(ch for ch, _, _ in layout)] == 0.5)          # every bias gradient accumulated
    _check_restatement(res['y'], res['segs'], res['dy'], (G.P0, G.P0 + hw))
    assert alloc.intact()


@pytest.mark.parametrize('rows,name,layout', G.level_cases(), ids=['%d-%s' % c[:2] for c in G.level_cases()])
def test_three_levels_leave_the_parents_bits_in_both_call_forms(rows, name, layout, parent_bits, monkeypatch):
    got = {}
    for form, batched in (('concat', False), ('levels', True)):
        alloc = _Guarded()
        _guard_the_wrappers_buffers(monkeypatch, alloc, rows, len(G.LEVEL_HWS) if batched else 1)
        res = G.run_levels(rows, layout, batched, alloc)
        monkeypatch.undo()
        got[form], want = G.packed(res), parent_bits[G.key(rows, name, form)]
        print(rows, name, form, 'floats that differ from the recorded ones: %d of %d' % (int((got[form] != want).sum()), want.size))
        assert torch.equal(torch.from_numpy(got[form]), torch.from_numpy(want))
        _check_restatement(res['y'], res['segs'], res['dy'], (0, G.LEVEL_P))
        assert alloc.intact()
    assert torch.equal(torch.from_numpy(got['concat']), torch.from_numpy(got['levels']))      # as today: one launch = the loop
