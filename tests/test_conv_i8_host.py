"""Host checks of the INT8 conv's test instrument (tests/golden/conv_i8_cases.py) and of its weight packing: the oracle against
torch's conv in float64, the pack round trip, the walk maps' geometry, and the near-tie cap of the random-scale cases on the
oracle alone.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import conv_i8_cases as QC
from lfd_amd import ops


@pytest.mark.parametrize('c', [c for c in QC.small_cases() if c.cin == 64 or c.kind != 'edge'], ids=QC.case_id)
def test_oracle_matches_torch_conv_in_float64(c):
    x, w, res = QC.operands(c)
    acc = QC.acc_ref(x, w, c.stride)
    ref = F.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), stride=c.stride, padding=c.ks // 2).permute(0, 2, 3, 1)
    assert acc.shape == ref.shape == (c.n,) + QC.out_hw(c.h, c.w, c.ks, c.stride) + (c.cout,)
    assert torch.equal(acc, ref)                        # integers below 2^53: both exact
    assert float(acc.abs().max()) < 2 ** 22
    k = QC.exact_constants(c)
    v, q, f = QC.epilogue_ref(acc, k, res, relu=True)
    manual = torch.round((acc * k.mult.double() + k.biasq.double() + res.double() * 0.75).clamp(min=0)).clamp(-127, 127)
    assert torch.equal(q.double(), manual) and torch.equal(f, v * 0.125)
    # the instrument's claim: every epilogue value is exact in fp32
    assert torch.equal(v.float().double(), v)
    if c.kind != 'pixel':
        assert int(q.min()) == 0 and int(q.max()) == 127 and 0.05 < float((q == 0).double().mean()) < 0.95
        _, q2, _ = QC.epilogue_ref(acc, k, None, relu=False)
        assert int(q2.min()) == -127 and int(q2.max()) == 127      # both clamps are reached


@pytest.mark.parametrize('cin,cout,ks', [(64, 64, 3), (64, 128, 1), (128, 64, 3), (128, 128, 3)])
def test_pack_conv_weight_i8_round_trip(cin, cout, ks):
    w = QC._randint8((cout, cin, ks, ks), 5 + cin + cout + ks)          # asymmetric in every axis
    p = ops.pack_conv_weight_i8(w)
    assert p.shape == (cout // 32, ks * ks * cin // 32, 64, 16) and p.dtype == torch.int8 and p.is_contiguous()
    assert torch.equal(ops.unpack_conv_weight_i8(p, cin, ks), w)
    # the documented layout, element by element on a few entries
    for (slab, step, lane, j) in ((0, 0, 0, 0), (1, min(3, ks * ks * cin // 32 - 1), 37, 5), (cout // 32 - 1, ks * ks * cin // 32 - 1, 63, 15), (0, 1, 20, 9)):
        half, m = lane >> 5, lane & 31
        co = 32 * slab + 16 * ((m >> 2) & 1) + (m & 3) + 4 * (m >> 3)
        tap, q = divmod(step, cin // 32)
        assert int(p[slab, step, lane, j]) == int(w[co, 32 * q + 16 * half + j, tap // ks, tap % ks])
    # register g of lane half h of the 32x32 result (row (g & 3) + 8 (g >> 2) + 4 h) carries channel 16 h + g
    rows = ops._i8_rows()
    for h in (0, 1):
        for g in range(16):
            assert int(rows[(g & 3) + 8 * (g >> 2) + 4 * h]) == 16 * h + g


def test_walk_maps_give_workgroups_more_than_one_tile():
    for c in QC.walk_cases():
        tx, ty, nt, grid = QC.launch(c)
        assert (tx, ty) == (3, 2) and grid == QC.MAX_WORKGROUPS < nt <= 2 * grid
        oh, ow = QC.out_hw(c.h, c.w, c.ks, c.stride)
        assert oh == QC.tile_h(c.stride) + 1 and ow == 2 * QC.TW + 1
        two = [b for b in range(grid) if b + grid < nt]
        assert len(two) == nt - grid >= grid // 4
        # a workgroup's two tiles lie in different images at different places
        assert all((b % 6) != ((b + grid) % 6) and b // 6 != (b + grid) // 6 for b in two)
    for c in QC.small_cases():
        assert QC.launch(c)[2] <= 4 * c.n


@pytest.mark.parametrize('c', QC.random_cases(), ids=QC.case_id)
def test_near_tie_cap_holds_on_the_oracle(c):
    x, w, res = QC.operands(c)
    acc = QC.acc_ref(x, w, c.stride)
    k = QC.random_constants(c)
    for with_res in (False, True):
        for relu in (False, True):
            v, q, f = QC.epilogue_ref(acc, k, res if with_res else None, relu)
            assert float(QC.near_tie(v).double().mean()) <= QC.NEAR_TIE_CAP
            assert int(q.max()) == 127 and float(f.abs().max()) < 60000     # the range is used; fp16 does not overflow
