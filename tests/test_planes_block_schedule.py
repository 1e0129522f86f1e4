"""The step schedule of k_pl_blk64 (csrc/planes_block.hip: a 64-channel residual block of the planes mode as one row stream)
restated in Python and checked exhaustively.  With ONE workgroup barrier per step it is only correct if
  (a) every input row conv1 or the identity reads in step j has landed (the DMA waves wait for all but the two newest rows
      they issued before the barrier) and its ring slot was not re-targeted since;
  (b) every mid row conv2 reads in step j was written in a step < j and not overwritten since; no slot is written in a step
      in which it is read;
for segments that start at row 0, end at H, sit in the middle, and are shorter than the rings.
CPU test: pure arithmetic, the same formulas as the kernel (PB::NIN, NMID, LEAD; conv1 row j, conv2 row j - 4; T = R + 5)."""
import pytest

NIN, NMID, LEAD = 8, 4, 5


def schedule(R):
    """per step j: (input rows DMA'd at the end of j, input rows read, mid rows written, mid rows read)"""
    T = R + 5
    steps = []
    for j in range(T):
        dma = [j + LEAD]
        rin, wmid, rmid = [], [], []
        if 0 <= j < R + 2:                       # conv1 contracts mid row j from input rows j .. j + 2
            rin += [j, j + 1, j + 2]
        if 0 <= j - 1 < R + 2:                   # conv1 B finishes mid row j - 1
            wmid.append(j - 1)
        ol = j - 4
        if 0 <= ol < R:                          # conv2 contracts output row ol from mid rows ol .. ol + 2, identity input row ol + 2
            rmid += [ol, ol + 1, ol + 2]
            rin.append(ol + 2)
        steps.append((dma, rin, wmid, rmid))
    return steps


@pytest.mark.parametrize('R', list(range(1, 40)))
def test_rings_are_safe(R):
    issued = {il: -1 for il in range(LEAD)}      # prologue: rows 0 .. LEAD - 1 before step 0
    in_slot = {il % NIN: il for il in range(LEAD)}
    mid_written, mid_slot = {}, {}
    for j, (dma, rin, wmid, rmid) in enumerate(schedule(R)):
        for il in rin:
            assert il in issued, (R, j, il)
            # landed: the DMA waves' vmcnt leaves only the two newest rows issued so far in flight
            assert il <= max(issued) - 2, (R, j, il, max(issued))
            assert in_slot[il % NIN] == il, ('input row overwritten', R, j, il)
        slots_read = {m % NMID for m in rmid}
        for m in rmid:
            assert m in mid_written and mid_written[m] < j, ('mid row not ready', R, j, m)
            assert mid_slot[m % NMID] == m, ('mid row overwritten', R, j, m)
        for m in wmid:
            assert m % NMID not in slots_read, ('mid slot written while read', R, j, m)
            mid_written[m] = j
            mid_slot[m % NMID] = m
        for il in dma:
            # the slot's previous row must have no read in this step or later
            old = in_slot.get(il % NIN)
            if old is not None:
                assert all(old not in s[1] for s in schedule(R)[j:]), ('slot re-targeted too early', R, j, il, old)
            issued[il] = j
            in_slot[il % NIN] = il


@pytest.mark.parametrize('H,SH', [(135, 34), (68, 9), (34, 4), (3, 4), (1, 4), (7, 4)])
def test_segments_cover_every_row_once(H, SH):
    """segment s covers output rows [s SH, min(H, (s + 1) SH)); every row of the map exactly once"""
    SH = min(SH, H)
    segs = -(-H // SH)
    rows = [s * SH + r for s in range(segs) for r in range(min(SH, H - s * SH))]
    assert rows == list(range(H))
