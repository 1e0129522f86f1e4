"""Cases of the wide output pass of csrc/head.hip -- lfd_head_forward_wide_f16, k_head2 with three and four tiles of final rows -- on
the instrument of tests/golden/head_cases.py, which is used as it is: operands, the float64 chain, the float32 emulations, the launch
geometry and the guarded device buffers.  Shared by tests/test_gpu_wide_head_infer.py (the device) and
tests/test_wide_head_infer_host.py (the gates and the walk properties, on the CPU)."""
import ctypes as C

import head_cases as H

# rows = (regression rows, class rows).  64 < rows <= 96: three tiles, <= 128: four.
CASES = [
    H.case('w84', 3, [(96, 64), (33, 128)], rows=(4, 80), seed=31),                       # ft 3, every class row in a 16-byte store
    H.case('w65', 1, [(63, 64), (31, 128)], rows=(4, 61), seed=32),                       # the first wide row count: one live row in tile 3
    H.case('w85', 1, [(65, 64), (1, 128)], rows=(4, 81), seed=33),                        # 81 class channels: scalar stores
    H.case('w128', 3, [(65, 64), (33, 128)], rows=(4, 124), seed=34),                     # ft 4, row 127 live
    H.case('wc128', 1, [(127, 64), (96, 128)], rows=(0, 128), scale=False, seed=35),      # separate class tower, every row of four tiles
    H.case('wc81', 1, [(127, 64), (96, 128)], rows=(0, 81), scale=False, seed=36),
    H.case('w84_g8', 3, [(96, 64), (33, 128)], groups=8, rows=(4, 80), seed=37),
    H.case('w84_walk', 3, [(1368 * 32 + 5, 64)], chunk=2, rows=(4, 80), seed=38),         # a block runs three items
    H.case('w84_switch', 1, [(33253, 64), (17893, 128)], chunk=2, rows=(4, 80), seed=39),
    # the two levels above make 200 work items, fewer than the 256 blocks of a launch: every block runs one item.  The level table of
    # head_cases' own 'switch' case (400 items) is the smallest of its kind in which a workgroup changes level, and neck K length,
    # inside its walk -- the final filter of a wide head is then re-fetched behind the level-switch barrier
    H.case('w84_switch4', 1, [(33253, 64), (33253, 64), (17893, 128), (17893, 128)], chunk=2, rows=(4, 80), seed=40),
]
BY_NAME = dict((c['name'], c) for c in CASES)
WALKS = ('w84_walk', 'w84_switch', 'w84_switch4')
# every k_head2 variant ships for wide heads: the three output-pass instantiations (plain, AccVGPR-resident folded filters, stored
# tower-1 activations) of both tile counts compile without scratch
VARIANTS = list(H.VARIANTS)

# Gates: head_cases.GATES['head2'] wherever the float32 emulations of a case stay within a quarter of it
# (tests/test_wide_head_infer_host.py re-derives that); a case that does not gets its own figure here, by head_cases' rule: 4 x the
# largest emulation deviation, rounded up by at most a tenth.
CASE_GATES = {
    # the three large cases: the largest of 4 .. 10 million class logits sits further out than that of the small cases the shared
    # gate was derived over (a quarter of it: 3.125e-3)
    'w84_walk': dict(cls=1.4e-2),           # emulation 3.376e-3
    'w84_switch': dict(cls=1.4e-2),         # emulation 3.336e-3
    'w84_switch4': dict(cls=1.5e-2, reg=1.9e-2),       # emulations 3.542e-3, 4.669e-3 (a quarter of the shared reg gate: 4.5e-3)
}


def gate(name, key):
    return CASE_GATES.get(name, {}).get(key, H.GATES['head2'][key])


class WideDevice(H.Device):
    """head_cases.Device whose output pass is lfd_head_forward_wide_f16 (passes 1 and 2 and the finalize calls: the shared entries)"""

    def forward(self, p, d=None, lv=None, ab2=True):
        if p != 3:
            return H.Device.forward(self, p, d=d, lv=lv, ab2=ab2)
        from lfd_amd._lib import lib, stream_ptr
        P = C.c_void_p
        return lib().lfd_head_forward_wide_f16(C.byref(d or self.d), lv or self.lv, P(self.ab[0].ptr), P(self.ab[1].ptr if ab2 else 0),
                                               P(self.cls.ptr), P(self.reg.ptr), P(self.zeros.data_ptr()), stream_ptr())
