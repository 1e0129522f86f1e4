"""Host side of the stem_int8 option (lfd_stem_conv_i8 in csrc/stem.hip, lfd_stem_faster_fused_i8 in csrc/stem_fused.hip, the
stem_int8 keyword of lfd_amd/engine_i8.py and lfd_amd/deployment.py): the reference of tests/golden/stem_i8_cases.py
against an independent torch double chain and against hand-derived values, the restated launch geometry of the case tables,
Int8Plan.stem_int8_formats for every shipped configuration, the refused option values, what the option leaves unchanged in the
plan, the new exports and the status codes of refused calls.  No GPU: a refused call returns before any launch.

The tests of the reference itself (test_quantize_ref_hand_derived_values, test_reference_equals_an_independent_double_chain) check
the instrument, not the feature: they need only this file's golden module and would pass on a tree without the kernels.  Every
other test here needs the new symbols or the new keyword."""
import ctypes as C
import os
import re

import numpy
import pytest
import torch
import torch.nn.functional as F

import stem_cases as S
import stem_i8_cases as Q
from lfd_amd import _lib, configs, engine_i8, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# name -> the frame formats (in_format) for which the stem launch writes int8 under stem_int8=True.  'fast' stems of 64 stored
# channels (TL_LFD_S: 48 real ones padded to 64) take all three; 'faster' stems the two NHWC formats (NCHW fp32 frames run the
# two-kernel stem); the 32-channel 'faster' stem of WIDERFACE_LFD_XS none
FORMATS = {'WIDERFACE_LFD_XS': (), 'WIDERFACE_LFD_S': (1, 2), 'WIDERFACE_LFD_M': (0, 1, 2), 'WIDERFACE_LFD_L': (0, 1, 2),
           'TT100K_LFD_S': (1, 2), 'TT100K_LFD_L': (0, 1, 2), 'TL_LFD_S': (0, 1, 2), 'TL_LFD_L': (0, 1, 2)}


# ------------------------------------------------------------------------------------------------ the reference
def test_quantize_ref_hand_derived_values():
    q = Q.quantize_ref
    # products exactly on x.5 round to the even neighbour
    assert q(numpy.array([0.5, 1.5, 2.5, 3.5, 126.5]), 1.0).tolist() == [0, 2, 2, 4, 126]
    assert q(numpy.array([1.0, 3.0, 5.0, 7.0]), 0.25).tolist() == [0, 1, 1, 2]              # 0.25, 0.75, 1.25, 1.75
    assert q(numpy.array([2.0, 6.0, 10.0]), 0.25).tolist() == [0, 2, 2]                      # 0.5, 1.5, 2.5
    # the clamp, both ways (the stem's outputs are ReLU outputs, the function does not rely on it)
    assert q(numpy.array([127.4, 127.6, 508.0, 510.0, 2048.0, -2048.0]), 1.0).tolist() == [127, 127, 127, 127, 127, -127]
    assert q(numpy.array([508.0, 509.0, 510.0, 511.0, 512.0]), 0.25).tolist() == [127, 127, 127, 127, 127]      # 127.25 is above
    assert q(numpy.array([506.0, 507.0]), 0.25).tolist() == [126, 127]                       # 126.5 -> 126 (even), 126.75 -> 127
    # the fp16 rounding comes first: 2.4996 is 2.5 in fp16 (spacing 2^-9), and 2.5 * 3 = 7.5 -> 8; unrounded it would be 7
    assert q(numpy.array([2.4996]), 3.0).tolist() == [8] and int(numpy.rint(2.4996 * 3.0)) == 7
    # the product is ONE fp32 multiply: fp16(0.1) = 0.0999755859375, times fp32(10) = 0.999755859375 -> 1
    assert q(numpy.array([0.1]), 10.0).tolist() == [1]
    # ... and it is rounded to fp32 before rint: fp32(1 / 3) = 11184811 * 2^-25, times 1.5 = 16777216.5 * 2^-25, which needs 25
    # bits and rounds (to even) to 0.5 exactly -> 0; the same product in float64 is 0.5000000149 -> 1
    assert q(numpy.array([1.5]), 1.0 / 3.0).tolist() == [0]
    assert int(numpy.rint(1.5 * float(numpy.float32(1.0 / 3.0)))) == 1
    assert q(torch.tensor([[0.5, 300.0]], dtype=torch.float64), 1.0).tolist() == [[0, 127]]  # a torch tensor, shape kept
    assert q(numpy.zeros((2, 3)), 5.0).dtype == numpy.int8


def _double_chain_i8(values, stages, inv_scale):
    """independent of stem_cases.stem_ref and of numpy: F.conv2d in float64 with its own padding, fp16 between the stages and at
    the end, the quantise step with torch"""
    y = values.permute(0, 3, 1, 2).double()
    for w, b, stride in stages:
        y = F.conv2d(y, w.double(), b.double(), stride=stride, padding=w.shape[-1] // 2).relu()
        y = y.float().half().double()
    p = y.permute(0, 2, 3, 1).float() * torch.tensor(inv_scale, dtype=torch.float32)
    return torch.round(p).clamp(-127, 127).to(torch.int8)


@pytest.mark.parametrize('inst', Q.PAIR_INSTANCES + Q.X2_INSTANCES[::2], ids=S.inst_id)
@pytest.mark.parametrize('gauss', [None, 0, 1], ids=['gauss', 'int_ties', 'int_clamp'])
def test_reference_equals_an_independent_double_chain(inst, gauss):
    n, h, w = (2, 37, 53)
    if gauss is None:
        values, stages = S.gauss_values(inst, n, h, w, 5), S.gauss_stages(inst, 5)
        if inst.fmt == S.FMT_U8:
            values = S.int_values(inst, n, h, w, 5)
        y = S.stem_ref(values, stages)
        inv = 113.7 / float(y.abs().max())                      # no power of two
    else:
        values, stages = S.int_values(inst, n, h, w, 5), S.int_stages(inst, 5)
        inv = Q.INT_INV_SCALES[gauss]
    got = Q.stem_i8_ref(values, stages, inv)
    ref = _double_chain_i8(values, stages, inv)
    assert got.dtype == numpy.int8 and got.shape == tuple(ref.shape) == (n,) + S.out_map(inst, h, w) + (64,)
    assert numpy.array_equal(got, ref.numpy())
    assert got.min() >= 0 and Q.FILL not in got
    if gauss is not None:
        # the instrument: exact in fp16; ties with the first inv_scale, clamped values with the second
        assert Q.INT_INV_SCALES == (0.5, 2.0)
        y = S.stem_ref(values, stages)
        assert float(y.abs().max()) <= S.F16_EXACT and torch.equal(y, y.round())
        p = y * inv
        if gauss == 0:
            assert int((p - p.floor() == 0.5).sum()) > got.size // 8
        else:
            assert int((p > 127.5).sum()) > got.size // 100 and got.max() == 127
        assert int(((got > 0) & (got < 127)).sum()) > got.size // 8       # and most of the rest is neither 0 nor clamped


def test_case_tables_restate_the_launch_geometry():
    pair = Q.PAIR_INSTANCES[1]
    assert S.tile_geometry(pair) == (4, 32, 1, 2048, False)
    L = [S.launch(pair, *s) for s in Q.PAIR_SHAPES]
    assert [(l.tiles_x, l.tiles_y, l.ntiles, l.blocks) for l in L] == [(1, 1, 1, 1), (1, 1, 1, 1), (2, 2, 4, 4), (1, 5, 10, 10),
                                                                         (12, 32, 3072, 2048)]
    assert [S.out_map(pair, h, w) for _, h, w in Q.PAIR_SHAPES[:3]] == [(1, 1), (4, 32), (5, 33)]
    x2 = Q.X2_INSTANCES[0]
    assert S.tile_geometry(x2) == (4, 32, 2, 256, True)
    geo = dict((c, S.launch(x2, c.n, c.h, c.w)) for c in (Q.X2_ONE_PIXEL, Q.X2_ONE_TILE, Q.X2_PAST_TILE, Q.X2_896, Q.X2_STAGGER, Q.X2_WIDTH))
    assert (geo[Q.X2_ONE_PIXEL].ntiles, geo[Q.X2_ONE_PIXEL].blocks) == (1, 8) and S.out_map(x2, 16, 128) == (4, 32)
    assert (geo[Q.X2_ONE_TILE].ntiles, geo[Q.X2_PAST_TILE].ntiles) == (1, 4) and S.out_map(x2, 17, 129) == (5, 33)
    assert (geo[Q.X2_896].ntiles, geo[Q.X2_896].blocks) == (896, 256)                         # 3.5 tiles per workgroup
    assert geo[Q.X2_STAGGER].ntiles >= 4096 and S.x2_stagger_active(geo[Q.X2_STAGGER]) and not S.x2_stagger_active(geo[Q.X2_896])
    assert Q.X2_WIDTH.w % 8 != 0 and Q.X2_PAST_TILE.w % 8 != 0
    for inst in Q.X2_INSTANCES:
        cases = Q.x2_cases(inst)
        assert len(set(cases)) == len(cases)
        for c in cases:                                         # every case reaches its <U8, ALN> instantiation
            aligned_rows = c.w % 8 == 0 and c.route != 'knob'
            assert (aligned_rows and (inst.fmt == S.FMT_U8 or c.route != 'misaligned')) == bool(inst.aln), (inst, c)
        assert [c.stagger for c in cases if (c.n, c.h, c.w) == S.X2_C] == [0, 1]
        assert any((c.n, c.h, c.w) == (4, 448, 1024) for c in cases)
    fu = open(os.path.join(ROOT, 'lfd-a-light-and-fast-detector_amd', 'csrc', 'stem_fused.hip')).read()
    st = open(os.path.join(ROOT, 'lfd-a-light-and-fast-detector_amd', 'csrc', 'stem.hip')).read()
    for a, b in (('false', 'true'), ('false', 'false'), ('true', 'true'), ('true', 'false')):
        assert 'launch_stem2x<%s, %s, true>(a, st)' % (a, b) in fu
    assert st.count('return launch_stem<2, IN_') == 3 and 'k_stem<NCT, FMT, TAIL, OI8>' in st


# ------------------------------------------------------------------------------------------------ plan and interface
def _args(name, ch=3):
    m = configs.build_model(name, seed=666, input_channels=ch)
    m.eval()
    return (m._backbone, m._neck, m._head, torch.device('cpu'))


@pytest.mark.parametrize('name', sorted(FORMATS))
def test_stem_int8_formats_of_the_shipped_configurations(name):
    assert sorted(configs.ARCHS) == sorted(FORMATS)
    args = _args(name)
    for fused, b128 in ((False, False), (True, False), ('full', False), ('full', True)):
        on = engine_i8.Int8Plan(*args, fused=fused, block128=b128, stem_int8=True)
        off = engine_i8.Int8Plan(*args, fused=fused, block128=b128)
        assert on.stem_int8 is True and off.stem_int8 is False
        assert isinstance(on.stem_int8_formats, frozenset) and on.stem_int8_formats == frozenset(FORMATS[name])
        assert off.stem_int8_formats == frozenset()
        # the launch list, the layers and the names do not depend on the option
        assert on.launches == off.launches and on.int8_launches() == off.int8_launches() and on.tensor_names == off.tensor_names
        assert [c.name for c in on.layers] == [c.name for c in off.layers] and on.taps == off.taps
        assert on.tap_ready_after == off.tap_ready_after and on.entry_f16 == off.entry_f16
        assert on.qbuf_channels == off.qbuf_channels and on.route == off.route and on.block128 == off.block128
        if fused == 'full':
            assert off.entry_f16 == 0 and 0 in off.unwritten
            # an eligible stem writes int8 buffer 0, so it has a buffer; nothing else changes
            assert on.unwritten == (off.unwritten - frozenset([0]) if FORMATS[name] else off.unwritten)
        else:
            assert on.unwritten == off.unwritten and 0 not in on.unwritten
    # the stem launch the fp16 plan runs: one-launch 'faster' stem <-> formats without NCHW fp32
    assert (on.stem_fused is not None) == (on.backbone._stem_mode == 'faster')
    assert on.stem_channels_real == {'TL_LFD_S': 48, 'WIDERFACE_LFD_XS': 32}.get(name, 64)
    assert on.buf_channels[on.stage_in] == (32 if name == 'WIDERFACE_LFD_XS' else 64)


@pytest.mark.parametrize('name', ['WIDERFACE_LFD_S', 'TT100K_LFD_L', 'TL_LFD_S'])
def test_gray_models_have_no_int8_stem(name):
    for fused in (False, 'full'):
        p = engine_i8.Int8Plan(*_args(name, 1), fused=fused, stem_int8=True)
        q = engine_i8.Int8Plan(*_args(name, 1), fused=fused)
        assert p.stem_int8 is True and p.stem_int8_formats == frozenset() and p.unwritten == q.unwritten and p.launches == q.launches


def test_refused_option_values():
    args = _args('WIDERFACE_LFD_S')
    for bad in (1, 0, 'yes', numpy.bool_(True), numpy.bool_(False), None):
        for fused in (False, True, 'full'):
            with pytest.raises(ValueError):
                engine_i8.Int8Plan(*args, fused=fused, stem_int8=bad)
    for fused in (False, True, 'full'):                         # allowed with every route
        assert engine_i8.Int8Plan(*args, fused=fused, stem_int8=True).stem_int8 is True
    with pytest.raises(ValueError):                             # the other options keep their rules
        engine_i8.Int8Plan(*args, fused=False, block128=True, stem_int8=True)


def test_supported_queries_and_exports():
    header = open(os.path.join(ROOT, 'include', 'lfd_hip.h')).read()
    for sym in ('lfd_stem_conv_i8', 'lfd_stem_conv_i8_supported', 'lfd_stem_faster_fused_i8', 'lfd_stem_faster_fused_i8_supported'):
        assert re.search(r'LFD_API int %s\(' % sym, header), sym
        assert sym in _lib._SIGNATURES and _lib._SIGNATURES[sym][0] is C.c_int
        assert getattr(_lib.lib(), sym).restype is C.c_int
    for fmt in (0, 1, 2):
        assert ops.stem_conv_i8_supported(fmt, 64, True)
        assert not ops.stem_conv_i8_supported(fmt, 64, False) and not ops.stem_conv_i8_supported(fmt, 32, True)
        assert not ops.stem_conv_i8_supported(fmt, 48, True) and not ops.stem_conv_i8_supported(fmt, 128, True)
        assert ops.stem_faster_fused_i8_supported(fmt, 64) == (fmt != 0) and not ops.stem_faster_fused_i8_supported(fmt, 32)
    assert not ops.stem_conv_i8_supported(3, 64, True) and not ops.stem_conv_i8_supported(-1, 64, True)
    assert not ops.stem_faster_fused_i8_supported(3, 64)
    import inspect
    from lfd_amd import deployment
    sig = inspect.signature(deployment.build_int8_engine)
    assert list(sig.parameters)[2:] == ['fused', 'block128', 'stem_int8'] and sig.parameters['stem_int8'].default is False
    assert isinstance(deployment.Int8Engine.stem_int8, property)


def test_refused_calls_return_status_codes():
    l = _lib.lib()
    buf = (C.c_char * 8192)()
    base = C.addressof(buf)
    base += -base % 16
    a, b, c_, odd = (C.c_void_p(base + o) for o in (0, 1024, 2048, 1028))
    INVALID, UNSUPPORTED = -1, -4

    def pair(x=a, fmt=1, n=1, h=4, w=4, ch=64, w1=b, b1=b, w2=b, b2=b, out=c_):
        return l.lfd_stem_conv_i8(x, fmt, n, h, w, ch, w1, b1, w2, b2, 0.5, out, None)

    def chain(x=a, fmt=1, n=1, h=4, w=4, ch=64, w1=b, b1=b, w2=b, b2=b, w3=b, b3=b, w4=b, b4=b, out=c_):
        return l.lfd_stem_faster_fused_i8(x, fmt, n, h, w, ch, w1, b1, w2, b2, w3, b3, w4, b4, 0.5, out, None)

    for kw in (dict(x=None), dict(w1=None), dict(b1=None), dict(out=None), dict(w2=None), dict(b2=None), dict(out=odd), dict(w1=odd),
               dict(b1=odd), dict(w2=odd), dict(b2=odd), dict(n=0), dict(h=0), dict(w=-1)):
        assert pair(**kw) == INVALID, kw
    for kw in (dict(ch=32), dict(ch=48), dict(ch=128), dict(fmt=3), dict(fmt=-1), dict(w2=None, b2=None)):
        assert pair(**kw) == UNSUPPORTED, kw
    for kw in ([dict([(k, None)]) for k in ('x', 'w1', 'b1', 'w2', 'b2', 'w3', 'b3', 'w4', 'b4', 'out')] +
               [dict([(k, odd)]) for k in ('w1', 'b1', 'w2', 'b2', 'w3', 'b3', 'w4', 'b4', 'out')] + [dict(n=0), dict(h=-1), dict(w=0)]):
        assert chain(**kw) == INVALID, kw
    for kw in (dict(fmt=0), dict(ch=32), dict(fmt=3), dict(fmt=2, ch=32)):
        assert chain(**kw) == UNSUPPORTED, kw
    assert all(v == b'\x00' for v in buf)                       # host memory here: nothing was launched, nothing written
