"""Host side of the one-launch 128-channel residual block (csrc/block128_i8.hip, the block128 option of lfd_amd/engine_i8.py):
the reference of tests/golden/block128_i8_cases.py against a plain float64 conv chain, the restated launch geometry, the lowering
of the layer list into launches with block128=True, synthetic layer lists that must or must not fuse, and the status codes of
refused calls.  No GPU: a refused call returns before any launch."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import block128_i8_cases as BC
from lfd_amd import _lib, configs, engine_i8

CONFIGS = [('WIDERFACE_LFD_S', 3), ('WIDERFACE_LFD_XS', 3), ('TT100K_LFD_L', 3), ('TL_LFD_L', 3),
           ('WIDERFACE_LFD_S', 1), ('WIDERFACE_LFD_XS', 1), ('TT100K_LFD_L', 1), ('TL_LFD_L', 1)]
IDS = ['%s%s' % (n, '_gray' if c == 1 else '') for n, c in CONFIGS]
# int8 launches of the stages per forward under fused='full', block128=True
LAUNCHES = {'WIDERFACE_LFD_S': 12, 'WIDERFACE_LFD_XS': 12, 'TT100K_LFD_L': 14}
KINDS = dict((c.kind, c) for c in BC.cases())


def _conv_f64(x, w):
    """NHWC int8 x, OIHW int8 w -> NHWC float64 (exact: |sum| < 2^31), 3x3 stride 1 over an explicitly zero-padded input"""
    xp = F.pad(x.permute(0, 3, 1, 2).double(), (1, 1, 1, 1), value=0.0)
    return F.conv2d(xp, w.double()).permute(0, 2, 3, 1)


def _requant(v):
    return torch.round(v).clamp(-127, 127).to(torch.int8)


@pytest.mark.parametrize('kind', ['pixel', 'edge', 'general'])
@pytest.mark.parametrize('big_bias', [False, True])
def test_reference_is_a_plain_float64_conv_chain(kind, big_bias):
    c = KINDS[kind]
    x, w1, w2 = BC.operands(c)
    assert tuple(x.shape) == (c.n, c.h, c.w, 128) and tuple(w1.shape) == tuple(w2.shape) == (128, 128, 3, 3)
    assert not torch.equal(w1, w2) and int(w1.min()) == int(w2.min()) == -127 and int(w1.max()) == int(w2.max()) == 127
    assert kind == 'pixel' or (int(x.min()), int(x.max())) == (-127, 127)      # full range, independent draws
    k1, k2 = BC.exact_constants(c, big_bias)
    mid, v, q, f = BC.block128_ref(x, w1, w2, k1, k2)
    mid2 = _requant((_conv_f64(x, w1) * k1.mult.double() + k1.biasq.double()).clamp(min=0))
    assert torch.equal(mid, mid2)
    a2 = _conv_f64(mid2, w2)                                   # pads the MID map with zeros: conv2's padding rule
    v2 = (a2 * k2.mult.double() + k2.biasq.double() + x.double() * k2.res_mult).clamp(min=0)
    assert torch.equal(v, v2) and torch.equal(q, _requant(v2)) and torch.equal(f, v2 * k2.out_scale)
    assert torch.equal(v.float().double(), v)                  # the instrument: exact in fp32
    if kind != 'pixel':
        assert int(q.max()) == 127 and int(q.min()) == 0 and 0.3 < float(((q > 0) & (q < 127)).double().mean())
    if big_bias:
        # the padding rule is observable: conv1 evaluated on the all-zero input outside the image would be BIG_BIAS, and conv2
        # of a mid map padded with it differs from the reference
        midp = F.pad(mid2.permute(0, 3, 1, 2).double(), (1, 1, 1, 1), value=BC.BIG_BIAS)
        assert not torch.equal(F.conv2d(midp, w2.double()).permute(0, 2, 3, 1), a2)


def test_shape_table_and_launch_geometry():
    assert (BC.TH, BC.TW, BC.MAX_WORKGROUPS, BC.C) == (8, 16, 256, 128)
    assert sorted(KINDS) == ['edge', 'general', 'pixel', 'walk']
    assert (KINDS['pixel'].n, KINDS['pixel'].h, KINDS['pixel'].w) == (1, 1, 1) and BC.launch(KINDS['pixel']) == (1, 1, 1, 1)
    e = KINDS['edge']
    assert (e.n, e.h, e.w) == (2, BC.TH + 1, BC.TW + 1) and BC.launch(e) == (2, 2, 8, 8)
    g = KINDS['general']
    assert (g.n, g.h, g.w) == (2, 37, 53) and g.h % BC.TH and g.w % BC.TW and BC.launch(g) == (4, 5, 40, 40)
    w = KINDS['walk']
    tx, ty, nt, grid = BC.launch(w)
    assert (tx, ty) == (3, 2) and (w.h, w.w) == (BC.TH + 1, 2 * BC.TW + 1)      # a ragged row and a ragged column of one pixel
    assert grid == BC.MAX_WORKGROUPS < nt and nt / grid >= 3.5 and nt // grid == 3 and 0 < nt % grid
    assert w.n == BC._walk_images(BC.MAX_WORKGROUPS) and (w.n - 1) * tx * ty < 3.5 * grid      # no image more than needed
    # a workgroup's consecutive tiles b, b + grid, ...: another image (grid >= a whole image), another place (grid % 6 != 0)
    assert grid >= tx * ty and grid % (tx * ty) != 0


def _plans(name, ch):
    m = configs.build_model(name, seed=666, input_channels=ch)
    m.eval()
    args = (m._backbone, m._neck, m._head, torch.device('cpu'))
    return (engine_i8.Int8Plan(*args), engine_i8.Int8Plan(*args, fused=True), engine_i8.Int8Plan(*args, fused='full'),
            engine_i8.Int8Plan(*args, fused=True, block128=True), engine_i8.Int8Plan(*args, fused='full', block128=True))


def _is_block128(lay, i):
    """the issue's conditions for one 'block128' launch over layers i, i + 1, written out independently of lower_fused"""
    if i + 1 >= len(lay):
        return False
    a, b = lay[i], lay[i + 1]
    others = [c for j, c in enumerate(lay) if j not in (i, i + 1)]
    return ((a.ks, a.stride, a.relu, a.res, a.tap) == (3, 1, True, None, None) and (b.ks, b.stride, b.relu) == (3, 1, True)
            and (a.cin, a.cout, b.cin, b.cout) == (128,) * 4 and b.src == a.dst and b.res == a.src
            and all(a.dst not in (c.src, c.res) for c in others))


@pytest.mark.parametrize('name,ch', CONFIGS, ids=IDS)
def test_lowering_with_block128(name, ch):
    plain, fused, full, fused_b, full_b = _plans(name, ch)
    lay = plain.layers
    assert [p.route for p in (plain, fused, full, fused_b, full_b)] == ['layers', 'fused', 'full', 'fused', 'full']
    assert [p.block128 for p in (plain, fused, full, fused_b, full_b)] == [False, False, False, True, True]
    assert engine_i8.ROUTES == ('layers', 'fused', 'full')
    # without the option the function returns what it returned before
    assert fused.launches == engine_i8.lower_fused(lay) == engine_i8.lower_fused(lay, block128=False)
    assert full.launches == engine_i8.lower_fused(lay, entry=True) == engine_i8.lower_fused(lay, entry=True, block128=False)
    assert not [l for p in (fused, full) for l in p.launches if l.kind == 'block128']
    starts = [i for i in range(len(lay)) if _is_block128(lay, i)]
    assert (len(starts) > 0) == (name != 'WIDERFACE_LFD_XS')
    if name == 'TL_LFD_L':
        assert len(starts) == 3
    for base, opt, entry in ((fused, fused_b, False), (full, full_b, True)):
        la = opt.launches
        assert la == engine_i8.lower_fused(lay, entry=entry, block128=True)    # a pure function of the layer list
        assert [i for l in la for i in l.layers] == list(range(len(lay)))      # every layer once, in order
        # a 'block128' exactly where the conditions hold, replacing two 'conv' launches; everything else as without the option
        assert [l.layers for l in la if l.kind == 'block128'] == [(i, i + 1) for i in starts]
        expect = []
        for l in base.launches:
            if l.layers[0] in starts:
                assert l.kind == 'conv'
                expect.append(engine_i8.Launch('block128', (l.layers[0], l.layers[0] + 1)))
            elif l.layers[0] - 1 in starts:
                assert l.kind == 'conv'
            else:
                expect.append(l)
        assert la == expect
        assert opt.int8_launches() == len(la) == base.int8_launches() - len(starts)
        # conv1's map of every 'block128' launch has no buffer; no launch reads or adds a map that nothing writes
        assert opt.unwritten == base.unwritten | frozenset(lay[i].dst for i in starts)
        for k, l in enumerate(la):
            inside = set(lay[i].dst for i in l.layers)
            outside = set(b for i in l.layers for b in (lay[i].src, lay[i].res) if b is not None and b not in inside)
            assert not (outside & opt.unwritten) or (k == opt.entry_f16 and outside & opt.unwritten == set([0]))
        assert opt.entry_f16 == base.entry_f16
        # tap_ready_after indexes the new launch list: the launch in front of it carries the tap
        assert len(opt.tap_ready_after) == len(plain.tap_ready_after) == len(opt.taps) > 0
        for k, after in enumerate(opt.tap_ready_after):
            l = la[after - 1 - len(opt.convs)]
            assert opt.layers[l.layers[-1]].tap == opt.taps[k]
        assert opt.tap_ready_after[-1] == len(opt.convs) + len(la)
        assert opt.tensor_names == plain.tensor_names and opt.taps == plain.taps and opt.qbuf_channels == plain.qbuf_channels
    if name == 'WIDERFACE_LFD_XS':                              # no eligible block: the same launch lists as without the option
        assert fused_b.launches == fused.launches and full_b.launches == full.launches
        assert fused_b.unwritten == fused.unwritten and full_b.unwritten == full.unwritten


def test_launch_counts_of_the_shipped_configurations():
    """int8 launches per forward under fused='full', block128=True: the 'full' count minus one per eligible 128-channel block
    (derived in test_lowering_with_block128), then the literals"""
    got = {}
    for name in sorted(LAUNCHES):
        plain, fused, full, fused_b, full_b = _plans(name, 3)
        n128 = len([i for i in range(len(plain.layers)) if _is_block128(plain.layers, i)])
        assert full_b.int8_launches() == full.int8_launches() - n128 and fused_b.int8_launches() == fused.int8_launches() - n128
        got[name] = full_b.int8_launches()
    assert got == LAUNCHES


def _layer(i, cin, cout, ks, stride, src, res=None, tap=None):
    c = engine_i8.ConvI8()
    c.cin, c.cout, c.ks, c.stride, c.relu, c.src, c.dst, c.res, c.tap = cin, cout, ks, stride, True, src, i + 1, res, tap
    return c


def _kinds(lays, **kw):
    return [l.kind for l in engine_i8.lower_fused(lays, **kw)]


def test_synthetic_layer_lists():
    blk = [_layer(0, 128, 128, 3, 1, 0), _layer(1, 128, 128, 3, 1, 1, res=0)]
    assert engine_i8.lower_fused(blk, block128=True) == [engine_i8.Launch('block128', (0, 1))]
    assert _kinds(blk) == _kinds(blk, block128=False) == ['conv', 'conv'] and _kinds(blk, entry=True, block128=True) == ['block128']
    # a tapped block fuses (conv2 carries the tap); a tap on conv1 does not
    assert _kinds([blk[0], _layer(1, 128, 128, 3, 1, 1, res=0, tap=7)], block128=True) == ['block128']
    assert _kinds([_layer(0, 128, 128, 3, 1, 0, tap=7), blk[1]], block128=True) == ['conv', 'conv']
    # conv1's map read by a third layer, as input or as residual
    assert _kinds(blk + [_layer(2, 128, 128, 3, 1, 1)], block128=True) == ['conv', 'conv', 'conv']
    assert _kinds(blk + [_layer(2, 128, 128, 3, 1, 2, res=1)], block128=True) == ['conv', 'conv', 'conv']
    # a 1x1 conv in either place, stride 2, a 64 -> 128 block, a residual that is not the block's input
    assert _kinds([_layer(0, 128, 128, 1, 1, 0), blk[1]], block128=True) == ['conv', 'conv']
    assert _kinds([blk[0], _layer(1, 128, 128, 1, 1, 1, res=0)], block128=True) == ['conv', 'conv']
    assert _kinds([_layer(0, 128, 128, 3, 2, 0), blk[1]], block128=True) == ['conv', 'conv']
    assert _kinds([_layer(0, 64, 128, 3, 1, 0), blk[1]], block128=True) == ['conv', 'conv']
    assert _kinds([blk[0], _layer(1, 128, 128, 3, 1, 1, res=None)], block128=True) == ['conv', 'conv']
    # the 64-channel block is untouched by the option, and two blocks in a row both fuse
    b64 = [_layer(0, 64, 64, 3, 1, 0), _layer(1, 64, 64, 3, 1, 1, res=0)]
    assert _kinds(b64, block128=True) == _kinds(b64) == ['block']
    two = blk + [_layer(2, 128, 128, 3, 1, 2), _layer(3, 128, 128, 3, 1, 3, res=2)]
    assert engine_i8.lower_fused(two, block128=True) == [engine_i8.Launch('block128', (0, 1)), engine_i8.Launch('block128', (2, 3))]
    assert engine_i8.lower_fused([], block128=True) == []


def test_block128_needs_a_fused_route():
    m = configs.build_model('WIDERFACE_LFD_S', seed=666)
    m.eval()
    args = (m._backbone, m._neck, m._head, torch.device('cpu'))
    with pytest.raises(ValueError):
        engine_i8.Int8Plan(*args, fused=False, block128=True)
    with pytest.raises(ValueError):
        engine_i8.Int8Plan(*args, block128=True)
    for bad in (1, 0, None, 'yes'):
        with pytest.raises(ValueError):
            engine_i8.Int8Plan(*args, fused=True, block128=bad)
    for bad in ('all', 'fused', 2, None, 'Full'):               # the routes keep their three values
        with pytest.raises(ValueError):
            engine_i8.Int8Plan(*args, fused=bad, block128=True)


def test_refused_calls_return_status_codes():
    l = _lib.lib()
    buf = (C.c_char * 4096)()
    base = C.addressof(buf)
    base += -base % 16
    a, b, c_, odd = (C.c_void_p(base + o) for o in (0, 1024, 2048, 1028))

    def block(n=1, h=4, w=4, x=a, w1=b, m1=b, b1=b, w2=b, m2=b, b2=b, out=c_, f=None):
        return l.lfd_block128_i8_fused(n, h, w, x, w1, m1, b1, w2, m2, b2, 0.5, out, f, 1.0, None)

    for kw in (dict(x=None), dict(w1=None), dict(m1=None), dict(b1=None), dict(w2=None), dict(m2=None), dict(b2=None), dict(out=None),
               dict(x=odd), dict(w1=odd), dict(m1=odd), dict(b1=odd), dict(w2=odd), dict(m2=odd), dict(b2=odd), dict(out=odd),
               dict(f=odd), dict(n=0), dict(h=0), dict(w=-1), dict(out=a)):
        assert block(**kw) == -1, kw
    assert block(h=4096, w=4096) == -4 and block(h=1, w=2 ** 24) == -4          # h * w * 128 >= 2^31
    assert all(v == b'\x00' for v in buf)                       # host memory here: nothing was launched, nothing written
