"""Host side of the one-launch stage-entry block (csrc/entry_i8.hip, the fused='full' route of lfd_amd/engine_i8.py): the reference
of tests/golden/entry_i8_cases.py against a plain int64 conv chain, what the shape table claims, that the instrument is not
degenerate, the fp16-input generator, the lowering of the layer list into launches, and the status codes of refused calls.
No GPU: a refused call returns before any launch."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import conv_i8_cases as QC
import entry_i8_cases as EC
from lfd_amd import _lib, configs, engine_i8, ops

CONFIGS = [('WIDERFACE_LFD_S', 3), ('WIDERFACE_LFD_XS', 3), ('TT100K_LFD_L', 3), ('WIDERFACE_LFD_S', 1)]
IDS = ['%s%s' % (n, '_gray' if c == 1 else '') for n, c in CONFIGS]
SLOTS = ['name', 'cin', 'cout', 'cout_real', 'ks', 'stride', 'relu', 'src', 'dst', 'res', 'tap', 'src_name', 'res_name']


def _conv_i64(x, w, stride):
    """NHWC int8 x, OIHW int8 w -> NHWC int64, explicit zero padding ks // 2"""
    p = w.shape[2] // 2
    xp = F.pad(x.permute(0, 3, 1, 2).long(), (p, p, p, p), value=0)
    return F.conv2d(xp, w.long(), stride=stride).permute(0, 2, 3, 1)


def _requant(v):
    return torch.round(v).clamp(-127, 127).to(torch.int8)


@pytest.mark.parametrize('shape', [(1, 1, 1), (2, 3, 5), (1, 4, 6), (1, 9, 17)])
@pytest.mark.parametrize('big_bias', [False, True])
def test_reference_is_a_plain_int64_conv_chain(shape, big_bias):
    c = EC.EntryCase('tiny', *shape)
    x, w1, wd, w2 = EC.operands(c)
    k1, kd, k2 = EC.exact_constants(c, big_bias)
    y1, ident, v, q = EC.entry_ref(x, w1, wd, w2, k1, kd, k2)
    oh, ow = EC.out_hw(c.h, c.w)
    assert tuple(q.shape) == tuple(y1.shape) == tuple(ident.shape) == (c.n, oh, ow, 64)
    y1b = _requant((_conv_i64(x, w1, 2).double() * k1.mult.double() + k1.biasq.double()).clamp(min=0))
    idb = _requant(_conv_i64(x, wd, 2).double() * kd.mult.double() + kd.biasq.double())
    assert torch.equal(y1, y1b) and torch.equal(ident, idb)
    a2 = _conv_i64(y1b, w2, 1)                                 # the Y1 map padded with zeros: conv2's padding rule
    v2 = (a2.double() * k2.mult.double() + k2.biasq.double() + idb.double() * k2.res_mult).clamp(min=0)
    assert torch.equal(v, v2) and torch.equal(q, _requant(v2))
    assert torch.equal(v.float().double(), v)                  # the instrument: exact in fp32
    if big_bias:
        # the padding rule is observable: conv1 evaluated on the all-zero input outside the map would be BIG_BIAS, and conv2 of
        # a y1 map padded with it differs from the reference
        y1p = F.pad(y1b.permute(0, 3, 1, 2).long(), (1, 1, 1, 1), value=int(EC.BIG_BIAS))
        assert not torch.equal(F.conv2d(y1p, w2.long()).permute(0, 2, 3, 1), a2)


def test_shape_table_holds_what_it_claims():
    kinds = dict((c.kind, c) for c in EC.cases())
    assert sorted(kinds) == ['edge_even', 'edge_odd', 'general', 'pixel', 'walk', 'walk_deep']
    assert (kinds['pixel'].n, kinds['pixel'].h, kinds['pixel'].w) == (1, 1, 1)
    odd, even = kinds['edge_odd'], kinds['edge_even']
    assert EC.out_hw(odd.h, odd.w) == EC.out_hw(even.h, even.w) == (EC.TH + 1, EC.TW + 1)      # one tile + a row and a column
    assert EC.launch(odd)[:2] == EC.launch(even)[:2] == (2, 2)
    assert odd.h % 2 == 1 and odd.w % 2 == 1 and even.h % 2 == 0 and even.w % 2 == 0
    # even: the identity branch (rows 0, 2, ..) leaves the last input row and column unread and conv1's last window ends on them;
    # odd: conv1's last window reaches one row and column into the padding
    for c, last in ((even, lambda n: n - 1), (odd, lambda n: n)):
        oh, ow = EC.out_hw(c.h, c.w)
        assert (2 * (oh - 1) + 1, 2 * (ow - 1) + 1) == (last(c.h), last(c.w))
    assert 2 * (EC.TH + 1 - 1) == even.h - 2 and 2 * (EC.TW + 1 - 1) == even.w - 2
    g = kinds['general']
    assert (g.n, g.h, g.w) == (2, 37, 53) and EC.out_hw(g.h, g.w)[0] % EC.TH and EC.out_hw(g.h, g.w)[1] % EC.TW
    assert EC.launch(g)[2] > 1
    tx, ty, nt, grid = EC.launch(kinds['walk'])
    assert (tx, ty) == (3, 2) and grid == EC.MAX_WORKGROUPS < nt and abs(nt / grid - 1.5) < 0.01
    assert EC.MAX_WORKGROUPS % (tx * ty) != 0                   # a workgroup's second tile: another image, another place
    # walk_deep: every workgroup runs at least three tiles and some four, so both LDS buffers of each kind are written twice
    tx, ty, nt, grid = EC.launch(kinds['walk_deep'])
    assert (tx, ty) == (3, 2) and grid == EC.MAX_WORKGROUPS and nt // grid == 3 and 0 < nt % grid and nt / grid >= 3.5


@pytest.mark.parametrize('c', [c for c in EC.cases() if c.kind != 'pixel'], ids=EC.case_id)
@pytest.mark.parametrize('consts', ['exact', 'random'])
def test_the_instrument_is_not_degenerate(c, consts):
    """shares of each map that are neither 0 nor at a clamp, on the reference alone: a kernel that drops a tap, a stage or the
    identity cannot hide behind saturated or all-zero outputs"""
    x, w1, wd, w2 = EC.operands(c)
    ks = EC.exact_constants(c) if consts == 'exact' else EC.random_constants(c)
    y1, ident, v, q = EC.entry_ref(x, w1, wd, w2, *ks)
    s1, sd, so = EC.useful_share(y1), EC.useful_share(ident), EC.useful_share(q)
    print('%s %s: y1 %.3f id %.3f out %.3f' % (EC.case_id(c), consts, s1, sd, so))
    assert s1 >= 0.35 and sd >= 0.70 and so >= 0.35
    assert int(q.max()) == 127 and int(q.min()) == 0 and int(ident.min()) == -127      # ReLU floor, the clamps, no ReLU on id


@pytest.mark.parametrize('channels', EC.F16_CHANNELS)
def test_f16_input_puts_products_on_and_next_to_half_integers(channels):
    c = EC.EntryCase('tiny', 2, 9, 11)
    x, inv = EC.f16_input(c, channels, exact=True)
    assert x.dtype == torch.float16 and tuple(x.shape) == (2, 9, 11, channels) and inv == 4.0
    p = x.double() * inv                                        # exact: fp16 times a power of two
    assert torch.equal((x.float() * inv).double(), p)
    tie = (p - torch.floor(p)) == 0.5
    near = ((p - torch.floor(p)) - 0.5).abs() < 0.26
    assert 0.2 < float(tie.double().mean()) < 0.3 and float((near & ~tie).double().mean()) > 0.4
    q = EC.quantize_ref(x, inv)
    assert tuple(q.shape) == (2, 9, 11, 64) and bool((q[..., channels:] == 0).all())
    assert int(q.max()) == 127 and int(q.min()) == -127         # both clamps are reached
    # a wrong rounding mode is visible: half away from zero differs on the ties towards an even value, truncation nearly everywhere
    away = (torch.sign(p) * torch.floor(p.abs() + 0.5)).clamp(-127, 127).to(torch.int8)
    assert 0.05 < float((away != q[..., :channels]).double().mean())
    assert float((torch.trunc(p).clamp(-127, 127).to(torch.int8) != q[..., :channels]).double().mean()) > 0.3
    # the arbitrary scale: three quarters of the products lie within an fp16 step or two of a half-integer, where the one rounded
    # fp32 multiply decides the side
    xr, invr = EC.f16_input(c, 64, exact=False)
    pr = (xr.float() * torch.tensor(invr, dtype=torch.float32)).double()
    assert invr != 4.0 and float((((pr - torch.floor(pr)) - 0.5).abs() < 0.2).double().mean()) > 0.7
    assert int(EC.quantize_ref(xr, invr).max()) == 127 and int(EC.quantize_ref(xr, invr).min()) == -127


def _plans(name, ch):
    m = configs.build_model(name, seed=666, input_channels=ch)
    m.eval()
    args = (m._backbone, m._neck, m._head, torch.device('cpu'))
    return engine_i8.Int8Plan(*args), engine_i8.Int8Plan(*args, fused=True), engine_i8.Int8Plan(*args, fused='full')


def _is_entry(lay, i):
    """the issue's conditions for one 'entry' launch over layers i, i + 1, i + 2, written out independently of lower_fused"""
    if i + 2 >= len(lay):
        return False
    d, c1, c2 = lay[i], lay[i + 1], lay[i + 2]
    others = [c for j, c in enumerate(lay) if j not in (i, i + 1, i + 2)]
    return ((d.ks, d.stride, d.relu, d.res, d.tap) == (1, 2, False, None, None)
            and (c1.ks, c1.stride, c1.relu, c1.res, c1.tap) == (3, 2, True, None, None) and c1.src == d.src
            and (d.cin, d.cout, c1.cin, c1.cout, c2.cin, c2.cout) == (64,) * 6
            and (c2.ks, c2.stride, c2.relu, c2.tap) == (3, 1, True, None) and (c2.src, c2.res) == (c1.dst, d.dst)
            and all(b not in (c.src, c.res) for c in others for b in (d.dst, c1.dst)))


@pytest.mark.parametrize('name,ch', CONFIGS, ids=IDS)
def test_lowering_of_the_full_route(name, ch):
    plain, fused, full = _plans(name, ch)
    assert (plain.route, fused.route, full.route) == ('layers', 'fused', 'full') == engine_i8.ROUTES
    assert plain.fused is False and fused.fused is True and full.fused == 'full' and full.fused
    lay = plain.layers
    la = full.launches
    assert la == engine_i8.lower_fused(lay, entry=True)                        # a pure function of the layer list
    assert fused.launches == engine_i8.lower_fused(lay) == engine_i8.lower_fused(lay, entry=False)       # the default call
    assert [i for l in la for i in l.layers] == list(range(len(lay)))          # every layer once, in order
    # counts and kinds, derived: an 'entry' exactly where the conditions hold, replacing the 'pair' + 'conv' of the fused route
    starts = [i for i in range(len(lay)) if _is_entry(lay, i)]
    assert [l.layers for l in la if l.kind == 'entry'] == [(i, i + 1, i + 2) for i in starts] and len(starts) >= 2
    assert full.int8_launches() == len(la) == len(fused.launches) - len(starts)
    assert plain.int8_launches() == len(lay) and fused.int8_launches() == len(fused.launches)
    # 'full' differs from 'fused' only where an entry block was fused
    expect = []
    for l in fused.launches:
        if l.kind == 'pair' and l.layers[0] in starts:
            expect.append(engine_i8.Launch('entry', l.layers + (l.layers[1] + 1,)))
        elif not (l.kind == 'conv' and l.layers[0] - 2 in starts):
            expect.append(l)
    assert la == expect
    # the first entry launch sits behind the stem and takes its fp16 map: no quantise launch, no int8 copy of the stem map
    assert la[0].kind == 'entry' and lay[0].src == 0 and full.entry_f16 == 0 and plain.entry_f16 is None and fused.entry_f16 is None
    assert ops.entry_i8_fused_supported(1, full.buf_channels[full.stage_in])
    gone = set(lay[l.layers[0]].dst for l in la if l.kind == 'block')
    gone |= set(lay[i].dst for l in la if l.kind == 'entry' for i in l.layers[:2]) | set([0])
    assert full.unwritten == frozenset(gone) and plain.unwritten == frozenset()
    assert fused.unwritten == frozenset(lay[l.layers[0]].dst for l in fused.launches if l.kind == 'block')
    for k, l in enumerate(la):                                  # no launch reads or adds a map that nothing writes
        inside = set(lay[i].dst for i in l.layers)
        outside = set(b for i in l.layers for b in (lay[i].src, lay[i].res) if b is not None and b not in inside)
        assert not (outside & full.unwritten) or (k == full.entry_f16 and outside & full.unwritten == set([0]))
    # tap_ready_after indexes the new launch list: the launch in front of it carries the tap, and no entry launch does
    assert len(full.tap_ready_after) == len(plain.tap_ready_after) == len(full.taps) > 0
    for k, after in enumerate(full.tap_ready_after):
        l = la[after - 1 - len(full.convs)]
        assert full.layers[l.layers[-1]].tap == full.taps[k] and l.kind != 'entry'
    assert full.tap_ready_after[-1] == len(full.convs) + len(la)


def test_launch_counts_of_the_shipped_configurations():
    """(full, fused, layer by layer); the full column follows from the lowering (test_lowering_of_the_full_route): an entry
    launch per untapped 64 -> 64 entry block.  WIDERFACE_LFD_XS has four 64 -> 64 entry blocks, but the last one's conv2 is a
    pyramid tap and keeps 'pair' + 'conv'."""
    got = {}
    for name in ('WIDERFACE_LFD_S', 'WIDERFACE_LFD_XS', 'TT100K_LFD_L'):
        plain, fused, full = _plans(name, 3)
        got[name] = (full.int8_launches(), fused.int8_launches(), plain.int8_launches())
        ents = [i for i, c in enumerate(plain.layers) if c.ks == 1 and (c.cin, c.cout) == (64, 64)]
        tapped = [i for i in ents if plain.layers[i + 2].tap is not None]
        assert got[name][0] == got[name][1] - (len(ents) - len(tapped))
    assert got == {'WIDERFACE_LFD_S': (14, 17, 26), 'WIDERFACE_LFD_XS': (12, 15, 26), 'TT100K_LFD_L': (16, 18, 28)}


@pytest.mark.parametrize('name,ch', CONFIGS, ids=IDS)
def test_layers_names_and_constants_are_the_same_on_the_three_routes(name, ch):
    plain, fused, full = _plans(name, ch)
    amax = dict((k, 0.5 + 0.25 * i) for i, k in enumerate(plain.tensor_names))
    for p in (plain, fused, full):
        p.set_scales(amax)
    for other in (fused, full):
        assert plain.tensor_names == other.tensor_names and len(plain.layers) == len(other.layers)
        assert plain.taps == other.taps and plain.qbuf_channels == other.qbuf_channels and plain.scales == other.scales
        assert plain.inv_stem_scale == other.inv_stem_scale
        for a, b in zip(plain.layers, other.layers):
            assert [getattr(a, s) for s in SLOTS] == [getattr(b, s) for s in SLOTS]
            assert torch.equal(a.w, b.w) and torch.equal(a.q_w, b.q_w) and torch.equal(a.s_w, b.s_w) and torch.equal(a.ref_b, b.ref_b)
            assert torch.equal(a.mult, b.mult) and torch.equal(a.biasq, b.biasq)
            assert (a.res_mult, a.s_in, a.s_out, a.s_res) == (b.res_mult, b.s_in, b.s_out, b.s_res)


def _layer(i, cin, cout, ks, stride, src, res=None, relu=True, tap=None):
    c = engine_i8.ConvI8()
    c.cin, c.cout, c.ks, c.stride, c.relu, c.src, c.dst, c.res, c.tap = cin, cout, ks, stride, relu, src, i + 1, res, tap
    return c


def _entry_block(cin, cout, tap=None, first=0):
    """downsample, conv1, conv2 over buffers first .. first + 3"""
    return [_layer(first, cin, cout, 1, 2, first, relu=False), _layer(first + 1, cin, cout, 3, 2, first),
            _layer(first + 2, cout, cout, 3, 1, first + 2, res=first + 1, tap=tap)]


def test_what_is_not_a_plain_64_channel_entry_block_lowers_as_under_fused():
    kinds = lambda lays, entry: [l.kind for l in engine_i8.lower_fused(lays, entry=entry)]
    assert kinds(_entry_block(64, 64), True) == ['entry'] and kinds(_entry_block(64, 64), False) == ['pair', 'conv']
    for lays in (_entry_block(64, 64, tap=7),                  # a tapped entry block: the entry launch has no fp16 output
                 _entry_block(64, 128), _entry_block(128, 128)):
        assert engine_i8.lower_fused(lays, entry=True) == engine_i8.lower_fused(lays) \
            == [engine_i8.Launch('pair', (0, 1)), engine_i8.Launch('conv', (2,))]
    # a fourth layer that reads the identity map or conv1's map: both must exist, so no entry launch
    for buf in (1, 2):
        lays = _entry_block(64, 64) + [_layer(3, 64, 64, 3, 1, buf)]
        assert kinds(lays, True) == kinds(lays, False) == ['pair', 'conv', 'conv']
    # ... but one that reads the block's output does not matter, and a block behind it is still fused
    lays = _entry_block(64, 64) + [_layer(3, 64, 64, 3, 1, 3), _layer(4, 64, 64, 3, 1, 4, res=3)]
    assert kinds(lays, True) == ['entry', 'block'] and kinds(lays, False) == ['pair', 'conv', 'block']
    assert engine_i8.lower_fused([], entry=True) == []


def test_a_bad_fused_value_raises():
    m = configs.build_model('WIDERFACE_LFD_XS', seed=666)
    m.eval()
    for bad in ('all', 'fused', 2, None, 'Full'):
        with pytest.raises(ValueError):
            engine_i8.Int8Plan(m._backbone, m._neck, m._head, torch.device('cpu'), fused=bad)


def test_supported_query_and_refused_calls_return_status_codes():
    l = _lib.lib()
    for fmt in (-1, 0, 1, 2):
        for ch in (0, 16, 32, 48, 64, 96, 128):
            want = (fmt == 0 and ch == 64) or (fmt == 1 and ch in EC.F16_CHANNELS)
            assert (l.lfd_entry_i8_fused_supported(fmt, ch) == 0) == want == ops.entry_i8_fused_supported(fmt, ch)
            assert l.lfd_entry_i8_fused_supported(fmt, ch) in (0, -4)
    buf = (C.c_char * 4096)()
    base = C.addressof(buf)
    base += -base % 16
    a, b, c_, odd = (C.c_void_p(base + o) for o in (0, 1024, 2048, 1028))

    def entry(n=1, h=4, w=4, fmt=0, ch=64, x=a, w1=b, m1=b, b1=b, wd=b, md=b, bd=b, w2=b, m2=b, b2=b, out=c_):
        return l.lfd_entry_i8_fused(n, h, w, fmt, ch, x, 1.0, w1, m1, b1, wd, md, bd, w2, m2, b2, 0.5, out, None)

    for kw in (dict(x=None), dict(w1=None), dict(m1=None), dict(b1=None), dict(wd=None), dict(md=None), dict(bd=None), dict(w2=None),
               dict(m2=None), dict(b2=None), dict(out=None), dict(x=odd), dict(w1=odd), dict(md=odd), dict(b2=odd), dict(out=odd),
               dict(n=0), dict(h=0), dict(w=-1), dict(out=a), dict(fmt=1, x=odd), dict(fmt=1, out=a)):
        assert entry(**kw) == -1, kw
    for kw in (dict(ch=32), dict(ch=128), dict(fmt=1, ch=16), dict(fmt=1, ch=128), dict(fmt=2), dict(fmt=-1),
               dict(h=4096, w=4096), dict(h=1, w=2 ** 24), dict(fmt=1, ch=32, h=4096, w=4096)):          # h * w * 128 >= 2^31
        assert entry(**kw) == -4, kw
    assert all(v == b'\x00' for v in buf)                       # host memory here: nothing was launched, nothing written
