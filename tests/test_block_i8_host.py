"""Host side of the fused int8 launches (csrc/block_i8.hip, csrc/conv_i8.hip, the fused=True route of lfd_amd/engine_i8.py): the reference of
tests/golden/block_i8_cases.py against a plain int64 conv chain, what the shape tables claim, the lowering of the layer list into
launches, and the status codes of refused calls.  No GPU: a refused call returns before any launch."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import block_i8_cases as BC
import conv_i8_cases as QC
from lfd_amd import _lib, configs, engine_i8, ops

# int8 launches of the stages per forward (the quantise launch not counted): fused, layer by layer
LAUNCHES = {'WIDERFACE_LFD_S': (17, 26), 'WIDERFACE_LFD_XS': (15, 26), 'TT100K_LFD_L': (18, 28)}


def _conv_i64(x, w, stride):
    """NHWC int8 x, OIHW int8 w -> NHWC int64, zero padding ks // 2"""
    return F.conv2d(x.permute(0, 3, 1, 2).long(), w.long(), stride=stride, padding=w.shape[2] // 2).permute(0, 2, 3, 1)


def _requant(v):
    return torch.round(v).clamp(-127, 127).to(torch.int8)


@pytest.mark.parametrize('shape', [(1, 1, 1), (2, 3, 5), (1, 9, 17)])
@pytest.mark.parametrize('big_bias', [False, True])
def test_block_reference_is_a_plain_int64_conv_chain(shape, big_bias):
    c = BC.BlockCase('tiny', *shape)
    x, w1, w2 = BC.block_operands(c)
    k1, k2 = BC.block_exact_constants(c, big_bias)
    mid, v, q, f = BC.block_ref(x, w1, w2, k1, k2)
    a1 = _conv_i64(x, w1, 1)
    mid2 = _requant((a1.double() * k1.mult.double() + k1.biasq.double()).clamp(min=0))
    assert torch.equal(mid, mid2)
    a2 = _conv_i64(mid2, w2, 1)                                # F.conv2d pads the MID map with zeros: conv2's padding rule
    v2 = (a2.double() * k2.mult.double() + k2.biasq.double() + x.double() * k2.res_mult).clamp(min=0)
    assert torch.equal(v, v2) and torch.equal(q, _requant(v2)) and torch.equal(f, v2 * k2.out_scale)
    assert torch.equal(v.float().double(), v)                  # the instrument: exact in fp32
    if big_bias:
        # the padding rule is observable: conv1 evaluated on the all-zero input outside the image would be BIG_BIAS, and conv2
        # of a mid map padded with it differs from the reference
        midp = F.pad(mid2.permute(0, 3, 1, 2).long(), (1, 1, 1, 1), value=int(BC.BIG_BIAS))
        a2w = F.conv2d(midp, w2.long()).permute(0, 2, 3, 1)
        assert not torch.equal(a2w, a2)


@pytest.mark.parametrize('c', [BC.PairCase(64, 64, 'tiny', 1, 1, 1), BC.PairCase(64, 128, 'tiny', 2, 4, 7),
                               BC.PairCase(128, 128, 'tiny', 1, 5, 6)], ids=BC.pair_id)
def test_pair_reference_is_two_plain_int64_convs(c):
    x, w3, wd = BC.pair_operands(c)
    k3, kd = BC.pair_exact_constants(c)
    v3, q3, vd, qd = BC.pair_ref(x, w3, wd, k3, kd)
    assert tuple(q3.shape) == tuple(qd.shape) == (c.n,) + BC.pair_out_hw(c.h, c.w) + (c.cout,)
    r3 = (_conv_i64(x, w3, 2).double() * k3.mult.double() + k3.biasq.double()).clamp(min=0)
    rd = _conv_i64(x, wd, 2).double() * kd.mult.double() + kd.biasq.double()
    assert torch.equal(v3, r3) and torch.equal(q3, _requant(r3)) and torch.equal(vd, rd) and torch.equal(qd, _requant(rd))
    assert bool((vd < 0).any())                                # the identity branch has no ReLU


def test_shape_tables_hold_what_they_claim():
    kinds = dict((c.kind, c) for c in BC.block_cases())
    assert (kinds['pixel'].n, kinds['pixel'].h, kinds['pixel'].w) == (1, 1, 1)
    assert BC.block_launch(kinds['edge'])[:2] == (2, 2) and (kinds['edge'].h, kinds['edge'].w) == (BC.TH + 1, BC.TW + 1)
    assert kinds['general'].h % BC.TH and kinds['general'].w % BC.TW and BC.block_launch(kinds['general'])[2] > 1
    tx, ty, nt, grid = BC.block_launch(kinds['walk'])
    assert (tx, ty) == (3, 2) and grid == BC.MAX_WORKGROUPS < nt and abs(nt / grid - 1.5) < 0.01
    assert BC.MAX_WORKGROUPS // (tx * ty) >= 1 and BC.MAX_WORKGROUPS % (tx * ty) != 0     # the second tile: another image, another place
    for key in BC.PAIR_KEYS:
        ks = dict((c.kind, c) for c in BC.pair_cases() if (c.cin, c.cout) == key)
        assert sorted(ks) == ['edge_even', 'edge_odd', 'general', 'pixel', 'walk']
        assert BC.pair_out_hw(ks['edge_odd'].h, ks['edge_odd'].w) == BC.pair_out_hw(ks['edge_even'].h, ks['edge_even'].w) == (5, 17)
        assert ks['edge_odd'].h % 2 == 1 and ks['edge_even'].h % 2 == 0 and ks['general'].h % 2 == 1 and ks['general'].w % 2 == 1
        tx, ty, nt, grid = BC.pair_launch(ks['walk'])
        assert (tx, ty) == (3, 2) and grid == BC.PAIR_MAX_WORKGROUPS < nt and abs(nt / grid - 1.5) < 0.01
        assert BC.PAIR_MAX_WORKGROUPS % (tx * ty) != 0
    assert tuple(BC.PAIR_KEYS) == tuple(engine_i8.PAIR_KEYS)


def _plans(name):
    m = configs.build_model(name, seed=666)
    m.eval()
    args = (m._backbone, m._neck, m._head, torch.device('cpu'))
    return engine_i8.Int8Plan(*args), engine_i8.Int8Plan(*args, fused=True)


@pytest.mark.parametrize('name', sorted(LAUNCHES))
def test_lowering_gives_the_launch_lists_of_the_shipped_configurations(name):
    plain, fused = _plans(name)
    n_fused, n_plain = LAUNCHES[name]
    assert not plain.fused and plain.launches is None and plain.int8_launches() == len(plain.layers) == n_plain
    assert fused.fused and fused.int8_launches() == len(fused.launches) == n_fused
    la = engine_i8.lower_fused(plain.layers)                    # a pure function of the layer list
    assert la == fused.launches
    assert [i for l in la for i in l.layers] == list(range(len(plain.layers)))        # every layer once, in order
    lay = plain.layers
    for l in la:
        cs = [lay[i] for i in l.layers]
        if l.kind == 'pair':
            d, c1 = cs
            assert (d.ks, d.stride, d.relu, c1.ks, c1.stride, c1.relu) == (1, 2, False, 3, 2, True) and d.src == c1.src
            nxt = lay[l.layers[1] + 1]                          # conv2 follows as a single launch with res = ds_out
            assert (nxt.src, nxt.res) == (c1.dst, d.dst) and engine_i8.Launch('conv', (l.layers[1] + 1,)) in la
        elif l.kind == 'block':
            c1, c2 = cs
            assert c1.cin == c1.cout == c2.cin == c2.cout == 64 and (c1.ks, c1.stride, c2.ks, c2.stride) == (3, 1, 3, 1)
            assert c2.src == c1.dst and c2.res == c1.src and c1.tap is None
        else:
            assert l.kind == 'conv' and len(cs) == 1
    # 128-channel blocks stay layer by layer; every 64-channel block without a downsample is fused
    in_block = set(i for l in la if l.kind == 'block' for i in l.layers)
    for i, c in enumerate(lay):
        if c.ks == 3 and c.stride == 1 and c.cin == c.cout == 128:
            assert i not in in_block
    for i, c in enumerate(lay):
        if (c.ks, c.stride, c.cin, c.cout) == (3, 1, 64, 64):   # ... or it is the conv2 of an entry block
            assert i in in_block or (c.res is not None and lay[i - 2].ks == 1 and lay[i - 2].dst == c.res)
    ents = [c for c in lay if c.ks == 1]
    assert [l.kind for l in la].count('pair') == len(ents) > 0
    # the map between a fused block's convs has no buffer; everything else has
    assert fused.unwritten == frozenset(lay[l.layers[0]].dst for l in la if l.kind == 'block') and plain.unwritten == frozenset()
    # tap_ready_after indexes the fused launch list: the launch in front of it carries the tap
    assert len(fused.tap_ready_after) == len(plain.tap_ready_after) == len(fused.taps)
    for k, after in enumerate(fused.tap_ready_after):
        last = fused.layers[la[after - 1 - len(fused.convs)].layers[-1]]
        assert last.tap == fused.taps[k]
    assert fused.tap_ready_after[-1] == len(fused.convs) + n_fused and plain.tap_ready_after[-1] == len(plain.convs) + n_plain


@pytest.mark.parametrize('name', sorted(LAUNCHES) + ['TL_LFD_S'])
def test_layers_names_and_constants_are_the_same_with_and_without_fused(name):
    plain, fused = _plans(name)
    assert plain.tensor_names == fused.tensor_names
    slots = ['name', 'cin', 'cout', 'cout_real', 'ks', 'stride', 'relu', 'src', 'dst', 'res', 'tap', 'src_name', 'res_name']
    for a, b in zip(plain.layers, fused.layers):
        assert [getattr(a, s) for s in slots] == [getattr(b, s) for s in slots]
        assert torch.equal(a.w, b.w) and torch.equal(a.q_w, b.q_w) and torch.equal(a.s_w, b.s_w) and torch.equal(a.ref_b, b.ref_b)
    assert len(plain.layers) == len(fused.layers) and plain.taps == fused.taps and plain.qbuf_channels == fused.qbuf_channels
    amax = dict((k, 0.5 + 0.25 * i) for i, k in enumerate(plain.tensor_names))
    plain.set_scales(amax)
    fused.set_scales(amax)
    assert plain.scales == fused.scales
    for a, b in zip(plain.layers, fused.layers):
        assert torch.equal(a.mult, b.mult) and torch.equal(a.biasq, b.biasq)
        assert (a.res_mult, a.s_in, a.s_out, a.s_res) == (b.res_mult, b.s_in, b.s_out, b.s_res)


def test_a_layer_list_with_nothing_to_fuse_lowers_to_itself():
    L = engine_i8.ConvI8

    def layer(i, cin, cout, ks, stride, src, res=None):
        c = L()
        c.cin, c.cout, c.ks, c.stride, c.relu, c.src, c.dst, c.res, c.tap = cin, cout, ks, stride, True, src, i + 1, res, None
        return c

    lays = [layer(0, 128, 128, 3, 1, 0), layer(1, 128, 128, 3, 1, 1, res=0)]
    assert engine_i8.lower_fused(lays) == [engine_i8.Launch('conv', (0,)), engine_i8.Launch('conv', (1,))]
    assert engine_i8.lower_fused([]) == []
    # a block whose mid map is read by a third layer is not fused
    lays = [layer(0, 64, 64, 3, 1, 0), layer(1, 64, 64, 3, 1, 1, res=0), layer(2, 64, 64, 3, 1, 1)]
    assert [l.kind for l in engine_i8.lower_fused(lays)] == ['conv', 'conv', 'conv']
    assert [l.kind for l in engine_i8.lower_fused(lays[:2])] == ['block']


def test_supported_query_and_refused_calls_return_status_codes():
    l = _lib.lib()
    for cin in (32, 64, 128, 256):
        for cout in (32, 64, 128, 256):
            want = (cin, cout) in BC.PAIR_KEYS
            assert (l.lfd_conv2d_downsample_nhwc_i8_supported(cin, cout) == 0) == want == ops.conv2d_downsample_i8_supported(cin, cout)
            assert l.lfd_conv2d_downsample_nhwc_i8_supported(cin, cout) in (0, -4)
    buf = (C.c_char * 4096)()
    base = C.addressof(buf)
    base += -base % 16
    a, b, c_, odd = (C.c_void_p(base + o) for o in (0, 1024, 2048, 1028))

    def block(n=1, h=4, w=4, x=a, w1=b, m1=b, b1=b, w2=b, m2=b, b2=b, out=c_, f=None):
        return l.lfd_block_i8_fused(n, h, w, x, w1, m1, b1, w2, m2, b2, 0.5, out, f, 1.0, None)

    for kw in (dict(x=None), dict(w1=None), dict(m1=None), dict(b1=None), dict(w2=None), dict(m2=None), dict(b2=None), dict(out=None),
               dict(x=odd), dict(w1=odd), dict(m2=odd), dict(out=odd), dict(f=odd), dict(n=0), dict(h=0), dict(w=-1), dict(out=a)):
        assert block(**kw) == -1, kw
    assert block(h=4096, w=4096) == -4 and block(h=1, w=2 ** 24) == -4          # h * w * 128 >= 2^31

    def pair(n=1, h=4, w=4, cin=64, cout=64, x=a, w3=b, m=b, bq=b, wd=b, md=b, bd=b, out=c_, ds=C.c_void_p(base + 3072)):
        return l.lfd_conv2d_downsample_nhwc_i8(n, h, w, cin, cout, x, w3, m, bq, wd, md, bd, out, ds, None)

    for kw in (dict(x=None), dict(w3=None), dict(m=None), dict(bq=None), dict(wd=None), dict(md=None), dict(bd=None), dict(out=None),
               dict(ds=None), dict(x=odd), dict(wd=odd), dict(ds=odd), dict(n=0), dict(h=0), dict(w=0), dict(out=a), dict(ds=a), dict(ds=c_)):
        assert pair(**kw) == -1, kw
    for key in ((32, 64), (128, 64), (64, 256), (256, 256)):
        assert pair(cin=key[0], cout=key[1]) == -4
    assert pair(h=4096, w=4096) == -4
    assert all(v == b'\x00' for v in buf)                       # host memory here: nothing was launched, nothing written
