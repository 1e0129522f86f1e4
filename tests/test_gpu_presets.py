"""LFDResNet's own block / stem / body presets (lfd_resnet.py:222-231; lfd_amd.configs.PRESETS) end to end on the HIP path, in the
'fp16' mode: the 'fast' body ends in 256 and 512 channels, the 'faster' body in 256 -- the layers of csrc/conv_wide.hip.  Each
case is the backbone under SimpleNeck(128) + LFDHead on a 2 x 3 x 128 x 192 batch; the fixtures tests/golden/presets_<case>.npz
hold what the REFERENCE classes compute on the CPU (tests/golden/make_golden_presets.py).

  (a) every conv launch of the backbone plan, and every lateral conv of the neck, re-derived in float64 from the tensors the
      plan stored: |got - ref| <= 0.5005 ulp16(ref) + 2^-19 sum |x||w|, the tolerance of
      tests/test_gpu_parity_fullsize.py::test_every_backbone_launch_rederived_from_the_stored_tensors (launches that round to
      fp16 inside -- a chained 1x1, a fused 64-channel block -- carry its `flips` term);
  (b) sigma(cls) and sigma(reg) against the reference within 2.5e-3, the fp16 mode's stated envelope;
  (c) the tapped backbone maps against the reference's (sampled) maps;
  (d) detect_resident returns the rows of detect(forward(x)); precision='fp32_storage' raises Unsupported on a wide model.
"""
import functools
import os

import numpy as np
import pytest
import torch

import conv_cases as CC
from lfd_amd import configs, engine, engine_sibling

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
SIGMA_GATE = 2.5e-3
WIDE = [k for k, a in configs.PRESETS.items() if max(a['body_channels'] or configs.PRESET_BODY_CHANNELS[a['body_mode']]) > 128]


def _state_sha(sd):
    import hashlib
    h = hashlib.sha256()
    for k in sd:
        h.update(k.encode())
        h.update(sd[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def _case(name):
    """the model on the GPU (weights rebuilt from the seed, checked against the fixture's sha256), the fixture, the input,
    one forward's outputs"""
    gold = np.load(os.path.join(GOLDEN, 'presets_%s.npz' % name))
    m = configs.build_model(configs.PRESETS[name])
    configs.perturb_weights(m)
    assert _state_sha(m.state_dict()) == str(gold['sha']), 'the weights are not the ones the fixture was made with'
    m.eval().cuda()
    x = (torch.from_numpy(gold['x_codes']).float() / 128 - 1).cuda()
    with torch.no_grad():
        cls, reg = m(x)
    torch.cuda.synchronize()
    return dict(model=m, gold=gold, x=x, cls=cls, reg=reg)


def _backbone_plan(m, dev):
    """the plan whose buffers the forward left filled: the model's fused plan, or the backbone plan of the layer engine"""
    if m._fused_plan_ok(dev):
        return engine.get_plan(m, m._backbone, m._neck, m._head, dev), None
    sp = engine_sibling.get_plan(m, m._backbone, m._neck, m._head, dev)
    return sp.bb_plan, sp


def _ulp16(v, floor):
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp(min=floor))) - 10)


@pytest.mark.parametrize('name', list(configs.PRESETS))
def test_every_conv_launch_rederived_from_the_stored_tensors(name):
    cs = _case(name)
    m, x = cs['model'], cs['x']
    dev = x.device
    plan, sp = _backbone_plan(m, dev)
    assert sp is not None, 'every preset taps 32, 256 or 512 channels somewhere: the layer engine runs the neck and the head'
    n, _, h, w = x.shape
    st = plan.state_for(n, h, w)
    worst = []

    def compare(tag, got16, ref, mag, flips=0.0):
        tol = 0.5005 * _ulp16(ref, 2.0 ** -14) + 2.0 ** -19 * mag + flips
        r = float(((got16.double() - ref).abs() / tol).max())
        worst.append((r, tag))
        assert r <= 1.0, (tag, r)

    def w64(t):
        return t.to(dev).half().double()

    nwide = 0
    for c in plan.convs:
        assert c.down is None or not engine._use_fused_down(n, st.bufs[c.src].shape[1], st.bufs[c.src].shape[2])
        assert c.blk128 is None, 'no 128-channel block without branch in these bodies'
        xin = st.bufs[c.src]
        wt, b = w64(c.ref_w), c.b.double()
        ref = CC.conv_ref(xin, wt, b, c.stride)
        mag = CC.conv_ref(xin.abs(), wt.abs(), b.abs(), c.stride)
        flips = 0.0
        second = c.tail[3:0:-2] if c.tail is not None else (c.blk[2:0:-1] if c.blk is not None else None)   # (w2 folded, b2)
        if second is not None:       # chained 1x1 tail / fused FasterBlock: conv -> ReLU -> fp16 -> second conv
            mid = ref.relu().float().half()
            w2, b2 = w64(second[0]), second[1].to(dev).double()
            ref = CC.conv_ref(mid, w2, b2, 1)
            mag = CC.conv_ref(mid.abs(), w2.abs(), b2.abs(), 1)
            flips = 4 * 2.0 ** -11 * float(mid.abs().max()) * float(w2.abs().max())
        if c.res is not None:
            ref = ref + st.bufs[c.res].double()
            mag = mag + st.bufs[c.res].double().abs()
        if c.relu:
            ref = ref.relu()
        nwide += engine.wide_conv(c.cin, c.cout, c.ks, c.stride)
        compare('conv%dx%d s%d %d->%d @%dx%d' % (c.ks, c.ks, c.stride, c.cin, c.cout, ref.shape[1], ref.shape[2]), st.bufs[c.dst], ref, mag,
                flips)
        if c.ds is not None:
            wd, bd = w64(c.ds[3]), c.ds[1].double()
            compare('downsample 1x1 s2 %d->%d' % (c.cin, c.cout), st.bufs[c.ds[2]], CC.conv_ref(xin, wd, bd, 2),
                    CC.conv_ref(xin.abs(), wd.abs(), bd.abs(), 2))
    # ---- the neck's lateral convs (1x1 + folded BatchNorm + ReLU) on the stored taps
    if sp is not None:
        for i, (lat, t) in enumerate(zip(sp.laterals, plan.taps)):
            seq = getattr(m._neck, 'neck%d' % i)
            wt, b = engine._fold_conv_norm(seq[0], seq[1])
            tap = st.bufs[t]
            wp = torch.zeros((128, tap.shape[-1], 1, 1), device=dev)
            wp[:, :wt.shape[1]] = wt
            got = lat(tap)
            ref = CC.conv_ref(tap, w64(wp), b.double(), 1).relu()
            compare('neck 1x1 %d->128' % tap.shape[-1], got, ref, CC.conv_ref(tap.abs(), w64(wp).abs(), b.double().abs(), 1))
            nwide += tap.shape[-1] > 128
    print('LAUNCHES %s: %d checked, %d on the wide kernel, worst error over tolerance %.3f (%s)'
          % ((name, len(worst), nwide) + max(worst)))
    # 256 / 512-channel layers, or (the 'fastest' body) the 64 -> 32 stride-2 layers conv_dispatch routes to the same kernel
    assert nwide >= (4 if name in WIDE else 3)


@pytest.mark.parametrize('name', list(configs.PRESETS))
def test_outputs_and_taps_against_the_reference(name):
    """(b): sigma(cls), sigma(reg) within 2.5e-3 of the reference.  (c): each tapped map within 2^-6 of the reference map's
    largest magnitude -- about twenty layers each round their operands to fp16 (2^-11 relative, twice), a random walk of
    sqrt(40) * 2^-11 = 3e-3 relative in the typical element and a few times that in the worst of 10^4..10^5: 1.6e-2 leaves
    room for that and none for a wrong tap, a wrong channel or a missing residual, which are errors of order one."""
    cs = _case(name)
    m, gold = cs['model'], cs['gold']
    sizes = [tuple(m.head_indexes_to_feature_map_sizes[i]) for i in range(5)]
    assert sizes == [tuple(s) for s in gold['sizes'].tolist()]
    sc = float((cs['cls'].cpu().sigmoid() - torch.from_numpy(gold['cls']).sigmoid()).abs().max())
    sr = float((cs['reg'].cpu().sigmoid() - torch.from_numpy(gold['reg']).sigmoid()).abs().max())
    plan, _ = _backbone_plan(m, cs['x'].device)
    st = plan.state_for(cs['x'].shape[0], cs['x'].shape[2], cs['x'].shape[3])
    rel = []
    for i, t in enumerate(plan.taps):
        s = int(gold['tap_steps'][i])
        ref = torch.from_numpy(gold['tap%d' % i])
        got = st.bufs[t].float().cpu().permute(0, 3, 1, 2)[:, :ref.shape[1], ::s, ::s]
        assert tuple(st.bufs[t].shape[1:3]) == tuple(gold['tap_shapes'][i][2:]) and got.shape == ref.shape
        rel.append(float((got - ref).abs().max() / ref.abs().max()))
        if st.bufs[t].shape[-1] > ref.shape[1]:
            assert not bool(st.bufs[t][..., ref.shape[1]:].any()), 'padded channels stay zero'
    print('PRESET %s: sigma(cls) %.2e sigma(reg) %.2e; taps max |err| / max |ref|: %s' % (name, sc, sr, ' '.join('%.1e' % r for r in rel)))
    assert max(rel) <= 2.0 ** -6
    assert sc <= SIGMA_GATE and sr <= SIGMA_GATE


def test_detect_resident_returns_the_rows_of_detect_of_forward():
    cs = _case('fast_fast_fast')
    m, x = cs['model'], cs['x']
    meta = torch.tensor([[192., 128., 1.0]] * 2, device='cuda')
    with torch.no_grad():
        thr = float(cs['cls'].sigmoid().flatten().kthvalue(cs['cls'].numel() - 150).values)
        want = m.detect(m.forward(x), meta, thr, 0.4)
        wd, wc = want.dets.clone(), want.counts.clone()
        for graph in (False, True):
            m.use_graph = graph
            try:
                out = m.detect_resident(x, meta, score_thr=thr, iou_thr=0.4)
                torch.cuda.synchronize()
            finally:
                m.use_graph = False
            assert torch.equal(out.counts, wc)
            for i in range(2):
                k = int(wc[i, 1])
                assert k > 0 and torch.equal(out.dets[i, :k], wd[i, :k])


def test_fp32_storage_mode_refuses_a_wide_model():
    cs = _case('faster_faster_faster')
    m = cs['model']
    m.precision = 'fp32_storage'
    try:
        with pytest.raises(engine.Unsupported, match="'fp16' mode"):
            with torch.no_grad():
                m(cs['x'])
    finally:
        m.precision = 'fp16'
    with torch.no_grad():
        cls, reg = m(cs['x'])
    assert torch.equal(cls, cs['cls']) and torch.equal(reg, cs['reg'])
