"""The torchvision-style ResNet-18 / 34 backbone end to end on the HIP path ('fp16' mode): configs.RESNET_SIBLINGS -- FCOS over
FPN, LFDv2 over SimpleFPN, LFD over SimpleNeck -- on a 2 x 3 x 128 x 192 batch (R18_FCOS_FPN also on 1 x 3 x 101 x 150) against
what the REFERENCE classes computed on the CPU (tests/golden/resnet_<case>.npz, tests/golden/make_golden_resnet.py).

  (a) every launch of the backbone plan (stem7, pool, every conv with its branch / residual) and every lateral conv of the neck
      re-derived in float64 from the tensors the plan stored: |got - ref| <= 0.5005 ulp16(ref) + 2^-19 sum |x||w| (+ the `flips`
      term of launches that round to fp16 inside), exactly as tests/test_gpu_presets.py; the pool bit for bit;
  (b) each tapped map against the reference's: max |err| / max |ref| <= 4 sqrt(2 L) 2^-11, L the conv layers in front of the tap
      (the random-walk bound tests/test_gpu_presets.py derives: L layers round their operands to fp16 twice, 2^-11 relative each,
      sqrt(2 L) 2^-11 in the typical element and a few times that in the worst of 10^4..10^5; 2^-6 at L = 20);
  (c) sigma(cls), sigma(reg) (sigma(centerness)) against the reference: see SIGMA_MEASURED;
  (d) the entry points agree with each other; (e) what the engine does not cover raises Unsupported; (f) one training step.
"""
import functools
import hashlib
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_cases as CC
import resnet_cases as RC
from lfd_amd import configs, engine, engine_resnet, engine_sibling, netdesc, optim, train

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
CASES = list(configs.RESNET_SIBLINGS)
# sigma(cls) / sigma(reg) / sigma(centerness) against the fixtures as measured on the MI355X (2 x 3 x 128 x 192; the odd shape of
# R18_FCOS_FPN in brackets).  Every case is <= 2.0e-3, so the gate is the fp16 mode's stated 2.5e-3 envelope.
SIGMA_MEASURED = {'R18_FCOS_FPN': (4.30e-4, 4.53e-4, 6.29e-4), 'R18_FCOS_FPN_odd': (4.09e-4, 4.28e-4, 4.77e-4),
                  'R34_LFDV2_SFPN': (4.57e-4, 5.09e-4), 'R18_LFD_SIMPLE': (4.64e-4, 7.05e-4)}
SIGMA_GATE = 2.5e-3
# launches on csrc/conv_wide.hip: per 256 / 512-channel stage its 1x1 branch + two convs per block, + the laterals on those taps
WIDE_LAUNCHES = {'R18_FCOS_FPN': 12, 'R34_LFDV2_SFPN': 22, 'R18_LFD_SIMPLE': 12}


def _state_sha(sd):
    h = hashlib.sha256()
    for k in sd:
        h.update(k.encode())
        h.update(sd[k].detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _frame(gold, suffix=''):
    return (torch.from_numpy(gold['x_codes' + suffix]).float() / 128 - 1).cuda()


@functools.lru_cache(maxsize=None)
def _case(name):
    """the model on the GPU (weights checked against the fixture's sha256), the fixture, the input, one forward's outputs"""
    gold = np.load(os.path.join(GOLDEN, 'resnet_%s.npz' % name))
    m = configs.build_resnet_model(name)
    assert _state_sha(m.state_dict()) == str(gold['sha']), 'the weights are not the ones the fixture was made with'
    m.eval()
    m.cuda()
    x = _frame(gold)
    with torch.no_grad():
        outs = m(x)
    torch.cuda.synchronize()
    return dict(model=m, gold=gold, x=x, outs=outs)


def _plans(m, dev):
    assert not (hasattr(m, '_fused_plan_ok') and m._fused_plan_ok(dev))
    sp = engine_sibling.get_plan(m, m._backbone, m._neck, m._head, dev)
    assert isinstance(sp.bb_plan, engine_resnet.ResNetPlan)
    return sp.bb_plan, sp


@pytest.mark.parametrize('name', CASES)
def test_every_launch_rederived_from_the_stored_tensors(name):
    cs = _case(name)
    m, x = cs['model'], cs['x']
    dev = x.device
    plan, sp = _plans(m, dev)
    n, _, h, w = x.shape
    st = plan.state_for(n, h, w)
    worst = []

    def compare(tag, got16, ref, mag, flips=0.0):
        tol = 0.5005 * RC.ulp16(ref) + 2.0 ** -19 * mag + flips
        r = float(((got16.double() - ref).abs() / tol).max())
        worst.append((r, tag))
        assert r <= 1.0, (tag, r)

    def w64(t):
        return t.to(dev).half().double()

    # ---- stem: conv7x7 s2 + folded BatchNorm + ReLU on the frame, then the pool (bit for bit)
    (_, _, w7, b7), = plan.stem_ref
    xin = x.permute(0, 2, 3, 1)
    ref = RC.conv_ref(xin, w64(w7), b7.double()).relu()
    y = st.bufs[plan.stem_out]
    compare('stem7', y, ref, RC.conv_ref(xin.abs(), w64(w7).abs(), b7.double().abs()))
    pooled = F.max_pool2d(y.permute(0, 3, 1, 2).float(), 3, 2, 1).permute(0, 2, 3, 1).half()
    assert torch.equal(st.bufs[plan.pool_out], pooled), 'max-pool'
    # ---- the stages
    nwide, skip = 0, -1
    for ci, c in enumerate(plan.convs):
        if ci == skip:
            continue
        xin = st.bufs[c.src]
        assert c.down is None or not engine._use_fused_down(n, xin.shape[1], xin.shape[2])
        wt, b = w64(c.ref_w), c.b.double()
        ref = CC.conv_ref(xin, wt, b, c.stride)
        mag = CC.conv_ref(xin.abs(), wt.abs(), b.abs(), c.stride)
        flips, second, last = 0.0, None, c
        assert c.tail is None
        if c.blk is not None:                      # fused 64-channel block: conv -> ReLU -> fp16 -> second conv
            second = (c.blk[2], c.blk[1])
        elif c.blk128 is not None and engine._use_fused_block128(n, xin.shape[1], xin.shape[2]):
            last = plan.convs[c.blk128]            # 128-channel block without branch in one launch, the same roundings
            second, skip = (last.ref_w, last.b), c.blk128
        if second is not None:
            mid = ref.relu().float().half()
            w2, b2 = w64(second[0]), second[1].to(dev).double()
            ref = CC.conv_ref(mid, w2, b2, 1)
            mag = CC.conv_ref(mid.abs(), w2.abs(), b2.abs(), 1)
            flips = 4 * 2.0 ** -11 * float(mid.abs().max()) * float(w2.abs().max())
        if last.res is not None:
            ref = ref + st.bufs[last.res].double()
            mag = mag + st.bufs[last.res].double().abs()
        if last.relu:
            ref = ref.relu()
        nwide += engine.wide_conv(c.cin, c.cout, c.ks, c.stride)
        compare('conv%dx%d s%d %d->%d @%dx%d' % (c.ks, c.ks, c.stride, c.cin, c.cout, ref.shape[1], ref.shape[2]), st.bufs[last.dst],
                ref, mag, flips)
        if c.ds is not None:
            wd, bd = w64(c.ds[3]), c.ds[1].double()
            compare('downsample 1x1 s2 %d->%d' % (c.cin, c.cout), st.bufs[c.ds[2]], CC.conv_ref(xin, wd, bd, 2),
                    CC.conv_ref(xin.abs(), wd.abs(), bd.abs(), 2))
    # ---- the neck's lateral convs on the stored taps
    prefix = 'neck%d' if sp.neck_kind == 'SimpleNeck' else 'lateral%d'
    for i, (lat, t) in enumerate(zip(sp.laterals, plan.taps)):
        layer, = netdesc.split_sequential(getattr(m._neck, prefix % i))
        wt, b = engine._fold_conv_norm(layer.conv, layer.norm)
        tap = st.bufs[t]
        assert tap.shape[-1] == wt.shape[1] and lat.cout == wt.shape[0], 'no padded channels in these models'
        ref = CC.conv_ref(tap, w64(wt), b.double(), 1)
        compare('lateral 1x1 %d->%d' % (tap.shape[-1], lat.cout), lat(tap), ref.relu() if layer.relu else ref,
                CC.conv_ref(tap.abs(), w64(wt).abs(), b.double().abs(), 1))
        nwide += tap.shape[-1] > 128
    print('LAUNCHES %s: %d checked, %d on the wide kernel, worst error over tolerance %.3f (%s)'
          % ((name, len(worst), nwide) + max(worst)))
    assert nwide >= WIDE_LAUNCHES[name]


def _tap_layers(bb):
    """conv layers on the main path in front of each tap: the stem conv + two per block"""
    out, nconv = [], 1
    for blk in netdesc.resnet_layers(bb).blocks:
        nconv += len(blk.convs)
        if blk.tap:
            out.append(nconv)
    return out


def _sigma_errors(outs, gold, suffix=''):
    return [float((o.cpu().sigmoid() - torch.from_numpy(gold[k + suffix]).sigmoid()).abs().max())
            for o, k in zip(outs, ('cls', 'reg', 'ctr'))]


@pytest.mark.parametrize('name,suffix', [(n, '') for n in CASES] + [('R18_FCOS_FPN', '_odd')])
def test_outputs_and_taps_against_the_reference(name, suffix):
    cs = _case(name)
    m, gold = cs['model'], cs['gold']
    if suffix:
        x = _frame(gold, suffix)
        with torch.no_grad():
            outs = m(x)
    else:
        x, outs = cs['x'], cs['outs']
    nl = len(gold['sizes' + suffix])
    assert [tuple(m.head_indexes_to_feature_map_sizes[i]) for i in range(nl)] == [tuple(s) for s in gold['sizes' + suffix].tolist()]
    assert [tuple(o.shape) for o in outs] == [tuple(gold[k + suffix].shape) for k in ('cls', 'reg', 'ctr')[:len(outs)]]
    plan, _ = _plans(m, x.device)
    st = plan.state_for(x.shape[0], x.shape[2], x.shape[3])
    rel, bounds = [], []
    for i, (t, nconv) in enumerate(zip(plan.taps, _tap_layers(m._backbone))):
        s = int(gold['tap_steps' + suffix][i])
        ref = torch.from_numpy(gold['tap%d%s' % (i, suffix)])
        got = st.bufs[t].float().cpu().permute(0, 3, 1, 2)[:, :ref.shape[1], ::s, ::s]
        assert tuple(st.bufs[t].shape[1:3]) == tuple(gold['tap_shapes' + suffix][i][2:]) and got.shape == ref.shape
        rel.append(float((got - ref).abs().max() / ref.abs().max()))
        bounds.append(4 * math.sqrt(2 * nconv) * 2.0 ** -11)
        assert not bool(st.bufs[t][..., ref.shape[1]:].any()), 'padded channels stay zero'
    sig = _sigma_errors(outs, gold, suffix)
    print('RESNET %s%s: sigma(cls, reg[, ctr]) %s; taps max |err| / max |ref|: %s (bounds %s)'
          % (name, suffix, ' '.join('%.2e' % v for v in sig), ' '.join('%.1e' % r for r in rel), ' '.join('%.1e' % b for b in bounds)))
    assert all(r <= b for r, b in zip(rel, bounds))
    assert max(sig) <= SIGMA_GATE


@pytest.mark.parametrize('name', CASES)
def test_frame_formats_and_graph_replay_agree(name):
    cs = _case(name)
    m, x, outs = cs['model'], cs['x'], cs['outs']
    with torch.no_grad():
        # the frame's values are fp16 numbers: the fp16 NHWC frame is the same operand
        x16 = x.permute(0, 2, 3, 1).half().contiguous()
        assert all(torch.equal(a, b) for a, b in zip(m(x16), outs))
        # uint8: normalised on the load -- compared with its own normalised fp16 twin
        codes = torch.from_numpy(cs['gold']['x_codes']).permute(0, 2, 3, 1).contiguous().cuda()
        twin = RC.normalize_u8(codes.cpu()).cuda()
        assert all(torch.equal(a, b) for a, b in zip(m(codes), m(twin)))
        m.use_graph = True
        try:
            first = [t.clone() for t in m(x)]
            again = [t.clone() for t in m(x)]          # the second call replays
        finally:
            m.use_graph = False
    assert all(torch.equal(a, b) and torch.equal(a, c) for a, b, c in zip(outs, first, again))


@pytest.mark.parametrize('name', ['R18_LFD_SIMPLE', 'R34_LFDV2_SFPN'])
def test_detect_resident_returns_the_rows_of_detect_of_forward(name):
    cs = _case(name)
    m, x = cs['model'], cs['x']
    meta = torch.tensor([[192., 128., 1.0]] * 2, device='cuda')
    with torch.no_grad():
        sc = cs['outs'][0].sigmoid().flatten()
        thr = float(sc.kthvalue(max(sc.numel() - 150, 1)).values)
        want = m.detect(m.forward(x), meta, thr, 0.4)
        wd, wc = want.dets.clone(), want.counts.clone()
        res = m.forward_resident(x)
        assert all(torch.equal(a, b) for a, b in zip(res, cs['outs']))
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


@pytest.mark.parametrize('name', CASES)
def test_get_results_runs(name):
    cs = _case(name)
    m, outs = cs['model'], cs['outs']
    old = m._classification_threshold
    sc = outs[0].sigmoid() * outs[2].sigmoid() if len(outs) == 3 else outs[0].sigmoid()
    m._classification_threshold = float(np.quantile(sc.cpu().numpy(), 0.9))
    try:
        res = m.get_results(outs, [dict(resized_height=128, resized_width=192, resize_scale=1.0)] * 2)
    finally:
        m._classification_threshold = old
    assert len(res) == 2 and all(len(r) > 0 and len(r[0]) == 6 for r in res)


def test_predict_for_single_image_runs():
    cs = _case('R18_LFD_SIMPLE')
    m = cs['model']
    image = cs['x'][0].permute(1, 2, 0).cpu().numpy()
    thr = float(np.quantile(cs['outs'][0][0].sigmoid().cpu().numpy(), 0.9))
    rows = m.predict_for_single_image(image, lambda sample: sample, classification_threshold=thr)
    assert len(rows) > 0 and len(rows[0]) == 6


def test_fp32_storage_mode_is_refused_and_fp16_keeps_its_bits():
    for name in ('R18_LFD_SIMPLE', 'R18_FCOS_FPN'):
        cs = _case(name)
        m = cs['model']
        m.precision = 'fp32_storage'
        try:
            with pytest.raises(engine.Unsupported, match='fp32-tensor kernel'):
                with torch.no_grad():
                    m(cs['x'])
        finally:
            m.precision = 'fp16'
        with torch.no_grad():
            outs = m(cs['x'])
        assert all(torch.equal(a, b) for a, b in zip(outs, cs['outs']))


@pytest.mark.parametrize('kw,word', [(dict(depth=50), 'depth=50'), (dict(deep_stem=True), 'deep_stem')])
def test_uncovered_backbones_raise_unsupported_naming_the_option(kw, word):
    m = configs.build_resnet_model('R18_FCOS_FPN', **kw)
    m.eval()
    m.cuda()
    x = torch.zeros(1, 3, 64, 64, device='cuda')
    with pytest.raises(engine.Unsupported, match=word):
        with torch.no_grad():
            m(x)


def test_one_training_step_under_autograd():
    """backbone, neck and head under PyTorch-ROCm autograd, targets and loss on the device as for every sibling; frozen_stages=1
    and the default norm_eval=True are respected"""
    m = configs.build_resnet_model('R18_FCOS_FPN', frozen_stages=1)
    m.cuda()
    m.train()
    bb = m._backbone
    frozen = {id(p) for mod in (bb.conv1, bb.bn1, bb.layer1) for p in mod.parameters()}
    assert all(p.requires_grad == (id(p) not in frozen) for p in m.parameters())
    assert not any(mod.training for mod in bb.modules() if isinstance(mod, torch.nn.BatchNorm2d)) and not bb.layer1[0].training
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    opt = optim.SGD(m.parameters(), lr=0.01, momentum=0.9, weight_decay=1e-4)
    x = torch.randn(2, 3, 128, 192, generator=torch.Generator().manual_seed(1)).cuda()
    ann = [(np.array([[10., 12., 60., 40.], [100., 20., 50., 84.]], np.float32), np.array([0, 2], np.int64)),
           (np.array([[40., 30., 24., 20.], [90., 50., 90., 70.]], np.float32), np.array([1, 0], np.int64))]
    values, _ = train.train_step(m, opt, x, ann)
    assert all(math.isfinite(float(v)) for v in values.values()) and float(values['loss']) > 0
    trainable = [(k, p) for k, p in m.named_parameters() if p.requires_grad]
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for _, p in trainable)
    # a Scale of a level without a positive point may see a zero gradient; everything else was reached by the loss
    assert all(bool(p.grad.ne(0).any()) for k, p in trainable if '_scale' not in k)
    after = m.state_dict()
    for k, p in m.named_parameters():
        if id(p) in frozen:
            assert p.grad is None and torch.equal(after[k], before[k]), k
    for k in after:        # eval-mode BatchNorm: the running statistics of the backbone did not move
        if k.startswith('_backbone.') and ('running_' in k or 'num_batches' in k):
            assert torch.equal(after[k], before[k]), k
