"""The INT8 deployment mode end to end on the MI355X (lfd_amd/deployment.py, lfd_amd/engine_i8.py): every int8 launch of
a forward re-derived from the tensors the plan stored, the quantise step, the logits against the reference's fp32 fixture, graph
replay, frame formats, post-processing, the calibration cache, and the refusal after a parameter change.

Weights and frames are those of tests/golden/ref_model_<ARCH>.npz (sha checked); the calibration set is the fixture's frames plus
four seeded frames of the same size, one frame per batch."""
import functools
import os
import tempfile

import numpy as np
import pytest
import torch

import conv_i8_cases as QC
from conftest import load_golden
from lfd_amd import INT8Calibrator, build_int8_engine, configs, deployment, engine_i8, ops

pytestmark = pytest.mark.gpu

CASES = [('WIDERFACE_LFD_S', 3), ('WIDERFACE_LFD_XS', 3), ('TT100K_LFD_L', 3), ('WIDERFACE_LFD_S', 1)]
IDS = ['%s%s' % (n, '_gray' if c == 1 else '') for n, c in CASES]

# max |sigmoid(out) - sigmoid(reference fp32)| over (cls, reg) of the fixture frames, measured on the MI355X with the calibration
# set above (the fp16 mode on the same frames: see DESIGN 4j); the gate is 1.5 x the measured value, the margin for which
# near-tie outputs round which way from run to run -- not to be widened
INT8_SIGMA_MEASURED = {
    'WIDERFACE_LFD_S': 3.425e-2,         # cls 3.425e-2, reg 2.909e-2; fp16 mode 7.8e-4 / 1.0e-3
    'WIDERFACE_LFD_XS': 3.536e-2,        # cls 3.536e-2, reg 2.837e-2; fp16 mode 1.2e-3 / 1.3e-3
    'TT100K_LFD_L': 5.935e-2,            # cls 5.935e-2, reg 4.410e-2; fp16 mode 1.5e-3 / 9.4e-4
    'WIDERFACE_LFD_S_gray': 2.235e-2,    # cls 1.788e-2, reg 2.235e-2; fp16 mode 6.3e-4 / 8.2e-4
}


def _frames(g, ch):
    n, h, w = [int(v) for v in g['shape']]
    return torch.rand(n, ch, h, w, generator=torch.Generator().manual_seed(int(g['x_seed']))) * 2 - 1


@functools.lru_cache(maxsize=None)
def _case(name, ch):
    g = load_golden(('ref_model_gray_%s.npz' if ch == 1 else 'ref_model_%s.npz') % name)
    m = configs.build_model(name, seed=666, input_channels=ch)
    configs.perturb_weights(m, seed=1)
    m.eval()
    assert deployment.state_sha256(m.state_dict()) == str(g['sha'])
    x = _frames(g, ch)
    extra = torch.rand(4, ch, x.shape[2], x.shape[3], generator=torch.Generator().manual_seed(1234)) * 2 - 1
    m.cuda()
    cache = os.path.join(tempfile.mkdtemp(prefix='lfd_int8_'), 'calibration.json')
    data = torch.cat([x, extra]).numpy()
    eng = build_int8_engine(m, INT8Calibrator(data, cache, batch_size=1))
    assert eng.calibrated and os.path.exists(cache)
    xc = x.cuda()
    with torch.no_grad():
        cls, reg = eng(xc)
    return dict(g=g, m=m, x=xc, eng=eng, cache=cache, data=data, cls=cls, reg=reg)


def _sigma_errors(outs, gold):
    return [float((o.cpu().sigmoid() - torch.from_numpy(gold[k]).sigmoid()).abs().max()) for o, k in zip(outs, ('cls', 'reg'))]


# TL_LFD_S: a 48-channel stem and first stage, run zero-padded to 64
@pytest.mark.parametrize('name,ch', CASES + [('TL_LFD_S', 3)], ids=IDS + ['TL_LFD_S'])
def test_every_int8_launch_rederived(name, ch):
    cs = _case(name, ch)
    eng, x = cs['eng'], cs['x']
    plan = eng.plan
    with torch.no_grad():
        eng.forward_resident(x)
    torch.cuda.synchronize()
    st = plan.state_for(x.shape[0], x.shape[2], x.shape[3], 0)
    assert len(plan.layers) == sum(len(b.convs) + (b.downsample is not None) for b in engine_i8.netdesc.backbone_layers(cs['m']._backbone).blocks)
    worst = 0.0
    for c in plan.layers:
        # the constants from the contract, from the scales and the folded weights the plan stored
        s_w, q_w = engine_i8.weight_scales(c.ref_w)
        assert torch.equal(ops.unpack_conv_weight_i8(c.w, c.cin, c.ks), q_w.to(c.w.device))
        s_in, s_out = eng.scales[c.src_name][1], eng.scales[c.name][1]
        assert (c.s_in, c.s_out) == (s_in, s_out) and s_out == (eng.scales[c.name][0] / 127 if eng.scales[c.name][0] > 0 else 1.0)
        assert torch.equal(c.mult.cpu(), (s_w.double().cpu() * s_in / s_out).float())
        assert torch.equal(c.biasq.cpu(), (c.ref_b.double().cpu() / s_out).float())
        res = st.qbufs[c.res] if c.res is not None else None
        if res is not None:
            assert c.res_mult == float(torch.tensor(eng.scales[c.res_name][1] / s_out, dtype=torch.float64).float())
        # the launch, from its actual int8 input buffer
        acc = QC.acc_ref(st.qbufs[c.src], q_w.cuda(), c.stride)
        k = QC.Consts(c.mult, c.biasq, c.res_mult, c.s_out)
        v, q_ref, f_ref = QC.epilogue_ref(acc, k, res, c.relu)
        tie = QC.near_tie(v)
        share = float(tie.double().mean())
        worst = max(worst, share)
        diff = (st.qbufs[c.dst].int() - q_ref.int()).abs()
        assert share <= QC.NEAR_TIE_CAP, (c.name, share)
        assert int(diff[~tie].max()) == 0 and int(diff.max()) <= 1, c.name
        if c.tap is not None:
            err = (st.bufs[c.tap].double() - f_ref).abs()
            assert bool((err <= QC.f16_ulp(f_ref)).all()), c.name
        # padded channels stay zero
        assert bool((st.qbufs[c.dst][..., c.cout_real:] == 0).all()), c.name
        if c.tap is not None:
            assert bool((st.bufs[c.tap][..., c.cout_real:] == 0).all()), c.name
    assert [c.tap is not None for c in plan.layers].count(True) == len(plan.taps)
    print('%s: %d int8 launches, largest near-tie share %.4f' % (name, len(plan.layers), worst))


@pytest.mark.parametrize('name,ch', CASES[:2] + [('TL_LFD_S', 3)], ids=IDS[:2] + ['TL_LFD_S'])
def test_quantise_launch_and_padded_channels(name, ch):
    cs = _case(name, ch)
    eng, x = cs['eng'], cs['x']
    plan = eng.plan
    with torch.no_grad():
        eng.forward_resident(x)
    torch.cuda.synchronize()
    st = plan.state_for(x.shape[0], x.shape[2], x.shape[3], 0)
    stem = st.bufs[plan.stage_in]
    inv = torch.tensor(1.0 / eng.scales['stem'][1], dtype=torch.float64).float()
    ref = torch.round(stem.float() * inv.cuda()).clamp(-127, 127).to(torch.int8)
    c = stem.shape[3]
    assert torch.equal(st.qbufs[0][..., :c], ref)
    assert 64 <= int(ref.abs().max()) <= 127              # amax is over the whole calibration set, these frames among them
    bb = cs['m']._backbone
    stem_real = [m_ for m_ in bb._stem if isinstance(m_, torch.nn.Conv2d)][-1].out_channels
    assert bool((st.qbufs[0][..., stem_real:] == 0).all())
    if name == 'WIDERFACE_LFD_XS':
        assert (c, stem_real, st.qbufs[0].shape[3]) == (32, 32, 64)      # 32 stem channels in front of stages padded to 64
        first = plan.layers[0]
        assert bool((first.q_w[:, 32:] == 0).all()) and bool((plan.layers[1].q_w[:, 32:] == 0).all())


@pytest.mark.parametrize('name,ch', CASES, ids=IDS)
def test_logits_against_the_reference_fp32_fixture(name, ch):
    cs = _case(name, ch)
    g, m = cs['g'], cs['m']
    key = name + ('_gray' if ch == 1 else '')
    assert cs['cls'].dtype == torch.float32 and cs['cls'].shape == g['cls'].shape and cs['reg'].shape == g['reg'].shape
    assert [list(m.head_indexes_to_feature_map_sizes[i]) for i in range(len(g['sizes']))] == g['sizes'].tolist()
    e8 = _sigma_errors((cs['cls'], cs['reg']), g)
    with torch.no_grad():
        e16 = _sigma_errors(m(cs['x']), g)
    print('%s: max |sigma(out) - sigma(ref)| cls / reg: int8 %.3e / %.3e, fp16 mode %.3e / %.3e' % (key, e8[0], e8[1], e16[0], e16[1]))
    assert INT8_SIGMA_MEASURED[key] is not None, 'no measured value recorded'
    assert max(e8) <= 1.5 * INT8_SIGMA_MEASURED[key]


def test_eager_and_graph_are_bit_equal_and_outputs_are_fresh():
    cs = _case(*CASES[0])
    eng, x = cs['eng'], cs['x']
    with torch.no_grad():
        a = eng(x)
        eng.use_graph = True
        try:
            b = eng(x)
            c = eng(x)                                                   # a replay
        finally:
            eng.use_graph = False
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(b[0], c[0]) and torch.equal(b[1], c[1])
    assert torch.equal(a[0], cs['cls']) and a[0].data_ptr() != b[0].data_ptr()


def test_frame_formats_agree_as_in_the_fp16_mode():
    cs = _case('WIDERFACE_LFD_XS', 3)
    eng = cs['eng']
    img = torch.randint(0, 256, (1, 120, 168, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0))
    xf = ((img.float() / 255 - 0.5) / 0.5)
    with torch.no_grad():
        a = [t.clone() for t in eng.forward_resident(img.cuda())]                        # uint8 NHWC, normalisation fused
        b = [t.clone() for t in eng.forward_resident(xf.half().cuda())]                  # fp16 NHWC
        c = [t.clone() for t in eng.forward_resident(xf.half().float().permute(0, 3, 1, 2).contiguous().cuda())]  # NCHW fp32
    assert torch.equal(a[0], b[0]) and torch.equal(b[0], c[0]) and torch.equal(b[1], c[1])


def _iou(a, b):
    x1, y1 = np.maximum(a[0], b[:, 0]), np.maximum(a[1], b[:, 1])
    x2, y2 = np.minimum(a[0] + a[2], b[:, 0] + b[:, 2]), np.minimum(a[1] + a[3], b[:, 1] + b[:, 3])
    inter = np.clip(x2 - x1, 0, None) * np.clip(y2 - y1, 0, None)
    return inter / (a[2] * a[3] + b[:, 2] * b[:, 3] - inter)


@pytest.mark.parametrize('name,ch', [CASES[0], CASES[2]], ids=[IDS[0], IDS[2]])
def test_detect_and_get_results(name, ch):
    cs = _case(name, ch)
    eng, m, x = cs['eng'], cs['m'], cs['x']
    n, h, w = x.shape[0], x.shape[2], x.shape[3]
    meta_rows = [dict(resized_height=h, resized_width=w, resize_scale=1.0)] * n
    meta = torch.tensor([[float(w), float(h), 1.0]] * n, device='cuda')
    with torch.no_grad():
        ref16 = m(x)
    old = m._classification_threshold
    m._classification_threshold = float(np.quantile(ref16[0].sigmoid().cpu().numpy() if cs['g']['cls'].shape[2] == 1
                                                    else ref16[0].softmax(-1)[..., :-1].cpu().numpy(), 0.9))
    try:
        with torch.no_grad():
            out = eng.detect(x, meta)
            rows8 = eng.get_results(eng(x), meta_rows)
            rows16 = m.get_results(ref16, meta_rows)
    finally:
        m._classification_threshold = old
    assert out.dets.shape[0] == n and out.dets.shape[2] == 5 and out.counts.shape == (n, 4)
    assert len(rows8) == n and all(len(r) == 6 for img in rows8 for r in img) and sum(len(r) for r in rows8) > 0
    found = total = 0
    for r8, r16 in zip(rows8, rows16):
        b8 = np.array(r8, np.float64).reshape(-1, 6)
        for r in r16:
            total += 1
            same = b8[b8[:, 0] == r[0]]
            found += int(len(same) > 0 and float(_iou(np.array(r[2:]), same[:, 2:]).max()) >= 0.5)
    print('%s: the int8 engine finds %d of the fp16 mode\'s %d detections (IoU >= 0.5, same label); its own count %d'
          % (name, found, total, sum(len(r) for r in rows8)))


def test_rebuild_from_the_cache_is_bit_equal_and_runs_no_calibration_batch():
    cs = _case(*CASES[0])

    class NoBatches(INT8Calibrator):
        def get_batch(self, names=None, p_str=None):
            raise AssertionError('the cache was there: no calibration batch may be asked for')

    eng2 = build_int8_engine(cs['m'], NoBatches(cs['data'], cs['cache'], batch_size=1))
    assert not eng2.calibrated and eng2.scales == cs['eng'].scales
    with torch.no_grad():
        cls, reg = eng2(cs['x'])
    assert torch.equal(cls, cs['cls']) and torch.equal(reg, cs['reg'])


@pytest.mark.parametrize('how', ['optimizer_step', 'load_state_dict'])
def test_parameter_change_makes_the_next_call_raise(how, tmp_path):
    g = load_golden('ref_model_WIDERFACE_LFD_XS.npz')
    m = configs.build_model('WIDERFACE_LFD_XS', seed=666)
    configs.perturb_weights(m, seed=1)
    m.eval().cuda()
    x = _frames(g, 3)
    cache = str(tmp_path / 'c.json')
    eng = build_int8_engine(m, INT8Calibrator(x.numpy(), cache, batch_size=1))
    with torch.no_grad():
        eng(x.cuda())
    if how == 'optimizer_step':
        p = next(m._backbone.parameters())
        p.grad = torch.ones_like(p)
        torch.optim.SGD([p], lr=0.1).step()
    else:
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        k0 = next(k for k in sd if k.endswith('weight'))
        sd[k0] = sd[k0] * 1.5
        m.load_state_dict(sd)
    with pytest.raises(RuntimeError, match='rebuild'):
        eng(x.cuda())
    # ... and the cache written for the old weights is not trusted: the rebuild calibrates again
    eng2 = build_int8_engine(m, INT8Calibrator(x.numpy(), cache, batch_size=1))
    assert eng2.calibrated
    with torch.no_grad():
        eng2(x.cuda())
