"""The INT8 mode's clipping calibration rules end to end on the MI355X (lfd_amd/calibration.py, deployment.py, engine_i8.py,
csrc/calib_hist.hip): the device histograms against Int8Plan.calibrate's amax, the default path unchanged, every int8
launch of an engine built under 'entropy', 'mse' and percentile=99 re-derived from the plan's own tensors, saturation at +127
counted exactly, the version-2 cache, graph replay, and the logits against the reference's fp32 fixture.

Models, frames and the calibration set are those of tests/test_gpu_int8_engine.py (its _case builds the default engine once for
both files)."""
import functools
import os
import shutil
import tempfile

import numpy as np
import pytest
import torch

import conv_i8_cases as QC
import test_gpu_int8_engine as E
from lfd_amd import INT8Calibrator, build_int8_engine, calibration, engine_i8, ops

pytestmark = pytest.mark.gpu

CONFIGS = ['WIDERFACE_LFD_S', 'TT100K_LFD_L']
RULES = {'entropy': ('entropy', {}), 'mse': ('mse', {}), 'percentile99': ('percentile', dict(percentile=99.0))}

# max |sigmoid(out) - sigmoid(reference fp32 fixture)| over (cls, reg) of the fixture frames, measured on the MI355X with the
# calibration set of tests/test_gpu_int8_engine.py (DESIGN 4k has the table; the default rule's values are INT8_SIGMA_MEASURED
# there: 3.425e-2 and 5.935e-2 for these two configurations).  The gate is 1.5 x the measured value: the kernels are deterministic, the margin covers another toolchain's fp16
# calibration bits -- not to be widened.  Whether a rule beats 'amax' is reported, not gated.
SIGMA_MEASURED = {
    ('WIDERFACE_LFD_S', 'entropy'): 3.812e-2,        # cls 2.727e-2, reg 3.812e-2
    ('WIDERFACE_LFD_S', 'mse'): 3.667e-2,            # cls 2.595e-2, reg 3.667e-2
    ('WIDERFACE_LFD_S', 'percentile99'): 1.683e-1,   # cls 9.577e-2, reg 1.683e-1
    ('TT100K_LFD_L', 'entropy'): 6.714e-2,           # cls 6.714e-2, reg 5.101e-2
    ('TT100K_LFD_L', 'mse'): 5.955e-2,               # cls 5.955e-2, reg 4.200e-2
    ('TT100K_LFD_L', 'percentile99'): 2.270e-1,      # cls 2.012e-1, reg 2.270e-1
}


def _batches(cs):
    return [torch.from_numpy(cs['data'][i:i + 1]).cuda() for i in range(cs['data'].shape[0])]


@functools.lru_cache(maxsize=None)
def _rule_case(name, rule):
    cs = E._case(name, 3)
    algorithm, params = RULES[rule]
    cache = os.path.join(tempfile.mkdtemp(prefix='lfd_int8_%s_' % rule), 'calibration.json')
    cal = INT8Calibrator(cs['data'], cache, batch_size=1, algorithm=algorithm, **params)
    eng = build_int8_engine(cs['m'], cal)
    assert eng.calibrated and os.path.exists(cache)
    with torch.no_grad():
        cls, reg = eng(cs['x'])
    return dict(eng=eng, cal=cal, cache=cache, cls=cls, reg=reg)


@functools.lru_cache(maxsize=None)
def _histograms(name):
    cs = E._case(name, 3)
    return cs['eng'].plan.calibrate_histograms(_batches(cs))


@pytest.mark.parametrize('name', CONFIGS)
def test_histogram_amax_is_calibrates_amax(name):
    cs = E._case(name, 3)
    plan = cs['eng'].plan
    hists = _histograms(name)
    amax = plan.calibrate(_batches(cs))
    assert list(hists) == plan.tensor_names == list(amax)
    for k in plan.tensor_names:
        assert hists[k].dtype == np.int64 and hists[k].shape == (32768,)
        assert calibration.amax_of(hists[k], k) == amax[k] == cs['eng'].scales[k][0], k
    # the counts are the real channels' elements: the stem, and every conv output at its own resolution
    frames, h, w = cs['data'].shape[0], cs['data'].shape[2], cs['data'].shape[3]
    st = plan.state_for(1, h, w, 0)
    stem = st.bufs[plan.stage_in]
    assert int(hists['stem'].sum()) == frames * stem.shape[1] * stem.shape[2] * plan.stem_channels_real
    for c in plan.layers:
        assert int(hists[c.name].sum()) == frames * st.qbufs[c.dst].shape[1] * st.qbufs[c.dst].shape[2] * c.cout_real, c.name
    assert hists['stem'][0] > 0                                       # post-ReLU: zeros are there, counted by the ballot path
    # a second pass gives the same bits
    again = plan.calibrate_histograms(_batches(cs))
    assert all(np.array_equal(hists[k], again[k]) for k in hists)


@pytest.mark.parametrize('name', CONFIGS)
def test_percentile_100_engine_is_the_default_engine(name):
    cs = E._case(name, 3)
    cache = os.path.join(tempfile.mkdtemp(prefix='lfd_int8_p100_'), 'calibration.json')
    eng = build_int8_engine(cs['m'], INT8Calibrator(cs['data'], cache, batch_size=1, algorithm='percentile', percentile=100))
    assert eng.calibrated and eng.scales == cs['eng'].scales
    assert eng.calibration['threshold'] == eng.calibration['amax'] == cs['eng'].calibration['amax']
    assert all(v == 0.0 for v in eng.calibration['clipped'].values())
    assert cs['eng'].calibration['algorithm'] == 'amax' and cs['eng'].calibration['threshold'] == cs['eng'].calibration['amax']
    with torch.no_grad():
        cls, reg = eng(cs['x'])
    assert torch.equal(cls, cs['cls']) and torch.equal(reg, cs['reg'])


@pytest.mark.parametrize('rule', list(RULES))
@pytest.mark.parametrize('name', CONFIGS)
def test_calibration_report_and_scales(name, rule):
    cs, rc = E._case(name, 3), _rule_case(name, rule)
    eng, rep = rc['eng'], rc['eng'].calibration
    hists = _histograms(name)
    algorithm, params = RULES[rule]
    assert sorted(rep) == ['algorithm', 'amax', 'clipped', 'params', 'threshold'] and rep['algorithm'] == algorithm
    assert rep['params'] == calibration.check_params(algorithm, params)
    clipped_any = 0
    for k in eng.plan.tensor_names:
        t, share = calibration.threshold(hists[k], algorithm, k, **params)
        assert (rep['threshold'][k], rep['clipped'][k]) == (t, share) and rep['amax'][k] == cs['eng'].scales[k][0]
        assert 0.0 <= t <= rep['amax'][k] and eng.scales[k] == (t, engine_i8.act_scale(t))
        clipped_any += int(share > 0)
        if rule == 'percentile99':
            assert share <= 0.01, k
    print('%s %s: %d of %d tensors clipped; largest clipped share %.3e; smallest T / amax %.3f'
          % (name, rule, clipped_any, len(rep['threshold']), max(rep['clipped'].values()),
             min(rep['threshold'][k] / rep['amax'][k] for k in rep['amax'])))


@pytest.mark.parametrize('rule', list(RULES))
@pytest.mark.parametrize('name', CONFIGS)
def test_every_int8_launch_rederived_under_a_clipping_rule(name, rule):
    cs, rc = E._case(name, 3), _rule_case(name, rule)
    eng, x = rc['eng'], cs['x']
    plan = eng.plan
    with torch.no_grad():
        eng.forward_resident(x)
    torch.cuda.synchronize()
    st = plan.state_for(x.shape[0], x.shape[2], x.shape[3], 0)
    worst, saturated = 0.0, 0
    for c in plan.layers:
        s_w, q_w = engine_i8.weight_scales(c.ref_w)
        assert torch.equal(ops.unpack_conv_weight_i8(c.w, c.cin, c.ks), q_w.to(c.w.device))
        s_in, s_out = eng.scales[c.src_name][1], eng.scales[c.name][1]
        assert (c.s_in, c.s_out) == (s_in, s_out) and s_out == engine_i8.act_scale(eng.calibration['threshold'][c.name])
        assert torch.equal(c.mult.cpu(), (s_w.double().cpu() * s_in / s_out).float())
        assert torch.equal(c.biasq.cpu(), (c.ref_b.double().cpu() / s_out).float())
        res = st.qbufs[c.res] if c.res is not None else None
        if res is not None:
            assert c.res_mult == float(torch.tensor(eng.scales[c.res_name][1] / s_out, dtype=torch.float64).float())
        acc = QC.acc_ref(st.qbufs[c.src], q_w.cuda(), c.stride)             # int64-exact conv in float64
        v, q_ref, f_ref = QC.epilogue_ref(acc, QC.Consts(c.mult, c.biasq, c.res_mult, c.s_out), res, c.relu)
        tie = QC.near_tie(v)
        share = float(tie.double().mean())
        worst = max(worst, share)
        diff = (st.qbufs[c.dst].int() - q_ref.int()).abs()
        assert share <= QC.NEAR_TIE_CAP, (c.name, share)
        assert int(diff[~tie].max()) == 0 and int(diff.max()) <= 1, c.name
        saturated += int((v[..., :c.cout_real] > 127.5).sum())
        if c.tap is not None:
            err = (st.bufs[c.tap].double() - f_ref).abs()
            assert bool((err <= QC.f16_ulp(f_ref)).all()), c.name
        assert bool((st.qbufs[c.dst][..., c.cout_real:] == 0).all()), c.name
    print('%s %s: %d int8 launches, largest near-tie share %.4f, %d outputs saturate at +127'
          % (name, rule, len(plan.layers), worst, saturated))


@pytest.mark.parametrize('name', CONFIGS)
def test_saturation_of_the_stem_map_is_real_and_exact(name):
    cs, rc = E._case(name, 3), _rule_case(name, 'percentile99')
    eng, x = rc['eng'], cs['x']
    plan = eng.plan
    with torch.no_grad():
        eng.forward_resident(x)
    torch.cuda.synchronize()
    st = plan.state_for(x.shape[0], x.shape[2], x.shape[3], 0)
    stem = st.bufs[plan.stage_in]
    inv = torch.tensor(1.0 / eng.scales['stem'][1], dtype=torch.float64).float().cuda()
    want = torch.round(stem.float() * inv).clamp(max=127.0) == 127.0
    got = st.qbufs[0][..., :stem.shape[3]] == 127
    assert int(got.sum()) == int(want.sum()) and torch.equal(got, want)
    assert int(want.sum()) > 0
    over = int((torch.round(stem.float() * inv) > 127.0).sum())
    assert over > 0                                                    # values beyond the threshold are there and were clipped
    assert int(st.qbufs[0].max()) == 127
    print('%s: %d stem codes at +127, %d of them clipped (of %d)' % (name, int(want.sum()), over, stem.numel()))


def test_second_build_reads_the_version_2_cache(tmp_path):
    cs, rc = E._case(CONFIGS[0], 3), _rule_case(CONFIGS[0], 'entropy')
    eng2 = build_int8_engine(cs['m'], rc['cal'])                      # the same calibrator object: its batches are used up
    assert not eng2.calibrated and eng2.scales == rc['eng'].scales
    assert eng2.calibration['threshold'] == rc['eng'].calibration['threshold'] and eng2.calibration['clipped'] is None
    assert eng2.calibration['amax'] == rc['eng'].calibration['amax']
    with torch.no_grad():
        cls, reg = eng2(cs['x'])
    assert torch.equal(cls, rc['cls']) and torch.equal(reg, rc['reg'])
    # other parameters, another rule and the default rule do not accept that cache (each on its own copy: a build rewrites it)
    p99 = _rule_case(CONFIGS[0], 'percentile99')
    for i, (src, kw) in enumerate(((p99['cache'], dict(algorithm='percentile', percentile=99.5)),
                                   (rc['cache'], dict(algorithm='percentile', percentile=99.0)), (rc['cache'], dict()))):
        copy = str(tmp_path / ('c%d.json' % i))
        shutil.copy(src, copy)
        assert build_int8_engine(cs['m'], INT8Calibrator(cs['data'][:1], copy, batch_size=1, **kw)).calibrated, kw
    # ... and a version-1 cache does not satisfy a clipping calibrator
    copy = str(tmp_path / 'v1.json')
    shutil.copy(cs['cache'], copy)
    assert build_int8_engine(cs['m'], INT8Calibrator(cs['data'][:1], copy, batch_size=1, algorithm='percentile')).calibrated


def test_graph_replay_equals_eager_under_a_clipping_rule():
    cs, rc = E._case(CONFIGS[0], 3), _rule_case(CONFIGS[0], 'mse')
    eng, x = rc['eng'], cs['x']
    with torch.no_grad():
        a = eng(x)
        eng.use_graph = True
        try:
            b = eng(x)
            c = eng(x)                                                   # a replay
        finally:
            eng.use_graph = False
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(b[0], c[0]) and torch.equal(b[1], c[1])
    assert torch.equal(a[0], rc['cls']) and torch.equal(a[1], rc['reg'])


@pytest.mark.parametrize('rule', list(RULES))
@pytest.mark.parametrize('name', CONFIGS)
def test_logits_against_the_reference_fp32_fixture(name, rule):
    cs, rc = E._case(name, 3), _rule_case(name, rule)
    e_rule = E._sigma_errors((rc['cls'], rc['reg']), cs['g'])
    e_amax = E._sigma_errors((cs['cls'], cs['reg']), cs['g'])
    print('%s %s: max |sigma(out) - sigma(ref)| cls / reg: %.3e / %.3e; default rule %.3e / %.3e'
          % (name, rule, e_rule[0], e_rule[1], e_amax[0], e_amax[1]))
    assert SIGMA_MEASURED[(name, rule)] is not None, 'no measured value recorded'
    assert max(e_rule) <= 1.5 * SIGMA_MEASURED[(name, rule)]
