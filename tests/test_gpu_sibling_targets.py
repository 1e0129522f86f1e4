"""GPU suite, siblings: target assignment (csrc/assign_sibling.hip) and the fused FCOS get_loss (csrc/getloss_fcos.hip)
against the targets / loss values / prediction gradients the REAL reference produced (ref_sibling_<NAME>.npz,
ref_sibling_FCOSV1.npz, and the edge cases of ref_sibling_targets.npz), and against the host route kept behind
`device_targets = False`.

Bounds.  FCOS: labels equal, distances bit-equal (fp32 subtractions in the reference's order).  LFDv2: positive set and
per-row argmax class identical, scores within 1 fp32 ulp (the stated bound of the assign kernels: "up to the last bit of the
host's sqrt"), regression targets bit-equal on every row the reference's algebra decides.  That is every row of an image with
at most 16 boxes; with more boxes torch's default CPU sort is not stable, so WHICH of several boxes sharing the row's best
score the reference selects (in practice: which box of an all-zero row, whose target no loss reads) is an artefact of that
sort -- on those rows of the 70-box image the kernel's choice is checked against its own rule (lowest index) instead
(tests/test_sibling_targets_host.py::v2_rule states both).  Losses against the fixtures: 2e-4 * max(1, |v|), gradients 2e-4
of the gradient's max (tests/test_gpu_siblings.py); device route against host route 1e-5 relative; repeated runs bit-equal."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from conftest import load_golden
from lfd_amd import _lib, configs, ops
from lfd_amd.model import FCOS, FCOSv1, LFDv2, losses as L
import sibling_cases as SC
import sibling_target_cases as TC
from test_sibling_targets_host import _levels, fcos_rule, v2_model, v2_rule

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
V2_NAMES = sorted(k for k, v in configs.SIBLINGS.items() if v['meta'] == 'LFDv2')
GRAY = [(int(lo * 0.9), int(hi * 1.1)) for lo, hi in TC.V2_RANGES]


def _ulps(a, b):
    """largest |a - b| in units of the fp32 spacing at max(|a|, |b|)"""
    a, b = a.astype(np.float32), b.astype(np.float32)
    sp = np.spacing(np.maximum(np.abs(a), np.abs(b)).astype(np.float32))
    return float((np.abs(a.astype(np.float64) - b) / sp).max())


def _model_fixture(name):
    g = load_golden('ref_sibling_%s.npz' % name)
    spec = configs.SIBLINGS[name]
    n, H, W = [int(v) for v in g['shape']]
    return g, spec, [tuple(s) for s in g['sizes'].tolist()], SC.synth_annotations(5, n, H, W, spec['head']['num_classes'])


def _check_v2(ct, rt, ref_c, ref_r, decided=None):
    ct, rt = ct.cpu().numpy(), rt.cpu().numpy()
    np.testing.assert_array_equal(ct > 0, ref_c > 0)                               # positive set
    pos = ref_c.max(-1) > 0
    np.testing.assert_array_equal(ct.argmax(-1)[pos], ref_c.argmax(-1)[pos])       # per-row class
    u = _ulps(ct, ref_c)
    print('score difference: %.2f ulp' % u)
    assert u <= 1.0
    if decided is None:
        np.testing.assert_array_equal(rt, ref_r)
    else:
        np.testing.assert_array_equal(rt[decided], ref_r[decided])
    return rt


# ----------------------------------------------------------------------------------------------- targets
def test_fcos_targets_equal_the_reference_on_the_model_fixtures():
    g, spec, sizes, ann = _model_fixture('FCOS_FPN')
    strides = list(configs.build_sibling_model('FCOS_FPN')._point_strides)
    C_ = spec['head']['num_classes']
    lab, reg = ops.assign_targets_fcos_from_host(sizes, strides, spec['regress_ranges'], C_, ann, DEV)
    assert lab.dtype == torch.int64 and tuple(lab.shape) == g['cls_target'].shape
    np.testing.assert_array_equal(lab.cpu().numpy(), g['cls_target'])
    np.testing.assert_array_equal(reg.cpu().numpy(), g['reg_target'])
    # FCOSv1 on the overlapping annotations; the list form (device-resident annotations) gives the same tensors
    ref = load_golden('ref_sibling_FCOSV1.npz')
    n, H, W = [int(v) for v in g['shape']]
    ann = SC.synth_annotations_overlapping(5, n, H, W, C_)
    lab, reg = ops.assign_targets_fcos_from_host(sizes, strides, spec['regress_ranges'], C_, ann, DEV, multi_label=True)
    np.testing.assert_array_equal(lab.cpu().numpy(), ref['cls_target'])
    np.testing.assert_array_equal(reg.cpu().numpy(), ref['reg_target'])
    lab2, reg2 = ops.assign_targets_fcos(sizes, strides, spec['regress_ranges'], C_, [torch.from_numpy(b).to(DEV) for b, _ in ann],
                                         [torch.from_numpy(l).to(DEV) for _, l in ann], multi_label=True)
    assert torch.equal(lab, lab2) and torch.equal(reg, reg2)


def test_fcos_targets_equal_the_reference_on_the_edge_cases():
    g = load_golden('ref_sibling_targets.npz')
    ann = TC.annotations()
    lab, reg = ops.assign_targets_fcos_from_host(TC.SIZES, TC.STRIDES, TC.FCOS_RANGES, TC.NUM_CLASSES, ann, DEV)
    np.testing.assert_array_equal(lab.cpu().numpy(), g['fcos_labels'])
    np.testing.assert_array_equal(reg.cpu().numpy(), g['fcos_reg'])
    lab, reg = ops.assign_targets_fcos_from_host(TC.SIZES, TC.STRIDES, TC.FCOS_RANGES, TC.NUM_CLASSES, ann, DEV, multi_label=True)
    np.testing.assert_array_equal(lab.cpu().numpy()[1:], g['fcosv1_labels'])
    np.testing.assert_array_equal(reg.cpu().numpy()[1:], g['fcosv1_reg'])
    assert bool((lab[0] == 1).all()) and not bool(reg[0].any())          # no boxes: all background (the mirror's rows)


@pytest.mark.parametrize('name', V2_NAMES)
def test_v2_targets_equal_the_reference_on_the_model_fixtures(name):
    g, spec, sizes, ann = _model_fixture(name)
    m = configs.build_sibling_model(name)
    ct, rt = ops.assign_targets_v2_from_host(sizes, m._point_strides, m._regression_ranges, m._gray_ranges, m._num_classes,
                                             m._range_assign_mode, m._regression_loss_type == 'independent', ann, DEV)
    _check_v2(ct, rt, g['cls_target'], g['reg_target'])
    ct2, rt2 = ops.assign_targets_v2(sizes, m._point_strides, m._regression_ranges, m._gray_ranges, m._num_classes,
                                     m._range_assign_mode, m._regression_loss_type == 'independent',
                                     [torch.from_numpy(b).to(DEV) for b, _ in ann], [torch.from_numpy(l).to(DEV) for _, l in ann])
    assert torch.equal(ct, ct2) and torch.equal(rt, rt2)


@pytest.mark.parametrize('ci', range(len(TC.V2_CASES)), ids=['%s-%s' % c for c in TC.V2_CASES])
def test_v2_targets_equal_the_reference_on_the_edge_cases(ci):
    mode, loss = TC.V2_CASES[ci]
    g = load_golden('ref_sibling_targets.npz')
    ann = TC.annotations()
    indep = loss == 'SmoothL1Loss'
    ct, rt = ops.assign_targets_v2_from_host(TC.SIZES, TC.STRIDES, TC.V2_RANGES, GRAY, TC.NUM_CLASSES, mode, indep, ann, DEV)
    pts, lvl = TC.points(), _levels(TC.SIZES)
    rule = [v2_rule(pts, lvl, TC.STRIDES, TC.V2_RANGES, GRAY, b, l, TC.NUM_CLASSES, mode, indep) for b, l in ann]
    decided = np.stack([r[2] for r in rule])
    assert decided[:2].all() and not decided[2].all()
    rt = _check_v2(ct, rt, g['v2_%d_cls' % ci], g['v2_%d_reg' % ci], decided)
    # rows of the 70-box image whose best score several boxes share: the kernel's rule, the lowest box index
    np.testing.assert_array_equal(rt[2], rule[2][1])


# ----------------------------------------------------------------------------------------------- get_loss vs the reference
def _loss_vs_fixture(model, preds, ann, want, grads):
    assert model._fused_loss_supported(preds[0]) or isinstance(model, LFDv2)
    lo = model.get_loss(tuple(preds), ann)
    assert set(lo['loss_values']) == set(want) and isinstance(lo['loss'], torch.Tensor)
    for k, v in want.items():
        assert isinstance(lo['loss_values'][k], float)
        print(k, lo['loss_values'][k], v)
        assert abs(lo['loss_values'][k] - v) <= 2e-4 * max(1.0, abs(v)), (k, lo['loss_values'][k], v)
    lo['loss'].backward()
    for ref_g, p in zip(grads, preds):
        scale = max(np.abs(ref_g).max(), 1e-12)
        err = np.abs(p.grad.cpu().numpy() - ref_g).max()
        print('grad err / max', err / scale)
        assert err <= 2e-4 * scale


@pytest.mark.parametrize('name', sorted(configs.SIBLINGS))
def test_get_loss_on_the_device_path_vs_reference(name):
    g, spec, sizes, ann = _model_fixture(name)
    model = configs.build_sibling_model(name, seed=1).to(DEV)
    for i, hw in enumerate(sizes):
        model._head_indexes_to_feature_map_sizes[i] = hw
    preds = [torch.from_numpy(g[k]).to(DEV).requires_grad_(True) for k in ('cls', 'reg', 'ctr') if k in g.files]
    assert model.device_targets
    assert model._fused_loss_supported(preds[0]) == (name != 'LFDV2_SFPN')       # GIoU: op by op on the device-made targets
    _loss_vs_fixture(model, preds, ann, json.loads(str(g['loss_values'])), [g[k] for k in ('dcls', 'dreg', 'dctr')[:len(preds)]])


def test_fcosv1_get_loss_on_the_device_path_vs_reference():
    from test_sibling_oracle_golden import _fcosv1_model_and_annotations
    g, model, ann = _fcosv1_model_and_annotations()
    ref = load_golden('ref_sibling_FCOSV1.npz')
    model.to(DEV)
    preds = [torch.from_numpy(g[k]).to(DEV).requires_grad_(True) for k in ('cls', 'reg', 'ctr')]
    assert model._fused_loss_supported(preds[0]) and model._multi_label
    _loss_vs_fixture(model, preds, ann, json.loads(str(ref['loss_values'])), [ref[k] for k in ('dcls', 'dreg', 'dctr')])


# ----------------------------------------------------------------------------------------------- device route vs host route
def _fcos_model(cls, reg_loss):
    m = cls(num_classes=TC.NUM_CLASSES, regress_ranges=TC.FCOS_RANGES, point_strides=TC.STRIDES,
            classification_loss_func=L.FocalLoss(gamma=2.0, alpha=0.25, loss_weight=1.25),
            regression_loss_func=getattr(L, reg_loss)(loss_weight=0.75),
            centerness_loss_func=L.BCEWithLogitsLoss(loss_weight=1.5))
    for i, hw in enumerate(TC.SIZES):
        m._head_indexes_to_feature_map_sizes[i] = hw
    return m


def _fcos_preds(n, seed=3):
    g = torch.Generator().manual_seed(seed)
    P = TC.total_points()
    return [torch.randn(n, P, TC.NUM_CLASSES, generator=g), torch.rand(n, P, 4, generator=g) * 40.0 + 1.0,
            torch.randn(n, P, 1, generator=g)]


def _run(model, preds, ann):
    ps = [p.clone().to(DEV).requires_grad_(True) for p in preds]
    lo = model.get_loss(tuple(ps), ann)
    lo['loss'].backward()
    return lo['loss_values'], lo['loss'].detach().clone(), [p.grad.clone() for p in ps]


def _compare_routes(model, preds, ann):
    a = _run(model, preds, ann)
    b = _run(model, preds, ann)
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))   # fixed-order sums
    model.device_targets = False
    h = _run(model, preds, ann)
    model.device_targets = True
    assert set(a[0]) == set(h[0])
    for k in h[0]:
        print(k, a[0][k], h[0][k])
        assert abs(a[0][k] - h[0][k]) <= 1e-5 * abs(h[0][k]), (k, a[0][k], h[0][k])
    for x, y in zip(a[2], h[2]):
        assert float((x - y).abs().max()) <= 1e-5 * float(y.abs().max())
    return a


@pytest.mark.parametrize('cls,reg_loss', [(FCOS, 'IoULoss'), (FCOS, 'GIoULoss'), (FCOS, 'DIoULoss'), (FCOS, 'CIoULoss'),
                                          (FCOSv1, 'GIoULoss')], ids=lambda v: getattr(v, '__name__', v))
def test_fcos_device_route_equals_the_host_route_on_the_edge_cases(cls, reg_loss):
    model = _fcos_model(cls, reg_loss)
    a = _compare_routes(model, _fcos_preds(TC.N_IMAGES), TC.annotations())
    assert a[0]['regression_loss'] > 0 and a[0]['centerness_loss'] > 0


V2_ROUTES = [('longer', 'CrossEntropyLoss', 'IoULoss', 'sigmoid'), ('dist', 'FocalLoss', 'IoULoss', 'exp'),
             ('sqrt', 'FocalLoss', 'GIoULoss', 'exp'), ('longer', 'FocalLoss', 'SmoothL1Loss', 'exp')]


@pytest.mark.parametrize('mode,closs,rloss,decode', V2_ROUTES, ids=['-'.join(r) for r in V2_ROUTES])
def test_v2_device_route_equals_the_host_route_on_the_edge_cases(mode, closs, rloss, decode):
    """the compositions of LFDV2_SIMPLE / LFDV2_HEADV1 (fused get_loss), LFDV2_SFPN and an 'independent' loss (op by op on the
    device-made targets).  Image 2 keeps its first 16 boxes: with more, the HOST route's regression target of a point in
    several core zones (equal scores) depends on torch's unstable sort (module docstring)."""
    model = LFDv2(num_classes=TC.NUM_CLASSES, regression_ranges=TC.V2_RANGES, gray_range_factors=TC.GRAY_FACTORS,
                  range_assign_mode=mode, point_strides=TC.STRIDES, classification_loss_func=getattr(L, closs)(),
                  regression_loss_func=getattr(L, rloss)(), distance_to_bbox_mode=decode)
    for i, hw in enumerate(TC.SIZES):
        model._head_indexes_to_feature_map_sizes[i] = hw
    ann = TC.annotations()
    ann[2] = (ann[2][0][:16], ann[2][1][:16])
    g = torch.Generator().manual_seed(5)
    P = TC.total_points()
    ch = TC.NUM_CLASSES + (1 if closs == 'CrossEntropyLoss' else 0)
    preds = [torch.randn(3, P, ch, generator=g), torch.randn(3, P, 4, generator=g) * 0.5 + (2.0 if decode == 'exp' else 0.0)]
    if rloss == 'SmoothL1Loss':
        preds[1] = torch.rand(3, P, 4, generator=g) * 0.6
    assert model._fused_loss_supported(preds[0].to(DEV)) == (rloss == 'IoULoss')
    a = _compare_routes(model, preds, ann)
    assert a[0]['regression_loss'] > 0


@pytest.mark.parametrize('cls', [FCOS, FCOSv1], ids=lambda c: c.__name__)
def test_fcos_batch_without_positives(cls):
    model = _fcos_model(cls, 'GIoULoss')
    empty = (np.zeros((0, 4), np.float32), np.zeros((0,), np.int64))
    far = (np.array([[500., 500., 20., 20.]], np.float32), np.array([1], np.int64))      # a box no point lies in
    vals, _, grads = _run(model, _fcos_preds(2), [empty, far])
    assert vals['regression_loss'] == 0.0 and vals['centerness_loss'] == 0.0 and vals['classification_loss'] > 0
    assert vals['loss'] == vals['classification_loss']
    assert not bool(grads[1].any()) and not bool(grads[2].any())
    assert bool(torch.isfinite(grads[0]).all()) and bool(grads[0].any())


def test_fcos_rank_arithmetic_on_one_device():
    """image-parallel training without a second GPU: a batch of 2 as two ranks of 1 -- local sums, their total as the
    all-reduced vector, rank_scale 2; the ranks' gradients, averaged as DDP does, are the whole-batch gradient"""
    ann = TC.annotations()[1:]
    preds = [p.to(DEV) for p in _fcos_preds(2, seed=9)]
    gout = torch.tensor([0., 0., 0., 1.], device=DEV)

    def desc(n):
        return ops.make_fcos_loss_desc(n, TC.SIZES, TC.STRIDES, TC.NUM_CLASSES, 'GIoULoss', cls_loss_weight=1.25,
                                       reg_loss_weight=0.75, ctr_loss_weight=1.5)
    lab, reg_t = ops.assign_targets_fcos_from_host(TC.SIZES, TC.STRIDES, TC.FCOS_RANGES, TC.NUM_CLASSES, ann, DEV)
    whole_sums = ops.fcos_loss_sums(desc(2), *preds, lab, reg_t)
    fin = ops.fcos_loss_finalize(desc(2), whole_sums, whole_sums)
    whole = ops.fcos_loss_backward(desc(2), *preds, lab, reg_t, fin, gout)
    halves = [[p[i:i + 1].contiguous() for p in preds] + [lab[i:i + 1].contiguous(), reg_t[i:i + 1].contiguous()] for i in (0, 1)]
    sums = [ops.fcos_loss_sums(desc(1), *h) for h in halves]
    total = sums[0] + sums[1]
    assert float((total - whole_sums).abs().max()) <= 1e-9 * float(whole_sums.abs().max())
    assert total[5:].tolist() == [0.0, 0.0, 0.0] and float(total[3]) > 0
    fins = [ops.fcos_loss_finalize(desc(1), s, total, rank_scale=2.0) for s in sums]
    # each rank reports rank_scale * (its share of the global loss): the mean over ranks is the whole-batch loss
    assert abs(float(fins[0][3] + fins[1][3]) / 2 - float(fin[3])) <= 1e-6 * float(fin[3])
    grads = [ops.fcos_loss_backward(desc(1), *h, f, gout) for h, f in zip(halves, fins)]
    for k in range(3):
        mean = torch.cat([grads[0][k], grads[1][k]], 0) / 2.0        # rank r's gradient is zero outside its own image
        assert float((mean - whole[k]).abs().max()) <= 1e-6 * float(whole[k].abs().max()), k


# ----------------------------------------------------------------------------------------------- argument validation
def test_argument_validation_returns_status_codes_without_launching():
    l = _lib.lib()
    fd, _ = ops.make_assign_fcos_desc(2, TC.SIZES, TC.STRIDES, TC.FCOS_RANGES, TC.NUM_CLASSES)
    vd, _ = ops.make_assign_desc(2, TC.SIZES, TC.STRIDES, TC.V2_RANGES, GRAY, TC.NUM_CLASSES, 'longer', False)
    one = C.c_int(0)
    p = C.byref(one)          # never dereferenced: every call below is refused on the host
    good = (C.c_int32 * 3)(0, 1, 2)
    back = (C.c_int32 * 3)(0, 2, 1)                                          # negative step
    over = (C.c_int32 * 3)(0, 1, 5)                                          # beyond num_boxes
    for fn, d in ((l.lfd_assign_targets_fcos_f32, fd), (l.lfd_assign_targets_v2_f32, vd)):
        assert fn(None, p, p, 2, p, good, p, p, None) == -1
        assert fn(C.byref(d), p, p, 2, None, good, p, p, None) == -1         # no offsets
        assert fn(C.byref(d), p, p, 2, p, good, None, p, None) == -1         # no outputs
        assert fn(C.byref(d), p, p, 2, p, good, p, None, None) == -1
        assert fn(C.byref(d), None, p, 2, p, good, p, p, None) == -1         # boxes announced, none given
        assert fn(C.byref(d), p, p, 2, p, back, p, p, None) == -1
        assert fn(C.byref(d), p, p, 2, p, over, p, p, None) == -1
        d.num_levels = _lib.MAX_LEVELS + 1
        assert fn(C.byref(d), p, p, 2, p, good, p, p, None) == -1
        d.num_levels = 3
        d.total_points += 1                                                  # levels do not add up
        assert fn(C.byref(d), p, p, 2, p, good, p, p, None) == -1
        d.total_points -= 1
    ld = ops.make_fcos_loss_desc(2, TC.SIZES, TC.STRIDES, TC.NUM_CLASSES, 'GIoULoss')
    assert l.lfd_fcos_loss_workspace_bytes() > 0
    assert l.lfd_fcos_loss_sums_f32(None, p, p, p, p, p, p, 1 << 20, p, None) == -1
    assert l.lfd_fcos_loss_sums_f32(C.byref(ld), p, p, None, p, p, p, 1 << 20, p, None) == -1
    assert l.lfd_fcos_loss_sums_f32(C.byref(ld), p, p, p, p, p, p, 8, p, None) == -2          # workspace too small
    assert l.lfd_fcos_loss_finalize_f32(C.byref(ld), None, p, 1.0, p, None) == -1
    assert l.lfd_fcos_loss_bwd_f32(C.byref(ld), p, p, p, p, p, p, p, p, p, None, None) == -1
    ld.box_loss = 4
    assert l.lfd_fcos_loss_sums_f32(C.byref(ld), p, p, p, p, p, p, 1 << 20, p, None) == -1
    ld.box_loss, ld.num_levels = 1, _lib.MAX_LEVELS + 1
    assert l.lfd_fcos_loss_bwd_f32(C.byref(ld), p, p, p, p, p, p, p, p, p, p, None) == -1
    with pytest.raises(RuntimeError):
        ops.assign_targets_fcos(TC.SIZES, TC.STRIDES, TC.FCOS_RANGES, TC.NUM_CLASSES, [torch.zeros(1, 4)], [torch.zeros(1).long()])
