"""GPU suite: the fused get_loss for every pair of loss modules LFD / LFDv2 accept (csrc/getloss_ex.hip).

1. Kernel level, through ops: all 4 x 6 pairs against a float64 restatement of lfd.py:300-395 and of the loss formulas
   (written below), next to the op-by-op route (LFD._loss_from_targets on the stand-alone HIP loss kernels) on the same
   inputs.  Gate, per output (the three loss values, d cls, d reg):
       max |fused - f64|  <=  2 * max |op-by-op - f64|  +  one fp32 ulp of max |f64|
   i.e. the error of a tensor is its largest absolute error and "the value" whose ulp is granted is the tensor's largest
   magnitude -- an element-wise reading would compare two independent roundings of the same last bit element by element.
   Exact: gray rows have zero gradients, non-positive rows a zero regression gradient, every output element is written
   (outputs are NaN before the launch), two runs are bit-equal.
2. Route against route: model.get_loss + backward with LFD_FUSED_LOSS_EX on and off, the gates of
   test_gpu_losses.py::test_fused_get_loss_equals_op_by_op_path_and_oracle (2e-5 / 2e-4 / 2e-3 relative, same zeros).
3. The REAL reference's values (ref_train_step_TL_LFD_L.npz: QFL + IoU; ref_sibling_LFDV2_SFPN.npz: Focal + GIoU): the fused
   route's error against the golden is at most twice the op-by-op route's error against the same golden.
4. Integration: the named models report the fused route (TL_LFD_L with the switch unset, LFDV2_SFPN with
   LFD_FUSED_LOSS_EX=1: unset, only the 'ex' pairs on IoULoss take it), LFDv2 takes DeviceAnnotations, GraphedTrainStep
   captures a QFL + GIoU network, LFDV2_SFPN trains -- the last three with LFD_FUSED_LOSS_EX=1.

Measured on the MI355X (printed by every test; tables in DESIGN 9h): worst fused / op-by-op error ratio of 1. 1.67 (the total
loss of QFL + DIoU, 1.7 fp32 ulp), 1.63 on a gradient; in 3. the fused route's errors equal the op-by-op route's or are 0.
"""
import copy
import ctypes as C
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from lfd_amd import _lib, configs, ops, optim, train
from lfd_amd.data import DeviceAnnotations
from lfd_amd.model import losses as L
from lfd_amd.model.lfd import LFD
from lfd_amd.model.lfdv2 import LFDv2
import sibling_cases as SC
import train_step_cases as TSC

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZES, STRIDES, RANGES = [(13, 17), (7, 9), (4, 5)], (8, 16, 32), ((4, 32), (32, 64), (64, 128))
CLS_KW = {'FocalLoss': dict(gamma=2.0, alpha=0.25, loss_weight=1.25), 'CrossEntropyLoss': dict(loss_weight=0.75),
          'QualityFocalLoss': dict(beta=2.0, loss_weight=2.0), 'BCEWithLogitsLoss': dict(loss_weight=1.5)}
REG_KW = {'IoULoss': dict(eps=1e-6, loss_weight=1.0), 'GIoULoss': dict(eps=1e-6, loss_weight=0.5),
          'DIoULoss': dict(eps=1e-6, loss_weight=1.5), 'CIoULoss': dict(eps=1e-6, loss_weight=0.8),
          'SmoothL1Loss': dict(beta=0.3, loss_weight=2.0), 'MSELoss': dict(loss_weight=3.0)}
INDEPENDENT = ('SmoothL1Loss', 'MSELoss')


@pytest.fixture
def ex_on(monkeypatch):
    """LFD_FUSED_LOSS_EX=1: every admitted pair on the fused route (unset, only the 'ex' pairs on IoULoss take it)"""
    monkeypatch.setenv('LFD_FUSED_LOSS_EX', '1')


# ------------------------------------------------------------------------------------------------------- inputs
def _inputs(seed, n, num_classes, cls_name, reg_name, decode, sizes=SIZES, no_positive=False):
    """cls targets with positives (one class score per point, a second smaller one on some rows: soft target vectors), green
    rows whose best score is below the 0.001 threshold, gray rows (a -1 somewhere, also on rows with a score), image 1
    without boxes; regression targets as distances ('union') or normalised ('independent'); predictions for the decode"""
    rng = np.random.default_rng(seed)
    P, Cn = sum(h * w for h, w in sizes), num_classes
    ct = np.zeros((n, P, Cn), np.float32)
    cls = rng.integers(0, Cn, (n, P))
    if not no_positive:
        pos = rng.random((n, P)) < 0.12
        pos[1] = False
        pos[-1, -3:] = True                                   # the last rows of the batch
        score = rng.uniform(0.05, 1.0, (n, P)).astype(np.float32)
        ii, pp = np.nonzero(pos)
        ct[ii, pp, cls[ii, pp]] = score[ii, pp]
        if Cn > 1:
            ii, pp = np.nonzero(pos & (rng.random((n, P)) < 0.3))
            ct[ii, pp, (cls[ii, pp] + 1) % Cn] = score[ii, pp] * 0.5
        low = ~pos & (rng.random((n, P)) < 0.03)
        low[1] = False
        ii, pp = np.nonzero(low)
        ct[ii, pp, cls[ii, pp]] = 0.0005
    gray = rng.random((n, P)) < 0.05
    if not no_positive:
        gray[1] = False
        gray[-1, -3:] = False
    ii, pp = np.nonzero(gray)
    ct[ii, pp, rng.integers(0, Cn, len(ii))] = -1.0
    ch = Cn + 1 if cls_name == 'CrossEntropyLoss' else Cn
    pc = rng.normal(-1, 2, (n, P, ch)).astype(np.float32)
    if reg_name in INDEPENDENT:
        rt = rng.uniform(0, 1, (n, P, 4)).astype(np.float32)
        pr = (rt + rng.normal(0, 0.4, (n, P, 4))).astype(np.float32)
    else:
        rt = rng.uniform(1, 40, (n, P, 4)).astype(np.float32)
        pr = (rng.normal(0, 0.5, (n, P, 4)) + 2.5 if decode == 'exp' else rng.normal(0, 1, (n, P, 4))).astype(np.float32)
    return [torch.from_numpy(a).to(DEV) for a in (pc, pr, ct, rt)]


def _bare_model(meta, cls_name, reg_name, decode, num_classes, cw=False, rw=False, sizes=SIZES, strides=STRIDES, ranges=RANGES,
                mode='dist'):
    m = meta(num_classes=num_classes, regression_ranges=ranges, point_strides=strides, range_assign_mode=mode,
             classification_loss_func=getattr(L, cls_name)(**CLS_KW[cls_name]),
             regression_loss_func=getattr(L, reg_name)(**REG_KW[reg_name]), distance_to_bbox_mode=decode,
             enable_classification_weight=cw, enable_regression_weight=rw)
    for i, hw in enumerate(sizes):
        m._head_indexes_to_feature_map_sizes[i] = hw
    return m


def _desc(n, num_classes, cls_name, reg_name, decode, cw, rw, sizes=SIZES, strides=STRIDES, ranges=RANGES):
    ck, rk = CLS_KW[cls_name], REG_KW[reg_name]
    return ops.make_loss_desc_ex(n, sizes, strides, ranges, num_classes, cls_name, reg_name, decode,
                                 gamma=ck.get('gamma', 2.0), alpha=ck.get('alpha', 0.25), qfl_beta=ck.get('beta', 2.0),
                                 smooth_l1_beta=rk.get('beta', 1.0), box_eps=rk.get('eps', 1e-6),
                                 cls_loss_weight=ck['loss_weight'], reg_loss_weight=rk['loss_weight'], cls_weighted=cw,
                                 reg_weighted=rw)


# ------------------------------------------------------------------------------------------------------- float64 reference
def _box_loss64(kind, p, t, eps):
    """iou_loss.py:105-283 on [K,4] xyxy boxes, float64"""
    lt, rb = torch.max(p[:, :2], t[:, :2]), torch.min(p[:, 2:], t[:, 2:])
    wh = (rb - lt).clamp(min=0)
    overlap = wh[:, 0] * wh[:, 1]
    ap = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
    ag = (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])
    if kind == 'IoULoss':
        union = (ap + ag - overlap).clamp(min=1e-6)
        return -(overlap / union).clamp(min=eps).log()
    union = ap + ag - overlap + eps
    ious = overlap / union
    ewh = (torch.max(p[:, 2:], t[:, 2:]) - torch.min(p[:, :2], t[:, :2])).clamp(min=0)
    if kind == 'GIoULoss':
        earea = ewh[:, 0] * ewh[:, 1] + eps
        return 1 - (ious - (earea - union) / earea)
    c2 = ewh[:, 0] ** 2 + ewh[:, 1] ** 2 + eps
    rho2 = ((t[:, 0] + t[:, 2]) - (p[:, 0] + p[:, 2])) ** 2 / 4 + ((t[:, 1] + t[:, 3]) - (p[:, 1] + p[:, 3])) ** 2 / 4
    if kind == 'DIoULoss':
        return 1 - (ious - rho2 / c2)
    w1, h1 = p[:, 2] - p[:, 0], p[:, 3] - p[:, 1] + eps
    w2, h2 = t[:, 2] - t[:, 0], t[:, 3] - t[:, 1] + eps
    v = (4 / np.pi ** 2) * (torch.atan(w2 / h2) - torch.atan(w1 / h1)) ** 2
    return 1 - (ious - (rho2 / c2 + v ** 2 / (1 - ious + v)))


def _ref64(pc, pr, ct, rt, cls_name, reg_name, decode, cw, rw, grad_scale, sizes=SIZES, strides=STRIDES, ranges=RANGES):
    """lfd.py:300-395 in float64 on the CPU -> ([classification_loss, regression_loss, loss], d cls, d reg, n_pos, row masks);
    the row classification compares the fp32 targets (the thresholds are not what is measured)"""
    ck, rk = CLS_KW[cls_name], REG_KW[reg_name]
    n, P, Cn = ct.shape
    ctf = ct.detach().cpu().reshape(-1, Cn)
    x = pc.detach().cpu().double().reshape(n * P, -1).requires_grad_(True)
    r = pr.detach().cpu().double().reshape(-1, 4).requires_grad_(True)
    rtd, ctd = rt.detach().cpu().double().reshape(-1, 4), ctf.double()
    green = ctf.min(-1)[0] >= 0
    mxf, mi = ctf.max(-1)
    pos = green & (mxf >= 0.001)
    label = torch.where(mxf >= 0.001, mi, torch.full_like(mi, Cn))
    mx = mxf.double()
    n_pos, w_sum = int(pos.sum()), mx[pos].sum()
    onehot = F.one_hot(label, Cn + 1)[:, :Cn].double()
    if cls_name == 'FocalLoss':
        p, g, a = torch.sigmoid(x), ck['gamma'], ck['alpha']
        el = -a * (1 - p) ** g * F.logsigmoid(x) * onehot - (1 - a) * p ** g * F.logsigmoid(-x) * (1 - onehot)
        rows = el.sum(-1)
    elif cls_name == 'CrossEntropyLoss':
        rows = -F.log_softmax(x, -1).gather(1, label[:, None])[:, 0]
    elif cls_name == 'QualityFocalLoss':
        t = onehot * mx[:, None]
        rows = (F.binary_cross_entropy_with_logits(x, t, reduction='none') * (t - torch.sigmoid(x)).abs() ** ck['beta']).sum(-1)
    else:
        rows = F.binary_cross_entropy_with_logits(x, ctd.clamp(min=0), reduction='none').sum(-1)     # (gray rows are masked)
    avg_c = w_sum if cw else n_pos + 1.0
    lc = ck['loss_weight'] * rows[green].sum() / avg_c
    if n_pos == 0:
        lr = r.sum() * 0.0                                  # lfd.py:386-387
    elif reg_name in INDEPENDENT:
        d = (r[pos] - rtd[pos]).abs()
        if reg_name == 'SmoothL1Loss':
            b = rk['beta']
            el = torch.where(d < b, 0.5 * d * d / b, d - 0.5 * b)
        else:
            el = d * d
        lr = rk['loss_weight'] * el.sum() / n_pos
    else:
        xs = torch.cat([(torch.arange(h * w) % w * s).double() for (h, w), s in zip(sizes, strides)]).repeat(n)
        ys = torch.cat([(torch.arange(h * w) // w * s).double() for (h, w), s in zip(sizes, strides)]).repeat(n)
        rmax = torch.cat([torch.full((h * w,), float(max(rg)), dtype=torch.float64) for (h, w), rg in zip(sizes, ranges)]).repeat(n)
        dist = r.exp() if decode == 'exp' else torch.sigmoid(r) * rmax[:, None]

        def boxes(dd):
            return torch.stack([xs - dd[:, 0], ys - dd[:, 1], xs + dd[:, 2], ys + dd[:, 3]], -1)
        el = _box_loss64(reg_name, boxes(dist)[pos], boxes(rtd)[pos], rk['eps'])
        if rw:
            el = el * mx[pos]
        lr = rk['loss_weight'] * el.sum() / (w_sum if rw else float(n_pos))
    loss = lc + lr
    (loss * grad_scale).backward()
    vals = np.array([float(lc.detach()), float(lr.detach()), float(loss.detach())])
    return vals, x.grad.numpy().reshape(n, P, -1), r.grad.numpy().reshape(n, P, 4), n_pos, green.numpy().reshape(n, P), \
        pos.numpy().reshape(n, P)


# ------------------------------------------------------------------------------------------------------- the two routes
def _fused_raw(desc, pc, pr, ct, rt, gout):
    """the four entry points called directly, every output NaN before the launch -> (sums[8], out[8], d cls, d reg)"""
    l = _lib.lib()
    nbytes = l.lfd_get_loss_ex_workspace_bytes()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    sums = torch.full((8,), float('nan'), dtype=torch.float64, device=DEV)
    out = torch.full((8,), float('nan'), dtype=torch.float32, device=DEV)
    gc, gr = torch.full_like(pc, float('nan')), torch.full_like(pr, float('nan'))
    g = torch.tensor(gout, dtype=torch.float32, device=DEV)
    p, st = ops.ptr, ops.stream_ptr()
    with torch.cuda.device(pc.device):
        assert l.lfd_get_loss_ex_sums_f32(C.byref(desc), p(pc), p(pr), p(ct), p(rt), p(ws), nbytes, p(sums), st) == 0
        assert l.lfd_get_loss_ex_finalize_f32(C.byref(desc), p(sums), p(sums), 1.0, p(out), st) == 0
        assert l.lfd_get_loss_ex_bwd_f32(C.byref(desc), p(pc), p(pr), p(ct), p(rt), p(out), p(g), p(gc), p(gr), st) == 0
    return sums, out, gc, gr


def _op_by_op(model, pc, pr, ct, rt, grad_scale):
    c, r = pc.clone().requires_grad_(True), pr.clone().requires_grad_(True)
    pts = model.generate_point_coordinates(model._head_indexes_to_feature_map_sizes)
    out = model._loss_from_targets(c, r, ct, rt, pts)
    (out['loss'] * grad_scale).backward()
    lv = out['loss_values']
    gr = r.grad if r.grad is not None else torch.zeros_like(r)
    return np.array([lv['classification_loss'], lv['regression_loss'], lv['loss']]), c.grad.cpu().numpy(), gr.cpu().numpy()


def _gate(tag, name, fused, op, ref):
    fused, op, ref = (np.asarray(a, dtype=np.float64) for a in (fused, op, ref))
    ef, eo = float(np.abs(fused - ref).max()), float(np.abs(op - ref).max())
    ulp = float(np.spacing(np.float32(np.abs(ref).max())))
    ratio = ef / max(eo, ulp)
    print('%-58s %-4s fused %.3e  op-by-op %.3e  ulp %.3e  ratio %.2f' % (tag, name, ef, eo, ulp, ratio))
    assert ef <= 2 * eo + ulp, (tag, name, ef, eo, ulp)
    return ratio


def _kernel_case(cls_name, reg_name, num_classes, n, decode, cw, rw, seed, sizes=SIZES, strides=STRIDES, ranges=RANGES,
                 no_positive=False):
    tag = '%s+%s C=%d n=%d %s cw=%d rw=%d%s' % (cls_name, reg_name, num_classes, n, decode, cw, rw, ' no-pos' if no_positive else '')
    pc, pr, ct, rt = _inputs(seed, n, num_classes, cls_name, reg_name, decode, sizes, no_positive)
    scale = 1.5
    ref_v, ref_gc, ref_gr, n_pos, green, pos = _ref64(pc, pr, ct, rt, cls_name, reg_name, decode, cw, rw, scale, sizes, strides,
                                                      ranges)
    desc = _desc(n, num_classes, cls_name, reg_name, decode, cw, rw, sizes, strides, ranges)
    sums, out, gc, gr = _fused_raw(desc, pc, pr, ct, rt, [0.0, 0.0, scale])
    sums2, out2, gc2, gr2 = _fused_raw(desc, pc, pr, ct, rt, [0.0, 0.0, scale])
    for a, b in ((sums, sums2), (out, out2), (gc, gc2), (gr, gr2)):
        assert not bool(torch.isnan(a).any()), tag              # every element written
        assert torch.equal(a, b), tag                           # two runs, equal bits
    out, gc, gr = out.cpu().numpy(), gc.cpu().numpy(), gr.cpu().numpy()
    assert out[3] == n_pos and out[6] == green.sum() and bool(pos.any()) != no_positive, tag
    assert not gc[~green].any() and not gr[~green].any(), tag   # gray rows: exactly zero
    assert not gr[~pos].any(), tag                              # non-positive rows: exactly zero regression gradient
    model = _bare_model(LFD, cls_name, reg_name, decode, num_classes, cw, rw, sizes, strides, ranges)
    op_v, op_gc, op_gr = _op_by_op(model, pc, pr, ct, rt, scale)
    assert model.last_loss_route == 'op_by_op'
    if no_positive:
        assert out[1] == 0.0 and not gr.any() and np.isfinite(gc).all() and gc.any(), tag
    ratios = [_gate(tag, nm, f, o, r) for nm, f, o, r in (('Lc', out[0], op_v[0], ref_v[0]), ('Lr', out[1], op_v[1], ref_v[1]),
                                                          ('L', out[2], op_v[2], ref_v[2]), ('dcls', gc, op_gc, ref_gc),
                                                          ('dreg', gr, op_gr, ref_gr))]
    return max(ratios)


# (num_classes, n, decode, classification weight, regression weight): every class count, both batch sizes, both decodes and
# both values of each flag occur
COMBOS = [(1, 2, 'exp', False, False), (3, 3, 'sigmoid', True, True), (5, 2, 'sigmoid', False, True), (80, 3, 'exp', True, False)]


@pytest.mark.parametrize('reg_name', sorted(REG_KW))
@pytest.mark.parametrize('cls_name', sorted(CLS_KW))
def test_kernels_against_float64_next_to_the_op_by_op_route(cls_name, reg_name):
    worst = 0.0
    for i, (Cn, n, decode, cw, rw) in enumerate(COMBOS):
        rw = rw and reg_name not in INDEPENDENT         # an independent loss is never row-weighted (not admitted)
        worst = max(worst, _kernel_case(cls_name, reg_name, Cn, n, decode, cw, rw, seed=100 + i))
    print('worst fused / op-by-op error ratio, %s + %s: %.2f' % (cls_name, reg_name, worst))


@pytest.mark.parametrize('cls_name,reg_name', [('QualityFocalLoss', 'GIoULoss'), ('BCEWithLogitsLoss', 'SmoothL1Loss'),
                                               ('CrossEntropyLoss', 'CIoULoss'), ('FocalLoss', 'MSELoss')])
def test_batch_without_a_positive_row(cls_name, reg_name):
    """regression loss exactly 0, an all-zero d reg, a finite d cls (lfd.py:386-387)"""
    _kernel_case(cls_name, reg_name, 3, 2, 'exp', False, False, seed=7, no_positive=True)


def test_second_grid_stride_trip():
    """2 x 300 x 440 = 264,000 rows > 1024 blocks x 256 threads: the last 1,856 rows are a thread's second row (they hold
    positives: _inputs marks the last three rows of the batch)"""
    sizes, strides, ranges = [(300, 440)], (8,), ((4, 512),)
    assert 2 * 300 * 440 > 1024 * 256
    _kernel_case('QualityFocalLoss', 'GIoULoss', 1, 2, 'exp', True, True, seed=11, sizes=sizes, strides=strides, ranges=ranges)


def test_ops_wrappers_equal_the_raw_calls_and_split_the_upstream_gradient():
    pc, pr, ct, rt = _inputs(3, 2, 5, 'BCEWithLogitsLoss', 'DIoULoss', 'sigmoid')
    desc = _desc(2, 5, 'BCEWithLogitsLoss', 'DIoULoss', 'sigmoid', False, True)
    _, out, gc, gr = _fused_raw(desc, pc, pr, ct, rt, [0.0, 0.0, 1.0])
    fin = ops.get_loss_ex_forward(desc, pc, pr, ct, rt)
    assert torch.equal(fin, out) and torch.equal(fin, ops.get_loss_forward(desc, pc, pr, ct, rt))      # dispatch on the descriptor
    g001 = torch.tensor([0.0, 0.0, 1.0], device=DEV)
    a = ops.get_loss_ex_backward(desc, pc, pr, ct, rt, fin, g001)
    b = ops.get_loss_backward(desc, pc, pr, ct, rt, fin, g001)
    assert torch.equal(a[0], gc) and torch.equal(a[1], gr) and torch.equal(b[0], gc) and torch.equal(b[1], gr)
    # d/d classification_loss + d/d regression_loss == d/d loss (both flow through the total)
    c = ops.get_loss_ex_backward(desc, pc, pr, ct, rt, fin, torch.tensor([1.0, 1.0, 0.0], device=DEV))
    assert torch.equal(c[0], gc) and torch.equal(c[1], gr)
    only_c = ops.get_loss_ex_backward(desc, pc, pr, ct, rt, fin, torch.tensor([1.0, 0.0, 0.0], device=DEV))
    assert torch.equal(only_c[0], gc) and not bool(only_c[1].any())
    with pytest.raises(RuntimeError):
        ops.get_loss_ex_forward(_desc(2, 5, 'FocalLoss', 'MSELoss', 'exp', False, True), pc, pr, ct, rt)   # LFD_ERR_UNSUPPORTED


def test_sums_are_deterministic_and_the_normaliser_is_global():
    """test_fused_get_loss_sums_are_deterministic_and_global_normaliser for QualityFocalLoss + GIoULoss: twice the local sums
    as the 'global' vector with rank_scale 2 changes nothing but the + 1 of the classification normaliser"""
    rng = np.random.default_rng(5)
    sizes, strides, ranges = [(40, 40), (20, 20)], [8, 16], [(4, 20), (20, 40)]
    P, n, Cn = 2000, 3, 1
    d = ops.make_loss_desc_ex(n, sizes, strides, ranges, Cn, 'QualityFocalLoss', 'GIoULoss', 'sigmoid')
    ct = torch.from_numpy(np.where(rng.random((n, P, Cn)) < 0.05, rng.random((n, P, Cn)), 0).astype(np.float32)).cuda()
    ct[0, :50] = -1
    rt = torch.from_numpy(rng.uniform(1, 30, (n, P, 4)).astype(np.float32)).cuda()
    pc = torch.from_numpy(rng.normal(0, 2, (n, P, Cn)).astype(np.float32)).cuda()
    pr = torch.from_numpy(rng.normal(0, 1, (n, P, 4)).astype(np.float32)).cuda()
    f1 = ops.get_loss_ex_forward(d, pc, pr, ct, rt)
    f2 = ops.get_loss_ex_forward(d, pc, pr, ct, rt)
    assert torch.equal(f1, f2)
    n_pos = float(f1[3])
    assert n_pos == float(((ct.max(-1)[0] >= 0.001) & (ct.min(-1)[0] >= 0)).sum()) and n_pos > 0
    assert float(f1[6]) == float((ct.min(-1)[0] >= 0).sum())
    g = ops.get_loss_ex_forward(d, pc, pr, ct, rt, reduce_sums=lambda s: s * 2, rank_scale=2.0)
    assert float(g[3]) == 2 * n_pos
    assert float(g[1]) == pytest.approx(float(f1[1]), rel=1e-6)                       # 2 * sum / (2 n_pos)
    assert float(g[0]) == pytest.approx(float(f1[0]) * (n_pos + 1) * 2 / (2 * n_pos + 1), rel=1e-6)


# ------------------------------------------------------------------------------------------------------- route against route
def _random_annotations(rng, n, hw, num_classes, max_boxes):
    ann = []
    for i in range(n):
        k = 0 if i == 1 else max_boxes                                    # image 1 has no boxes
        wh = np.exp(rng.uniform(np.log(6), np.log(120), (k, 2)))
        xy = rng.uniform(0, 1, (k, 2)) * (np.array([hw[1], hw[0]]) - wh).clip(1)
        ann.append((np.concatenate([xy, wh], 1).astype(np.float32), rng.integers(0, num_classes, k).astype(np.int64)))
    return ann


def _get_loss_and_grads(model, cls0, reg0, ann, scale=1.5):
    cls, reg = cls0.clone().requires_grad_(True), reg0.clone().requires_grad_(True)
    out = model.get_loss((cls, reg), ann)
    (out['loss'] * scale).backward()
    return out['loss_values'], cls.grad.cpu().numpy(), reg.grad.cpu().numpy(), model.last_loss_route


ROUTE_PAIRS = [('QualityFocalLoss', 'IoULoss', 'sigmoid', False), ('BCEWithLogitsLoss', 'IoULoss', 'sigmoid', False),
               ('FocalLoss', 'GIoULoss', 'exp', False), ('FocalLoss', 'DIoULoss', 'exp', False),
               ('FocalLoss', 'CIoULoss', 'sigmoid', False), ('CrossEntropyLoss', 'GIoULoss', 'exp', False),
               ('FocalLoss', 'SmoothL1Loss', 'exp', False), ('FocalLoss', 'MSELoss', 'exp', False),
               ('QualityFocalLoss', 'CIoULoss', 'exp', True)]


@pytest.mark.parametrize('cls_name,reg_name,decode,weighted', ROUTE_PAIRS, ids=['-'.join(map(str, r)) for r in ROUTE_PAIRS])
def test_get_loss_with_the_switch_on_and_off(cls_name, reg_name, decode, weighted, monkeypatch):
    import zlib
    rng = np.random.default_rng(zlib.crc32((cls_name + reg_name).encode()))
    hw, n, Cn = (104, 136), 3, 3
    m = _bare_model(LFD, cls_name, reg_name, decode, Cn, weighted, weighted)
    ann = _random_annotations(rng, n, hw, Cn, 8)
    P = sum(h * w for h, w in SIZES)
    ch = Cn + 1 if m._is_ce() else Cn
    cls0 = torch.from_numpy(rng.normal(-2, 2, (n, P, ch)).astype(np.float32)).to(DEV)
    if reg_name in INDEPENDENT:
        reg0 = torch.from_numpy(rng.uniform(0, 0.8, (n, P, 4)).astype(np.float32)).to(DEV)
    else:
        reg0 = torch.from_numpy((rng.normal(0, 0.5, (n, P, 4)) + 3.0 if decode == 'exp' else rng.normal(0, 1, (n, P, 4)))
                                .astype(np.float32)).to(DEV)
    monkeypatch.setenv('LFD_FUSED_LOSS_EX', '1')
    a = _get_loss_and_grads(m, cls0, reg0, ann)
    monkeypatch.setenv('LFD_FUSED_LOSS_EX', '0')
    b = _get_loss_and_grads(m, cls0, reg0, ann)
    assert (a[3], b[3]) == ('ex', 'op_by_op')
    assert a[0]['regression_loss'] > 0 and np.abs(a[2]).max() > 0
    for k in ('loss', 'classification_loss', 'regression_loss'):
        print(k, a[0][k], b[0][k])
        assert a[0][k] == pytest.approx(b[0][k], rel=2e-5), k
    np.testing.assert_allclose(a[1], b[1], rtol=2e-4, atol=1e-9)
    np.testing.assert_allclose(a[2], b[2], rtol=2e-3, atol=1e-9)
    for x, y in ((a[1], b[1]), (a[2], b[2])):
        assert np.array_equal(x == 0, y == 0) or np.abs(x[(x == 0) != (y == 0)]).max() < 1e-12


def test_focal_iou_never_leaves_the_base_kernels(monkeypatch):
    rng = np.random.default_rng(2)
    m = _bare_model(LFD, 'FocalLoss', 'IoULoss', 'sigmoid', 3)
    ann = _random_annotations(rng, 3, (104, 136), 3, 8)
    P = sum(h * w for h, w in SIZES)
    cls0 = torch.from_numpy(rng.normal(-2, 2, (3, P, 3)).astype(np.float32)).to(DEV)
    reg0 = torch.from_numpy(rng.normal(0, 1, (3, P, 4)).astype(np.float32)).to(DEV)
    monkeypatch.setenv('LFD_FUSED_LOSS_EX', '1')
    a = _get_loss_and_grads(m, cls0, reg0, ann)
    monkeypatch.setenv('LFD_FUSED_LOSS_EX', '0')
    b = _get_loss_and_grads(m, cls0, reg0, ann)
    assert a[3] == b[3] == 'base' and a[0] == b[0] and a[0]['regression_loss'] > 0
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


# ------------------------------------------------------------------------------------------------------- the real reference
def _golden_gate(tag, name, fused, op, ref, relative=False):
    fused, op, ref = (np.asarray(a, dtype=np.float64) for a in (fused, op, ref))
    den = np.abs(ref) if relative else 1.0
    ef, eo = float((np.abs(fused - ref) / den).max()), float((np.abs(op - ref) / den).max())
    print('%s %-20s error against the reference: fused %.3e  op-by-op %.3e' % (tag, name, ef, eo))
    return name, ef, eo


def _assert_golden(rows):
    bad = [(n, ef, eo) for n, ef, eo in rows if not ef <= 2 * eo]
    assert not bad, bad


def test_tl_lfd_l_qfl_iou_against_the_reference(monkeypatch):
    """ref_train_step_TL_LFD_L.npz: the reference's predictions, its three loss values of iteration 1 and its d cls / d reg"""
    g = load_golden('ref_train_step_TL_LFD_L.npz')
    m = configs.build_model('TL_LFD_L').to(DEV)
    for i, s in enumerate(g['sizes'].tolist()):
        m._head_indexes_to_feature_map_sizes[i] = tuple(s)
    ann = TSC.annotations('TL_LFD_L', 1)
    cls0, reg0 = torch.from_numpy(g['cls']).to(DEV), torch.from_numpy(g['reg']).to(DEV)
    monkeypatch.setenv('LFD_FUSED_LOSS_EX', '1')
    a = _get_loss_and_grads(m, cls0, reg0, ann, scale=1.0)
    monkeypatch.setenv('LFD_FUSED_LOSS_EX', '0')
    b = _get_loss_and_grads(m, cls0, reg0, ann, scale=1.0)
    assert (a[3], b[3]) == ('ex', 'op_by_op')
    want = dict(zip(('loss', 'classification_loss', 'regression_loss'), g['losses'][0]))
    rows = [_golden_gate('TL_LFD_L', k, a[0][k], b[0][k], want[k], relative=True) for k in want]
    rows += [_golden_gate('TL_LFD_L', 'dcls', a[1], b[1], g['dcls']), _golden_gate('TL_LFD_L', 'dreg', a[2], b[2], g['dreg'])]
    _assert_golden(rows)


def test_lfdv2_sfpn_focal_giou_against_the_reference(ex_on):
    """ref_sibling_LFDV2_SFPN.npz: the reference's predictions AND targets, its loss values and prediction gradients"""
    g = load_golden('ref_sibling_LFDV2_SFPN.npz')
    m = configs.build_sibling_model('LFDV2_SFPN', seed=1).to(DEV)
    for i, s in enumerate(g['sizes'].tolist()):
        m._head_indexes_to_feature_map_sizes[i] = tuple(s)
    ct, rt = torch.from_numpy(g['cls_target']).to(DEV), torch.from_numpy(g['reg_target']).to(DEV)
    res = []
    for fused in (True, False):
        cls = torch.from_numpy(g['cls']).to(DEV).requires_grad_(True)
        reg = torch.from_numpy(g['reg']).to(DEV).requires_grad_(True)
        if fused:
            out = m._get_loss_fused(cls, reg, ct, rt)
        else:
            out = m._loss_from_targets(cls, reg, ct, rt, m.generate_point_coordinates(m._head_indexes_to_feature_map_sizes))
        out['loss'].backward()
        res.append((out['loss_values'], cls.grad.cpu().numpy(), reg.grad.cpu().numpy(), m.last_loss_route))
    a, b = res
    assert (a[3], b[3]) == ('ex', 'op_by_op')
    want = json.loads(str(g['loss_values']))
    rows = [_golden_gate('LFDV2_SFPN', k, a[0][k], b[0][k], want[k], relative=True) for k in sorted(want)]
    rows += [_golden_gate('LFDV2_SFPN', 'dcls', a[1], b[1], g['dcls']), _golden_gate('LFDV2_SFPN', 'dreg', a[2], b[2], g['dreg'])]
    _assert_golden(rows)


# ------------------------------------------------------------------------------------------------------- integration
def _named_model_after_one_get_loss(name):
    if name == 'TL_LFD_L':
        g, m = load_golden('ref_train_step_TL_LFD_L.npz'), configs.build_model('TL_LFD_L').to(DEV)
        ann = TSC.annotations('TL_LFD_L', 1)
    else:
        g, m = load_golden('ref_sibling_LFDV2_SFPN.npz'), configs.build_sibling_model('LFDV2_SFPN', seed=1).to(DEV)
        n, H, W = [int(v) for v in g['shape']]
        ann = SC.synth_annotations(5, n, H, W, 4)
    for i, s in enumerate(g['sizes'].tolist()):
        m._head_indexes_to_feature_map_sizes[i] = tuple(s)
    assert m.last_loss_route is None
    m.get_loss((torch.from_numpy(g['cls']).to(DEV), torch.from_numpy(g['reg']).to(DEV)), ann)
    return m.last_loss_route


def test_named_models_report_the_fused_route(monkeypatch):
    """TL_LFD_L (QFL + IoU, a shipped configuration) takes the fused route with the switch unset; LFDV2_SFPN (Focal + GIoU, a
    composition no shipped configuration uses) with LFD_FUSED_LOSS_EX=1, and stays op by op without it"""
    monkeypatch.delenv('LFD_FUSED_LOSS_EX', raising=False)
    monkeypatch.delenv('LFD_FUSED_LOSS', raising=False)
    assert _named_model_after_one_get_loss('TL_LFD_L') == 'ex'
    assert _named_model_after_one_get_loss('LFDV2_SFPN') == 'op_by_op'
    monkeypatch.setenv('LFD_FUSED_LOSS_EX', '1')
    assert _named_model_after_one_get_loss('TL_LFD_L') == 'ex'
    assert _named_model_after_one_get_loss('LFDV2_SFPN') == 'ex'
    monkeypatch.setenv('LFD_FUSED_LOSS_EX', '0')
    assert _named_model_after_one_get_loss('TL_LFD_L') == 'op_by_op'


def test_lfdv2_takes_device_annotations(ex_on):
    m = _bare_model(LFDv2, 'FocalLoss', 'GIoULoss', 'exp', 3, mode='sqrt')
    rng = np.random.default_rng(9)
    host = _random_annotations(rng, 3, (104, 136), 3, 6)
    da = DeviceAnnotations(3, 32, DEV)
    k = 0
    offs = [0]
    for b, l in host:
        da.boxes[k:k + len(b)] = torch.from_numpy(b).to(DEV)
        da.labels[k:k + len(l)] = torch.from_numpy(l).to(DEV)
        k += len(b)
        offs.append(k)
    da.boxes[k:] = 1e4                                   # rows beyond offsets[n] are unspecified: never read
    da.offsets.copy_(torch.tensor(offs, dtype=torch.int32))
    P = sum(h * w for h, w in SIZES)
    cls0 = torch.from_numpy(rng.normal(-2, 2, (3, P, 3)).astype(np.float32)).to(DEV)
    reg0 = torch.from_numpy((rng.normal(0, 0.5, (3, P, 4)) + 3.0).astype(np.float32)).to(DEV)
    a = _get_loss_and_grads(m, cls0, reg0, da)
    b = _get_loss_and_grads(m, cls0, reg0, da.to_host())
    assert a[3] == b[3] == 'ex' and a[0] == b[0] and a[0]['regression_loss'] > 0
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def _xs_qfl_giou(state=None):
    m = configs.build_model('WIDERFACE_LFD_XS')
    m._classification_loss_func = L.QualityFocalLoss(beta=2.0, loss_weight=2.0)
    m._regression_loss_func = L.GIoULoss(eps=1e-6, loss_weight=1.0)
    if state is not None:
        m.load_state_dict(state)
    return m.to(DEV).train()


def test_graphed_train_step_captures_a_qfl_giou_network(ex_on):
    rng = np.random.default_rng(4)
    ma = _xs_qfl_giou()
    state = copy.deepcopy(ma.state_dict())
    kw = dict(lr=0.02, momentum=0.9, weight_decay=1e-4)
    clip = dict(max_norm=10, norm_type=2)
    batches = [(torch.from_numpy(rng.normal(0, 1, (2, 3, 96, 128)).astype(np.float32)).to(DEV),
                [(np.array([[10., 12., 30., 40.], [60., 20., 50., 44.]], np.float32) + i, np.zeros(2, np.int64)),
                 (np.array([[40., 30., 24., 20.]], np.float32), np.zeros(1, np.int64))]) for i in range(4)]
    oa = optim.SGD(ma.parameters(), **kw)
    eager = [train.train_step(ma, oa, x, ann, clip, True)[0] for x, ann in batches]
    assert ma.last_loss_route == 'ex'
    graphed = []
    for _ in range(2):
        mb = _xs_qfl_giou(state)
        ob = optim.SGD(mb.parameters(), **kw)
        step = train.GraphedTrainStep(mb, ob, clip, max_boxes=16)
        graphed.append([step(x, ann, True)[0] for x, ann in batches])
        assert len(step.graphs) == 1                      # first call eager, second captured, two replays
    assert graphed[0] == graphed[1]                       # bit-equal between two graphed runs
    for it, (e, g) in enumerate(zip(eager, graphed[0])):
        print(it, e, g)
        for k in ('loss', 'classification_loss', 'regression_loss'):
            assert g[k] == pytest.approx(e[k], rel=2e-5), (it, k)
    assert eager[0]['regression_loss'] > 0


def test_lfdv2_sfpn_trains_on_the_fused_loss(ex_on):
    model = configs.build_sibling_model('LFDV2_SFPN', seed=1).to(DEV).train()
    x = (torch.rand(2, 3, 96, 128, generator=torch.Generator().manual_seed(7)) * 2 - 1).to(DEV)
    ann = SC.synth_annotations(5, 2, 96, 128, 4)
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        lo = model.get_loss(model(x), ann)
        lo['loss'].backward()
        opt.step()
        losses.append(lo['loss_values']['loss'])
    print('LFDV2_SFPN losses on the fused get_loss', losses)
    assert model.last_loss_route == 'ex'
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
