"""The 'fp32_storage' precision mode of FCOS / LFDv2 and of LFD over FPN-family necks (lfd_amd/engine_sibling_p32.py,
csrc/precise_pyramid.hip, the merge instantiation of csrc/precise.hip) against the reference's fp32 tensors
(tests/golden/ref_sibling_*.npz: lfd/model/fcos.py:414-449, lfdv2.py:671-702 on 2 x 3 x 128 x 160 frames).

  * element-wise kernels: bit-equal to fp32 ATen on the CPU (expf: within 4 ulp -- each side's expf is good to ~1 ulp, doubled);
  * the merge conv: bit-equal to lfd_p32_conv2d_nhwc_f32 + lfd_p32_upsample_nearest_add_f32, and within 3e-6 * max(1, max|ref|)
    of float64 -- the bound tests/test_gpu_precise.py::test_p32_conv_vs_float64 holds the same kernel to, same distributions;
  * whole models: the mode's gates (tests/test_gpu_precise.py:172-173) -- cls / centerness / LFDv2 reg within 1e-4 absolute, FCOS
    distances within 1e-4 relative, sigmoid(cls) / sigmoid(centerness) within 1e-3; LFD_P32_MERGE 0 == 1, graph replay == eager,
    back to 'fp16' == the 'fp16' bits; get_results rows == the reference's for FCOS_FPN and LFDV2_SFPN (the two fixtures whose
    kept rows do not move under a 1e-4 perturbation of the logits).
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from lfd_amd import _lib, configs, engine_p32
from lfd_amd._lib import check, lib, ptr, stream_ptr
from test_sibling_oracle_golden import NAMES, assert_results_equal, model_input

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


# ----------------------------------------------------------------------------------------------- element-wise kernels
def _upadd(dst, src):
    n, H, W, c = dst.shape
    check(lib().lfd_p32_upsample_nearest_add_f32(ptr(dst), ptr(src), n, H, W, src.shape[1], src.shape[2], c, stream_ptr()),
          'lfd_p32_upsample_nearest_add_f32')
    torch.cuda.synchronize()
    return dst


@pytest.mark.parametrize('c', [64, 128])
@pytest.mark.parametrize('shape', [((12, 16), (6, 8)), ((13, 17), (7, 9)), ((7, 9), (4, 5)), ((5, 5), (1, 1)), ((6, 8), (6, 8))])
def test_p32_upsample_nearest_add_equals_aten(shape, c):
    (H, W), (h, w) = shape
    g = torch.Generator().manual_seed(3)
    dst = torch.randn(2, H, W, c, generator=g)
    src = torch.randn(2, h, w, c, generator=g)
    ref = dst.permute(0, 3, 1, 2) + F.interpolate(src.permute(0, 3, 1, 2), size=(H, W), mode='nearest')
    got = _upadd(dst.to(DEV).contiguous(), src.to(DEV).contiguous())
    assert torch.equal(got.cpu(), ref.permute(0, 2, 3, 1))


def test_p32_relu_and_maxpool_equal_aten():
    g = torch.Generator().manual_seed(4)
    x = torch.randn(2, 9, 11, 128, generator=g)
    xd = x.to(DEV)
    check(lib().lfd_p32_relu_f32(ptr(xd), xd.numel(), stream_ptr()), 'lfd_p32_relu_f32')
    assert torch.equal(xd.cpu(), x.relu())
    for src in (x, torch.randn(2, 1, 1, 64, generator=g)):
        n, h, w, c = src.shape
        sd = src.to(DEV)
        out = torch.full((n, (h + 1) // 2, (w + 1) // 2, c), 7.0, device=DEV)
        check(lib().lfd_p32_maxpool3x3s2_f32(ptr(sd), ptr(out), n, h, w, c, stream_ptr()), 'lfd_p32_maxpool3x3s2_f32')
        ref = F.max_pool2d(src.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
        assert torch.equal(out.cpu(), ref)


def test_p32_exp_rows_touches_only_its_slice():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 100, 4, generator=g) * 3
    xd = x.to(DEV)
    check(lib().lfd_p32_exp_rows_f32(ptr(xd), 2, 400, 20, 35, 4, stream_ptr()), 'lfd_p32_exp_rows_f32')
    got = xd.cpu()
    assert torch.equal(got[:, :20], x[:, :20]) and torch.equal(got[:, 55:], x[:, 55:])
    ref = x[:, 20:55].exp()
    ulp = (torch.nextafter(ref, ref.new_full((), float('inf'))) - ref).double()
    err = ((got[:, 20:55].double() - ref.double()).abs() / ulp).max()
    print('exp rows: %.2f ulp' % float(err))
    assert float(err) <= 4


# ----------------------------------------------------------------------------------------------- merge conv
def _p32_conv(x, wp, bp, cout, relu, up=None):
    n, h, w, cin = x.shape
    out = torch.empty((n, h, w, cout), dtype=torch.float32, device=DEV)
    d = _lib.P32ConvDesc(n, h, w, cin, cout, 1, 1, int(relu), -1, 0, 0)
    if up is None:
        check(lib().lfd_p32_conv2d_nhwc_f32(C.byref(d), ptr(x), ptr(out), ptr(wp), ptr(bp), None, None, stream_ptr()),
              'lfd_p32_conv2d_nhwc_f32')
    else:
        check(lib().lfd_p32_conv2d_merge_nhwc_f32(C.byref(d), ptr(x), ptr(out), ptr(wp), ptr(bp), ptr(up), up.shape[1], up.shape[2],
                                                  stream_ptr()), 'lfd_p32_conv2d_merge_nhwc_f32')
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('cin,cout', [(64, 64), (64, 128), (128, 128), (128, 64)])
def test_p32_merge_conv_equals_conv_plus_upsample_add_and_float64(cin, cout):
    """17 columns cross the 16-wide tile, 13 rows the 8-row tile of the 1x1 kernel; 5 x 5 <- 1 x 1 is the smallest pyramid step"""
    for (H, W), (h, w) in (((13, 17), (7, 9)), ((5, 5), (1, 1))):
        for relu in (True, False):
            g = torch.Generator().manual_seed(cin * 1000 + cout * 10 + H + int(relu))
            x = torch.randn(2, H, W, cin, generator=g) * 2
            wt = torch.randn(cout, cin, 1, 1, generator=g) * (1.0 / cin ** 0.5)
            b = torch.randn(cout, generator=g)
            up = torch.randn(2, h, w, cout, generator=g)
            xd, upd = x.to(DEV), up.to(DEV)
            wp, bp = engine_p32.pack_weight(wt).to(DEV), engine_p32._pad_bias(b).to(DEV)
            fused = _p32_conv(xd, wp, bp, cout, relu, up=upd)
            two = _upadd(_p32_conv(xd, wp, bp, cout, relu), upd)
            assert torch.equal(fused, two), (H, W, relu)
            y = F.conv2d(x.double().permute(0, 3, 1, 2), wt.double(), b.double())
            y = (y.relu() if relu else y) + F.interpolate(up.double().permute(0, 3, 1, 2), size=(H, W), mode='nearest')
            ref = y.permute(0, 2, 3, 1)
            err, mag = float((fused.cpu().double() - ref).abs().max()), float(ref.abs().max())
            print('p32 merge conv %d->%d %dx%d relu %d: err %.2e (max |y| %.2f)' % (cin, cout, H, W, relu, err, mag))
            assert err <= 3e-6 * max(1.0, mag)


def test_p32_merge_conv_validates_arguments():
    """argument checks happen on the host, before anything touches a device: the pointers below are host memory"""
    buf = (C.c_char * 128)()
    base = (C.addressof(buf) + 15) & ~15
    x, out, up, w = (C.c_void_p(base + 16 * k) for k in range(4))
    l = lib()
    assert l.lfd_p32_conv2d_merge_nhwc_f32(None, None, None, None, None, None, 1, 1, None) == -1
    d = _lib.P32ConvDesc(1, 8, 8, 64, 64, 3, 1, 1, -1, 0, 0)
    assert l.lfd_p32_conv2d_merge_nhwc_f32(C.byref(d), x, out, w, w, up, 4, 4, None) == -4     # a 3x3 is no lateral
    d = _lib.P32ConvDesc(1, 8, 8, 64, 64, 1, 1, 1, -1, 0, 0)
    assert l.lfd_p32_conv2d_merge_nhwc_f32(C.byref(d), x, out, w, w, up, 9, 4, None) == -1     # up larger than the map
    assert l.lfd_p32_conv2d_merge_nhwc_f32(C.byref(d), x, x, w, w, up, 4, 4, None) == -1       # in place
    assert l.lfd_p32_conv2d_merge_nhwc_f32(C.byref(d), x, out, w, w, out, 4, 4, None) == -1    # up is the output
    for k in range(3):                                                                         # in / out / up 4 bytes off
        ptrs = [x, out, up]
        ptrs[k] = C.c_void_p(ptrs[k].value + 4)
        assert l.lfd_p32_conv2d_merge_nhwc_f32(C.byref(d), ptrs[0], ptrs[1], w, w, ptrs[2], 4, 4, None) == -1


# ----------------------------------------------------------------------------------------------- whole models
def _lfd_over_sfpn():
    """LFD over the LFDV2_SFPN modules, as tests/test_gpu_siblings.py::test_lfd_meta_architecture_accepts_the_sibling_modules"""
    from lfd_amd.model import LFD
    v2 = configs.build_sibling_model('LFDV2_SFPN', seed=1).eval().to(DEV)
    spec = configs.SIBLINGS['LFDV2_SFPN']
    return LFD(backbone=v2._backbone, neck=v2._neck, head=v2._head, num_classes=spec['head']['num_classes'],
               regression_ranges=spec['regression_ranges'], range_assign_mode='dist', point_strides=v2._point_strides,
               classification_loss_func=v2._classification_loss_func, regression_loss_func=v2._regression_loss_func,
               distance_to_bbox_mode=spec['distance_to_bbox_mode']).eval()


@functools.lru_cache(maxsize=None)
def _runs(name):
    """every forward the tests below compare, once per model: 'fp16', 'fp32_storage' (LFD_P32_MERGE 1 and 0, eager and graph
    replay), 'fp16' again"""
    fixture = 'LFDV2_SFPN' if name == 'LFD_SFPN' else name
    g = load_golden('ref_sibling_%s.npz' % fixture)
    model = _lfd_over_sfpn() if name == 'LFD_SFPN' else configs.build_sibling_model(name, seed=1).eval().to(DEV)
    x = model_input(g).to(DEV)
    r = dict(g=g, model=model)
    prev = os.environ.get('LFD_P32_MERGE')
    try:
        with torch.no_grad():
            r['fp16'] = [o.clone() for o in model(x)]
            model.precision = 'fp32_storage'
            os.environ['LFD_P32_MERGE'] = '1'
            r['p32'] = [o.clone() for o in model(x)]
            r['sizes'] = [tuple(model.head_indexes_to_feature_map_sizes[i]) for i in range(len(g['sizes']))]
            os.environ['LFD_P32_MERGE'] = '0'
            r['p32_two_launch'] = [o.clone() for o in model(x)]
            os.environ['LFD_P32_MERGE'] = '1'
            model.use_graph = True
            for _ in range(2):                       # capture, then a pure replay
                r['p32_graph'] = [o.clone() for o in model(x)]
            model.use_graph = False
            model.precision = 'fp16'
            r['fp16_again'] = [o.clone() for o in model(x)]
    finally:
        if prev is None:
            os.environ.pop('LFD_P32_MERGE', None)
        else:
            os.environ['LFD_P32_MERGE'] = prev
    return r


@pytest.mark.parametrize('name', NAMES + ['LFD_SFPN'])
def test_sibling_fp32_storage_forward_vs_reference(name):
    r = _runs(name)
    g, outs = r['g'], r['p32']
    assert [list(s) for s in r['sizes']] == g['sizes'].tolist()
    keys = ('cls', 'reg', 'ctr')[:len(outs)]
    for key, o in zip(keys, outs):
        ref = g[key]
        assert tuple(o.shape) == ref.shape and o.dtype == torch.float32
        got = o.cpu().numpy()
        if key == 'reg' and name.startswith('FCOS'):      # exp(scale * conv): the logit error is the distance's relative error
            err = np.abs(got - ref) / np.abs(ref)
        else:
            err = np.abs(got - ref)
        print('fp32_storage %s %s: max %.2e mean %.2e' % (name, key, err.max(), err.mean()))
        assert err.max() <= 1e-4, (key, err.max())
        if key in ('cls', 'ctr'):
            sg = np.abs(1 / (1 + np.exp(-got.astype(np.float64))) - 1 / (1 + np.exp(-ref.astype(np.float64))))
            print('fp32_storage %s sigmoid(%s): max %.2e' % (name, key, sg.max()))
            assert sg.max() <= 1e-3, (key, sg.max())


@pytest.mark.parametrize('name', NAMES + ['LFD_SFPN'])
def test_sibling_fp32_storage_routes_agree_bit_for_bit(name):
    """the fused merge == conv + upsample-add; graph replay == eager launches; the mode switch really switches, and back"""
    r = _runs(name)
    for a, b, c in zip(r['p32'], r['p32_two_launch'], r['p32_graph']):
        assert torch.equal(a, b) and torch.equal(a, c)
    for a, b in zip(r['fp16'], r['fp16_again']):
        assert torch.equal(a, b)
    d = float((r['fp16'][0] - r['p32'][0]).abs().max())
    assert 1e-6 < d < 5e-2, d


@pytest.mark.parametrize('name', ['FCOS_FPN', 'LFDV2_SFPN'])
def test_sibling_fp32_storage_get_results_equal_reference_rows(name):
    r = _runs(name)
    g, model = r['g'], r['model']
    n, H, W = [int(v) for v in g['shape']]
    thr, iou = model._classification_threshold, model._nms_cfg
    model._classification_threshold = float(g['results_thr'])
    model._nms_cfg = dict(type='nms', iou_thr=float(g['results_iou']))
    try:
        for key, (hh, ww, sc) in (('results', (H, W, 1.0)), ('results_scaled', (H - 6, W - 10, 0.5))):
            res = model.get_results(tuple(r['p32']), [dict(resized_height=hh, resized_width=ww, resize_scale=sc)] * n)
            ref = json.loads(str(g[key]))
            for i in range(n):
                assert len(ref[i]) > 3
                assert_results_equal(res[i], ref[i])
    finally:
        model._classification_threshold, model._nms_cfg = thr, iou
