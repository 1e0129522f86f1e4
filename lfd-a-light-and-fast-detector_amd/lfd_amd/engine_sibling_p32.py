"""'fp32_storage' precision mode of the sibling meta-architectures: FCOS (lfd/model/fcos.py:414-449), LFDv2
(lfd/model/lfdv2.py:671-702) and LFD itself over the modules its constructor allows next to the shipped ones -- an FPN /
SimpleFPN neck (lfd/model/neck/fpn.py:127-152, simple_fpn.py:141-172) under an LFDHead of 1x1 or 3x3 towers, an FCOSHead
(lfd/model/head/fcos_head.py:129-154) or an LFDHeadV1 (lfd_head.py:164-185).  SimpleNeck + LFDHead, whatever the tower kernel
size, stays on engine_p32 (`covers`).  `model.precision = 'fp32_storage'` selects the mode; raw logits within 1e-4 of the
reference's fp32 tensors (tests/test_gpu_sibling_precise.py).

It is engine_sibling.SiblingPlan layer for layer on the kernels of engine_p32 -- the fp32-tensor form of the mode: every
inter-layer tensor dense fp32 NHWC, one launch per conv (csrc/precise.hip: exact hi/lo operand split, three MFMAs per
k-step, fp32 epilogue), eval BatchNorm folded in float64, GroupNorm (+ ReLU) by lfd_p32_groupnorm_relu_f32:

  backbone             engine_p32.PrecisePlan._build_backbone (the launches of LFD's plan, unchanged)
  lateral + merge      lfd_p32_conv2d_merge_nhwc_f32: conv 1x1 (+ BN, + ReLU) with `+= nearest(coarser level)` in its epilogue,
                       laterals walked from the coarsest level down; LFD_P32_MERGE=0 (host switch, read when a plan is
                       built, like LFD_P32_TAIL), a GroupNorm lateral or `neighbouring_mode`: conv, then
                       lfd_p32_upsample_nearest_add_f32 -- the same fp32 operations in the same order, the same bits
  extra levels         lfd_p32_relu_f32 (in place: rewrites the level it reads), conv 3x3 s2 | lfd_p32_maxpool3x3s2_f32
  output convs         lfd_p32_conv2d_nhwc_f32 writing straight into the level-concatenated cls / reg / centerness tensors
                       (out_pixel_stride / out_image_stride), Scale as a device scalar in its epilogue;
                       FCOSHead's exp: lfd_p32_exp_rows_f32 on the level's rows

A plane-form (hi/lo) pyramid path does not exist; this form is the mode's documented fallback with the same tolerance.
No PyTorch fallback: an unsupported module raises engine.Unsupported.
"""
import ctypes as C
import os

import torch
import torch.nn as nn

from . import _lib, engine, engine_p32, netdesc
from ._lib import check, ptr


def merge_enabled():
    """host-side A/B switch (tests, tools): LFD_P32_MERGE=0 runs a merged lateral as conv + upsample-add (two launches)"""
    return os.environ.get('LFD_P32_MERGE', '1') != '0'


def covers(model):
    """True when this plan, not engine_p32's, runs the model's fp32_storage forward: anything but SimpleNeck + LFDHead"""
    return type(model._neck).__name__ != 'SimpleNeck' or type(model._head).__name__ != 'LFDHead'


_LAUNCH = {'gn': 'lfd_p32_groupnorm_relu_f32', 'merge': 'lfd_p32_conv2d_merge_nhwc_f32',
           'upadd': 'lfd_p32_upsample_nearest_add_f32', 'relu': 'lfd_p32_relu_f32', 'pool': 'lfd_p32_maxpool3x3s2_f32',
           'exp': 'lfd_p32_exp_rows_f32'}


def _steps(seq):
    try:
        return netdesc.split_sequential(seq)
    except netdesc.UnknownModule as e:       # this mode raises engine.Unsupported like engine_p32
        engine._unsupported(str(e))


class SiblingPrecisePlan(engine_p32.PrecisePlan):
    """launch plan for one (module tree, parameter version, LFD_P32_MERGE); interface of engine_p32.PrecisePlan"""

    def __init__(self, model, device, merge=None):
        self.merge = merge_enabled() if merge is None else bool(merge)
        super().__init__(model, device)

    def level_bufs(self):
        return self.feats

    def launch_names(self):
        """the entry point of every launch, in order (tests, tools)"""
        return [_LAUNCH.get(o.kind) or ('lfd_p32_conv2d_tail_nhwc_f32' if o.tail is not None else 'lfd_p32_conv2d_nhwc_f32')
                for o in self.ops]

    # ------------------------------------------------------------------ building blocks
    def _simple(self, kind, src, dst=None, out=None, level=None):
        o = engine_p32._Op()
        o.kind, o.src, o.dst, o.out, o.level = kind, src, dst, out, level
        self.ops.append(o)

    def _layer(self, src, conv, norm, relu, up=None, scale=None, out=None, level=None):
        """conv [+ eval BatchNorm folded] [+ GroupNorm] [+ ReLU] on buffer `src`; up: buffer of the coarser level to merge
        in the epilogue; out / level: write the level's rows of an output tensor instead of a new buffer"""
        if not isinstance(conv, nn.Conv2d):
            engine._unsupported('expected nn.Conv2d, got %s' % type(conv).__name__)
        ks, st = conv.kernel_size[0], conv.stride[0]
        if conv.kernel_size != (ks, ks) or conv.stride != (st, st) or conv.padding != (ks // 2, ks // 2) \
                or ks not in (1, 3) or st not in (1, 2) or conv.groups != 1 or conv.dilation != (1, 1):
            engine._unsupported('conv %s' % (conv,))
        gn = norm if isinstance(norm, nn.GroupNorm) else None
        if norm is not None and gn is None and not isinstance(norm, nn.BatchNorm2d):
            engine._unsupported('norm %s' % type(norm).__name__)
        cin_have = self.buf_channels[src]
        # towers shared between levels (FCOSHead, share_head_flag) are folded, packed and uploaded once per plan
        shared = self.__dict__.setdefault('_packed', {})
        key = (id(conv), id(norm), cin_have, out is None)
        if key in shared and up is None:
            first = shared[key]
            dst = self._conv(src, first.ref_w, None, ks, st, relu and gn is None, scale=scale, out=out, level=level,
                             packed=(first.w, first.b))
            if gn is not None:
                g0, o = shared[key, 'gn'], engine_p32._Op()
                o.kind, o.src, o.relu = 'gn', dst, int(relu)
                o.gamma, o.beta, o.eps, o.groups = g0.gamma, g0.beta, g0.eps, g0.groups
                self.ops.append(o)
            return dst
        w, b = engine._fold_conv_norm(conv, None if gn is not None else norm)
        cout = w.shape[0]
        if out is None:
            cout = engine.pad_channels(max(cout, 32))       # a consumer reads 32-channel chunks; padded channels stay 0
            if cout > 128:
                engine._unsupported('neck / head convs with more than 128 output channels (%d)' % w.shape[0])
        if gn is not None:
            g = int(gn.num_groups)
            if cout != w.shape[0] or 256 % (cout // 4) or g > 64 or cout % g or (cout // g) % 4 or gn.weight is None:
                engine._unsupported('GroupNorm(%d, %d) in the fp32_storage mode' % (g, w.shape[0]))
        if w.shape[1] > cin_have:
            engine._unsupported('conv reads %d channels of a %d-channel map' % (w.shape[1], cin_have))
        wp = w.new_zeros((cout, cin_have, ks, ks))
        wp[:w.shape[0], :w.shape[1]] = w
        bp = b.new_zeros(cout)
        bp[:b.shape[0]] = b
        dst = self._conv(src, wp, bp, ks, st, relu and gn is None, scale=scale, out=out, level=level)
        if up is not None:
            # relu?(conv + bias) + nearest(up): `res` names the coarser level's buffer
            self.ops[-1].kind, self.ops[-1].res = 'merge', up
        else:
            shared[key] = self.ops[-1]
        if gn is not None:
            self._gn(dst, gn, relu=relu)
            shared[key, 'gn'] = self.ops[-1]
        return dst

    def _path(self, steps, src, scale=None, out=None, level=None):
        """the steps (netdesc.split_sequential) of an nn.Sequential of [conv, (norm), (ReLU)] groups / bare in-place ReLU /
        MaxPool2d(3, 2, 1) from buffer `src`; out: its last conv writes the level's rows of that output tensor (with `scale`
        in its epilogue)"""
        if out is not None and (not steps or not isinstance(steps[-1], netdesc.Layer) or isinstance(steps[-1].norm, nn.GroupNorm)):
            engine._unsupported('a head path must end in its output conv')
        cur = src
        for k, s in enumerate(steps):
            if s == 'relu':
                self._simple('relu', cur)       # nn.ReLU(inplace=True): the tensor it reads changes too (by design)
            elif s == 'pool':
                dst = self._new_buf(self.buf_channels[cur], self.buf_scale[cur] * 2)
                self._simple('pool', cur, dst)
                cur = dst
            else:
                last = out is not None and k == len(steps) - 1
                cur = self._layer(cur, s.conv, s.norm, s.relu, scale=scale if last else None, out=out if last else None,
                                  level=level if last else None)
        return cur

    # ------------------------------------------------------------------ neck
    def _build_neck(self, neck):
        kind = type(neck).__name__
        if kind == 'SimpleNeck':
            return [self._path(_steps(getattr(neck, 'neck%d' % i)), t) for i, t in enumerate(self.taps)]
        if kind not in ('FPN', 'SimpleFPN'):
            engine._unsupported('neck %s' % kind)
        ni, no = neck._num_inputs, neck._num_outputs
        if ni != len(self.taps):
            engine._unsupported('neck with %d inputs on %d backbone taps' % (ni, len(self.taps)))
        bottom_up = bool(getattr(neck, '_neighbouring_mode', False))
        lat = [None] * ni
        # top-down: lateral[i-1] += up(lateral[i]) walking from the coarsest level, so each merge reads an already-merged map
        for i in range(ni - 1, -1, -1):
            steps = _steps(getattr(neck, 'lateral%d' % i))
            merged = not bottom_up and i < ni - 1
            one = steps[0] if len(steps) == 1 and isinstance(steps[0], netdesc.Layer) else None
            fuse = merged and self.merge and one is not None and one.conv.kernel_size == (1, 1) and one.conv.stride == (1, 1) \
                and not isinstance(one.norm, nn.GroupNorm)
            if fuse:
                lat[i] = self._layer(self.taps[i], one.conv, one.norm, one.relu, up=lat[i + 1])
            else:
                lat[i] = self._path(steps, self.taps[i])
                if merged:
                    self._simple('upadd', lat[i + 1], lat[i])
        if bottom_up:       # simple_fpn.py:147-151 neighbouring_mode: from the finest level, each reads its UNmerged neighbour
            for i in range(ni - 1):
                self._simple('upadd', lat[i + 1], lat[i])
        outs = []
        for i in range(no):
            if i == ni:
                src = self.taps[-1] if neck._extra_on_input else outs[-1]
            elif i > ni:
                src = outs[-1]
            else:
                src = lat[i]
            outs.append(self._path(_steps(getattr(neck, 'fpn_out%d' % i)), src))
        return outs

    # ------------------------------------------------------------------ head
    def _scale(self, scale):
        return scale._scale.detach().float().reshape(1).to(self.device)

    def _build_head(self, head, feats):
        kind = type(head).__name__
        if head._num_heads != len(feats):
            engine._unsupported('head with %d levels on %d neck outputs' % (head._num_heads, len(feats)))
        self.num_levels = head._num_heads
        if kind == 'FCOSHead':
            self.has_ctr = True
            self.cls_channels = head._num_classes
            cls_t, reg_t = _steps(head._classification_path), _steps(head._regression_path)
            for i, f in enumerate(feats):
                tc, tr = self._path(cls_t, f), self._path(reg_t, f)
                self._layer(tc, head._classification, None, False, out='cls', level=i)
                self._layer(tc, head._centerness, None, False, out='ctr', level=i)
                # fcos_head.py:145-146 `scales[i](regression(x)).float().exp()`: conv, bias, Scale in the epilogue, then expf
                self._layer(tr, head._regression, None, False, scale=self._scale(head._scales[i]), out='reg', level=i)
                self._simple('exp', None, out='reg', level=i)
            return
        if kind not in ('LFDHead', 'LFDHeadV1'):
            engine._unsupported('head %s' % kind)
        self.cls_channels = head.num_cls_channels
        for i, (f, d) in enumerate(zip(feats, netdesc.lfd_head_levels(None, head))):
            scale = self._scale(d.scale) if d.scale is not None else None
            t = self._path(_steps(d.merge), f)
            if kind == 'LFDHeadV1':       # towers end without the output convs: those are per-level members
                tc, tr = self._path(_steps(d.cls), t), self._path(_steps(d.reg), t)
                self._layer(tc, d.cls_out, None, False, out='cls', level=i)
                self._layer(tr, d.reg_out, None, False, scale=scale, out='reg', level=i)
            else:
                self._path(_steps(d.cls + [netdesc.layer(d.cls_out)]), t, out='cls', level=i)
                self._path(_steps(d.reg + [netdesc.layer(d.reg_out)]), t, scale=scale, out='reg', level=i)

    def _build(self, model):
        self._build_backbone(model._backbone)
        self.feats = self._build_neck(model._neck)
        self._build_head(model._head, self.feats)

    # ------------------------------------------------------------------ launches
    def _run_op(self, o, x, fmt, st, l, sp):
        k = o.kind
        if k in ('conv', 'gn'):
            return super()._run_op(o, x, fmt, st, l, sp)
        if k == 'merge':
            src, dst, up = st.bufs[o.src], st.bufs[o.dst], st.bufs[o.res]
            d = _lib.P32ConvDesc(st.n, src.shape[1], src.shape[2], o.cin, o.cout, 1, 1, o.relu, -1, 0, 0)
            check(l.lfd_p32_conv2d_merge_nhwc_f32(C.byref(d), ptr(src), ptr(dst), ptr(o.w), ptr(o.b), ptr(up), up.shape[1], up.shape[2],
                                                  sp), _LAUNCH[k])
        elif k == 'upadd':
            src, dst = st.bufs[o.src], st.bufs[o.dst]
            check(l.lfd_p32_upsample_nearest_add_f32(ptr(dst), ptr(src), st.n, dst.shape[1], dst.shape[2], src.shape[1],
                                                     src.shape[2], dst.shape[3], sp), _LAUNCH[k])
        elif k == 'relu':
            t = st.bufs[o.src]
            check(l.lfd_p32_relu_f32(ptr(t), t.numel(), sp), _LAUNCH[k])
        elif k == 'pool':
            src, dst = st.bufs[o.src], st.bufs[o.dst]
            check(l.lfd_p32_maxpool3x3s2_f32(ptr(src), ptr(dst), st.n, src.shape[1], src.shape[2], src.shape[3], sp), _LAUNCH[k])
        else:       # 'exp'
            t = getattr(st, o.out)
            hh, ww = st.sizes[o.level]
            check(l.lfd_p32_exp_rows_f32(ptr(t), st.n, st.P * t.shape[2], st.p_off[o.level], hh * ww, t.shape[2], sp), _LAUNCH[k])


def get_plan(model, device):
    cache = model.__dict__.setdefault('_lfd_sibling_p32_cache', {})
    key = (device.type, device.index, merge_enabled())
    plan = cache.get(key)
    sig = engine._param_signature(model._backbone, model._neck, model._head)
    if plan is None or plan.param_sig != sig:
        plan = SiblingPrecisePlan(model, device)
        cache[key] = plan
    return plan


@torch.no_grad()
def sibling_forward(model, x, use_graph=False, slot=0):
    """eval-mode forward in the fp32_storage mode -> (cls [N,P,C'], reg [N,P,4], centerness [N,P,1] | None, sizes), fp32,
    level-concatenated: engine-owned buffers, overwritten by the next call of the same input shape and slot.
    use_graph: one HIP graph per input buffer, like engine_sibling.sibling_forward."""
    _lib.require_cuda(x, "%s.forward (precision='fp32_storage')" % type(model).__name__)
    if not x.is_contiguous():
        x = x.contiguous()
    fmt, n, h, w = engine._input_format(x, model._backbone._input_channels)
    plan = get_plan(model, x.device)
    st = plan.state_for(n, h, w, slot)
    with torch.cuda.device(x.device):
        if not use_graph:
            plan.run(x, fmt, st)
        else:
            key = (x.data_ptr(), fmt)
            ent = st.graph.get(key)
            if ent is None:
                if len(st.graph) >= 4:
                    st.graph.pop(next(iter(st.graph)))
                plan.run(x, fmt, st)                # warm-up outside capture: kernel attributes
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    plan.run(x, fmt, st)
                ent = (g, x)                        # keep the captured input alive
                st.graph[key] = ent
            ent[0].replay()
    return st.cls, st.reg, st.ctr, st.sizes
