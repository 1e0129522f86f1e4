"""Layer-by-layer gfx950 engine for the sibling meta-architectures: FCOS (lfd/model/fcos.py:414-449) and
LFDv2 (lfd/model/lfdv2.py:671-702) over an LFDResNet or a ResNet-18 / 34 backbone, an FPN / SimpleFPN / SimpleNeck neck
(lfd/model/neck/fpn.py:127-152, simple_fpn.py:141-172, simple_neck.py) and an FCOSHead / LFDHead with 1x1 or 3x3 towers
(lfd/model/head/fcos_head.py:129-154, lfd_head.py:164-185).

The LFD configurations the reference ships run on the fused plan of engine.py (stem / residual-block / 3-pass head
kernels).  The siblings are not used by any shipped config; they get the same kernels one layer at a time:

  backbone             engine.EnginePlan.run_backbone (the fused stem / block / conv kernels, unchanged); a ResNet:
                       engine_resnet.ResNetPlan.run_backbone (7x7 stem, max-pool, the same block / conv kernels)
  conv (+ folded BN)   lfd_conv2d_nhwc_f16                     (MFMA implicit GEMM, csrc/conv_impl.h; with cin or cout above 128
                                                               csrc/conv_wide.hip behind the same entry point)
                       lfd_conv256_nhwc_f16                    (csrc/conv256.hip: 3x3 stride 1 from 256 channels on a batch of at
                                                               least CONV256_MIN_PIXELS output pixels -- _Conv.route)
  GroupNorm (+ ReLU)   lfd_gn_train_stats_f16 + lfd_gn_train_apply_f16   (GroupNorm has no eval mode: same kernels as training)
  top-down merge       lfd_upsample_nearest_add_nhwc_f16       (csrc/sibling.hip)
  extra levels         lfd_relu_inplace_f16, conv 3x3 s2 | lfd_maxpool3x3s2_nhwc_f16
  output convs         lfd_conv2d_nhwc_f16_acc32 (fp32 logits; from 256 channels lfd_conv256_nhwc_f16 in its fp32-output form, 3x3
                       or 1x1) + lfd_pack_level_outputs_f32 (Scale, exp, [N,P,C] concat)

Inter-layer storage is NHWC fp16 like the LFD plan.  Widths: 32 / 64 / 128 / 256 channels (others zero-padded up: the rule of
engine.pad_channels); a backbone tap may have 512 channels (csrc/conv_wide.hip reads it), neck and head convs with more than
256 outputs (MAX_WIDTH) are rejected; GroupNorm with 8 channels per group (the kernels' group size: 256/32, 128/16, 64/8).  No
PyTorch fallback: an unsupported module raises.
"""
import torch
import torch.nn as nn

from . import _lib, engine, engine_resnet, netdesc, ops


# Neck and head widths: up to 256 channels (csrc/conv_wide.hip and csrc/conv256.hip); 512 is a backbone tap's width only.
MAX_WIDTH = 256
# A 3x3 stride-1 conv from 256 channels runs on csrc/conv256.hip (128 pixels x all channels per workgroup) when the batch has at
# least this many output pixels, else on csrc/conv_wide.hip (64 pixels x 32 channels): the crossover of DESIGN 4i.
CONV256_MIN_PIXELS = 12288


def _unsupported(msg):
    raise RuntimeError('lfd_amd sibling engine: unsupported configuration: %s (no PyTorch fallback for inference)' % msg)


class _Conv(object):
    """conv [+ eval BatchNorm folded] [+ GroupNorm] [+ ReLU] on an NHWC fp16 map whose channel count is `cin_have`
    (>= conv.in_channels: the producer's zero padding)."""

    def __init__(self, conv, norm, relu, cin_have, dev, f32out=False):
        if not isinstance(conv, nn.Conv2d):
            _unsupported('expected nn.Conv2d, got %s' % type(conv).__name__)
        ks, st = conv.kernel_size[0], conv.stride[0]
        if conv.kernel_size != (ks, ks) or conv.stride != (st, st) or conv.padding != (ks // 2, ks // 2) \
                or ks not in (1, 3) or st not in (1, 2) or conv.groups != 1 or conv.dilation != (1, 1):
            _unsupported('conv %s' % (conv,))
        bn = norm if isinstance(norm, nn.BatchNorm2d) else None
        self.gn = norm if isinstance(norm, nn.GroupNorm) else None
        if norm is not None and bn is None and self.gn is None:
            _unsupported('norm %s' % type(norm).__name__)
        w, b = engine._fold_conv_norm(conv, bn)
        self.cout_real = w.shape[0]
        cout = engine.pad_channels(max(self.cout_real, 32))        # output convs have 1 .. 6 filters: one 32-wide MFMA tile
        if cout > MAX_WIDTH:    # the 512-channel kernels are the backbone's; a lateral conv READS such a tap (cin_have)
            _unsupported('neck / head convs with more than %d output channels (%d)' % (MAX_WIDTH, self.cout_real))
        if f32out and cin_have == 128 and cout == 32:
            cout = 64                     # the 128-channel fp32-output kernels are instantiated for >= 64 outputs
        if f32out and cin_have > 128:
            # fp32 logits from a 256-channel tower: csrc/conv256.hip at every map size (conv_wide has no fp32-output form)
            if st != 1 or not ops.conv256_supported(cin_have, cout, ks, True):
                _unsupported('no fp32-output conv kernel for %d -> %d channels, %dx%d stride %d' % (cin_have, cout, ks, ks, st))
        elif (cin_have > 128 or cout > 128) and not ops.conv2d_supported(cin_have, cout, ks, st):
            # a lateral on a 256 / 512-channel tap, any conv of a 256-channel neck / head: asked with the key __call__
            # launches (lfd_conv2d_nhwc_f16, csrc/conv_wide.hip; the large-map route of route() shares conv_wide's keys)
            _unsupported('no conv kernel for %d -> %d channels, %dx%d stride %d' % (cin_have, cout, ks, ks, st))
        if self.gn is not None:
            if cout != self.cout_real or self.cout_real != 8 * self.gn.num_groups:
                _unsupported('GroupNorm(%d, %d): the kernels take 8 channels per group on 32/64/128 channels'
                             % (self.gn.num_groups, self.cout_real))
            self.gamma = (self.gn.weight.detach().float() if self.gn.weight is not None
                          else torch.ones(cout)).to(dev).contiguous()
            self.beta = (self.gn.bias.detach().float() if self.gn.bias is not None
                         else torch.zeros(cout)).to(dev).contiguous()
        wp = torch.zeros((cout, cin_have, ks, ks), dtype=torch.float32, device=w.device)
        wp[:w.shape[0], :w.shape[1]] = w
        bp = torch.zeros(cout, dtype=torch.float32, device=w.device)
        bp[:b.shape[0]] = b
        self.w = ops.pack_conv_weight(wp).to(dev)
        self.b = bp.to(dev).contiguous()
        self.cin, self.cout, self.ks, self.stride, self.relu, self.f32out = cin_have, cout, ks, st, bool(relu), f32out

    def route(self, pixels):
        """the kernel that computes this conv on a batch of `pixels` output pixels.  A function of the layer and of the input's
        SHAPE alone (never of its values), so a captured graph replays the route it was captured with."""
        if self.f32out:
            return 'conv256_f32' if self.cin > 128 else 'acc32'
        if self.cin == 256 and self.ks == 3 and self.stride == 1 and pixels >= CONV256_MIN_PIXELS \
                and ops.conv256_supported(self.cin, self.cout, self.ks):
            return 'conv256'
        return 'conv_wide' if self.cin > 128 or self.cout > 128 else 'conv'

    def __call__(self, x):
        r = self.route(x.shape[0] * x.shape[1] * x.shape[2])
        if r == 'conv256_f32':
            return ops.conv256_nhwc(x, self.w, self.b, self.cout, self.ks, relu=False, f32out=True)
        if self.f32out:
            return ops.conv2d_nhwc_f32out(x, self.w, self.b, self.cin, self.cout, self.ks, self.stride)
        if r == 'conv256':
            y = ops.conv256_nhwc(x, self.w, self.b, self.cout, self.ks, relu=self.relu and self.gn is None)
        else:
            y = ops.conv2d_nhwc(x, self.w, self.b, self.cin, self.cout, self.ks, self.stride, self.relu and self.gn is None)
        if self.gn is not None:
            stats = ops.gn_train_stats(y, self.gn.num_groups, self.gn.eps)
            y = ops.gn_train_apply(y, self.gn.num_groups, stats, self.gamma, self.beta, relu=self.relu)
        return y


def _steps(seq):
    try:
        return netdesc.split_sequential(seq)
    except netdesc.UnknownModule as e:
        _unsupported(str(e))


class _Path(object):
    """the compiled steps (netdesc.split_sequential) of an nn.Sequential"""

    def __init__(self, steps, cin_have, dev, f32out_last=False):
        self.ops = []
        c = cin_have
        for k, s in enumerate(steps):
            if isinstance(s, netdesc.Layer):
                layer = _Conv(s.conv, s.norm, s.relu, c, dev, f32out=f32out_last and k == len(steps) - 1)
                self.ops.append(layer)
                c = layer.cout
            else:
                self.ops.append(s)
        self.cout = c
        self.inplace_relu_first = bool(steps) and steps[0] == 'relu'

    def __call__(self, x):
        for o in self.ops:
            if o == 'relu':
                x = ops.relu_(x)          # nn.ReLU(inplace=True): the caller's tensor changes too (by design, see plan)
            elif o == 'pool':
                x = ops.maxpool3x3s2(x)
            else:
                x = o(x)
        return x


class SiblingPlan(object):
    """Compiled (neck, head) of a sibling model for one device; the backbone keeps its own engine.EnginePlan."""

    def __init__(self, backbone, neck, head, dev):
        self.param_sig = engine._param_signature(backbone, neck, head)
        self.dev = dev
        # the backbone plan by backbone class: the torchvision-style ResNet has its own (7x7 stem + pool, engine_resnet)
        if engine_resnet.is_resnet(backbone):
            self.bb_plan = engine_resnet.get_plan(backbone, dev)
        elif engine_resnet.is_lfd_resnet(backbone):
            self.bb_plan = engine.get_plan(backbone, backbone, None, None, dev)
        else:        # a foreign backbone: say so, instead of an AttributeError on the first attribute a plan reads
            engine._unsupported('backbone %s (LFDResNet and ResNet have plans)' % type(backbone).__name__)
        self.tap_real = list(self.bb_plan.tap_channels)
        self.tap_have = [engine.pad_channels(c) for c in self.tap_real]      # the plan's buffers carry padded channels
        self._build_neck(neck)
        self._build_head(head)

    def routes(self, pixels):
        """[(where, cin, cout, ks, stride, _Conv.route)] of every conv of the neck and of the first level's head on a map of
        `pixels` output pixels (batch included), in launch order"""
        out = []

        def walk(tag, what):
            for o in (what.ops if isinstance(what, _Path) else [what]):
                if isinstance(o, _Conv):
                    out.append((tag, o.cin, o.cout, o.ks, o.stride, o.route(pixels)))

        for i, p in enumerate(self.laterals):
            walk('lateral%d' % i, p)
        for i, p in enumerate(self.outs or []):
            walk('out%d' % i, p)
        for k in ('merge', 'cls_t', 'reg_t', 'cls_p', 'reg_p', 'cls_o', 'ctr_o', 'reg_o'):
            if self.levels[0].get(k) is not None:
                walk(k, self.levels[0][k])
        return out

    # ------------------------------------------------------------------ neck
    def _build_neck(self, neck):
        kind = type(neck).__name__
        self.neck_kind = kind
        if kind == 'SimpleNeck':
            self.laterals = [_Path(_steps(getattr(neck, 'neck%d' % i)), c, self.dev) for i, c in enumerate(self.tap_have)]
            self.outs, self.num_inputs, self.num_outputs = None, len(self.laterals), len(self.laterals)
            self.bottom_up = False
            self.merge = False
            return
        if kind not in ('FPN', 'SimpleFPN'):
            _unsupported('neck %s' % kind)
        self.merge = True
        self.num_inputs, self.num_outputs = neck._num_inputs, neck._num_outputs
        self.extra_on_input = neck._extra_on_input
        self.bottom_up = bool(getattr(neck, '_neighbouring_mode', False))
        self.laterals = [_Path(_steps(getattr(neck, 'lateral%d' % i)), c, self.dev) for i, c in enumerate(self.tap_have)]
        cn = self.laterals[0].cout
        self.outs, self.out_real = [], []
        for i in range(self.num_outputs):
            from_input = i == self.num_inputs and self.extra_on_input
            src_c = self.tap_have[-1] if from_input else (self.outs[-1].cout if i >= self.num_inputs else cn)
            path = _Path(_steps(getattr(neck, 'fpn_out%d' % i)), src_c, self.dev)
            self.outs.append(path)
            if any(isinstance(o, _Conv) for o in path.ops) or i < self.num_inputs:
                self.out_real.append(neck._num_output_channels)
            else:       # a pooled extra level keeps the channels of what it pools (the last input, or the previous level)
                self.out_real.append(neck._num_input_channels_list[-1] if from_input else self.out_real[-1])

    def run_neck(self, taps):
        """taps: NHWC fp16 maps of the backbone.  Mirrors FPN.forward / SimpleFPN.forward including their in-place
        semantics: `+=` on the lateral maps and the inplace ReLU in front of an extra level (which also rewrites the
        level it reads from -- fpn.py:66-79 builds Sequential(ReLU(inplace=True), conv) and feeds fpn_outputs[-1])."""
        lat = [p(t) for p, t in zip(self.laterals, taps)]
        if not self.merge:
            return lat
        if self.bottom_up:
            for i in range(self.num_inputs - 1):
                ops.upsample_nearest_add_(lat[i], lat[i + 1])
        else:
            for i in range(self.num_inputs - 1, 0, -1):
                ops.upsample_nearest_add_(lat[i - 1], lat[i])
        outs = []
        for i in range(self.num_outputs):
            if i == self.num_inputs:
                src = taps[-1] if self.extra_on_input else outs[-1]
            elif i > self.num_inputs:
                src = outs[-1]
            else:
                src = lat[i]
            outs.append(self.outs[i](src))
        return outs

    # ------------------------------------------------------------------ head
    def _build_head(self, head):
        kind = type(head).__name__
        self.head_kind = kind
        cn = self.laterals[0].cout
        self.levels = []
        if kind == 'FCOSHead':
            cls_t = _Path(_steps(head._classification_path), cn, self.dev)
            reg_t = _Path(_steps(head._regression_path), cn, self.dev)
            cls_o = _Conv(head._classification, None, False, cls_t.cout, self.dev, f32out=True)
            ctr_o = _Conv(head._centerness, None, False, cls_t.cout, self.dev, f32out=True)
            reg_o = _Conv(head._regression, None, False, reg_t.cout, self.dev, f32out=True)
            self.num_cls_channels = head._num_classes
            for i in range(head._num_heads):
                self.levels.append(dict(cls_t=cls_t, reg_t=reg_t, cls_o=cls_o, ctr_o=ctr_o, reg_o=reg_o,
                                        scale=float(head._scales[i]._scale.detach()), exp=True))
            self.has_ctr = True
            return
        if kind not in ('LFDHead', 'LFDHeadV1'):
            _unsupported('head %s' % kind)
        self.has_ctr = False
        self.num_cls_channels = head.num_cls_channels
        cache = {}

        def compiled(layers, cin, f32out_last=False):
            """towers shared between the levels (share_head_flag) are compiled once"""
            key = (tuple(id(l.conv) for l in layers), cin, f32out_last)
            if key not in cache:
                cache[key] = _Path(_steps(layers), cin, self.dev, f32out_last=f32out_last)
            return cache[key]

        for i, d in enumerate(netdesc.lfd_head_levels(None, head)):
            # (a parameter update changes the plan signature, so the value read here cannot go stale)
            lv = dict(exp=False, scale=float(d.scale._scale.detach()) if d.scale is not None else 1.0, ctr_o=None)
            if head._merge_path_flag:
                lv['merge'] = compiled(d.merge, cn)
                c = lv['merge'].cout
            else:
                lv['merge'] = None
                c = cn
            if kind == 'LFDHeadV1':     # towers end without the output convs: those are per-level members
                lv['cls_p'], lv['reg_p'] = compiled(d.cls, c), compiled(d.reg, c)
                lv['cls_o'] = _Conv(d.cls_out, None, False, lv['cls_p'].cout, self.dev, f32out=True)
                lv['reg_o'] = _Conv(d.reg_out, None, False, lv['reg_p'].cout, self.dev, f32out=True)
            else:
                lv['cls_p'] = compiled(d.cls + [netdesc.layer(d.cls_out)], c, True)
                lv['reg_p'] = compiled(d.reg + [netdesc.layer(d.reg_out)], c, True)
            self.levels.append(lv)

    def run_head(self, feats):
        """-> (cls [N,P,C'] fp32, reg [N,P,4] fp32, centerness [N,P,1] fp32 | None, sizes)"""
        n = feats[0].shape[0]
        sizes = [(f.shape[1], f.shape[2]) for f in feats]
        P = sum(h * w for h, w in sizes)
        dev = feats[0].device
        cls = torch.empty((n, P, self.num_cls_channels), dtype=torch.float32, device=dev)
        reg = torch.empty((n, P, 4), dtype=torch.float32, device=dev)
        ctr = torch.empty((n, P, 1), dtype=torch.float32, device=dev) if self.has_ctr else None
        p0 = 0
        for lv, f, (h, w) in zip(self.levels, feats, sizes):
            scale = lv['scale']
            if self.head_kind == 'FCOSHead':
                tc = lv['cls_t'](f)
                tr = lv['reg_t'](f)
                ops.pack_level_outputs(lv['cls_o'](tc), cls, 0, self.num_cls_channels, p0)
                ops.pack_level_outputs(lv['ctr_o'](tc), ctr, 0, 1, p0)
                ops.pack_level_outputs(lv['reg_o'](tr), reg, 0, 4, p0, scale=scale, exp=True)
            else:
                t = lv['merge'](f) if lv['merge'] is not None else f
                c, r = lv['cls_p'](t), lv['reg_p'](t)
                if 'cls_o' in lv:
                    c, r = lv['cls_o'](c), lv['reg_o'](r)
                ops.pack_level_outputs(c, cls, 0, self.num_cls_channels, p0)
                ops.pack_level_outputs(r, reg, 0, 4, p0, scale=scale)
            p0 += h * w
        return cls, reg, ctr, sizes


def get_plan(owner, backbone, neck, head, device):
    cache = owner.__dict__.setdefault('_lfd_sibling_cache', {})
    key = (device.type, device.index)
    plan = cache.get(key)
    sig = engine._param_signature(backbone, neck, head)
    if plan is None or plan.param_sig != sig:
        with torch.no_grad():
            plan = SiblingPlan(backbone, neck, head, device)
        cache[key] = plan
    return plan


def backbone_taps(plan, x):
    """image batch -> the backbone's tapped maps, NHWC fp16 (engine-owned buffers, padded channels)"""
    fmt, n, h, w = engine._input_format(x, plan.bb_plan.input_channels)
    st = plan.bb_plan.state_for(n, h, w)
    plan.bb_plan.run_backbone(x, fmt, st)
    return [st.bufs[t] for t in plan.bb_plan.taps]


@torch.no_grad()
def sibling_forward(model, x, use_graph=False):
    """eval-mode forward of FCOS / LFDv2 on the device -> (cls, reg, centerness | None, sizes), fp32, level-concatenated.
    use_graph: the ~100 launches of a forward are captured into one HIP graph per input buffer and replayed (the
    returned tensors are then graph-owned and overwritten by the next call with the same input buffer)."""
    _lib.require_cuda(x, '%s.forward' % type(model).__name__)
    if not x.is_contiguous():
        x = x.contiguous()
    plan = get_plan(model, model._backbone, model._neck, model._head, x.device)

    def run():
        return plan.run_head(plan.run_neck(backbone_taps(plan, x)))

    with torch.cuda.device(x.device):
        if not use_graph:
            return run()
        graphs = plan.__dict__.setdefault('graphs', {})
        key = (x.data_ptr(), tuple(x.shape), x.dtype)
        ent = graphs.get(key)
        if ent is None:
            if len(graphs) >= 4:
                graphs.pop(next(iter(graphs)))
            run()                               # warm-up outside capture: kernel attributes, workspaces
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                outs = run()
            ent = (g, outs, x)                  # keep the captured input alive
            graphs[key] = ent
        ent[0].replay()
        return ent[1]


@torch.no_grad()
def neck_forward(neck, inputs):
    """FPN / SimpleFPN .forward stand-alone on NCHW fp32 feature maps (reference types in and out, fpn.py:127-152); the
    layout / precision conversion around the kernels is plain tensor plumbing."""
    x0 = inputs[0]
    _lib.require_cuda(x0, '%s.forward' % type(neck).__name__)
    dev = x0.device
    cache = neck.__dict__.setdefault('_lfd_sibling_cache', {})
    sig = engine._param_signature(neck)
    key = (dev.type, dev.index)
    ent = cache.get(key)
    if ent is None or ent.param_sig != sig:
        ent = SiblingPlan.__new__(SiblingPlan)
        ent.param_sig, ent.dev = sig, dev
        ent.tap_have = [engine.pad_channels(t.shape[1]) for t in inputs]
        ent._build_neck(neck)
        cache[key] = ent
    with torch.cuda.device(dev):
        taps = []
        for t, c in zip(inputs, ent.tap_have):
            y = t.permute(0, 2, 3, 1).half()
            if c != t.shape[1]:
                y = torch.nn.functional.pad(y, (0, c - t.shape[1]))
            taps.append(y.contiguous())
        outs = ent.run_neck(taps)
    real = ent.out_real if ent.merge else [neck._num_neck_channels] * len(outs)
    return tuple(o[..., :c].permute(0, 3, 1, 2).float() for o, c in zip(outs, real))
