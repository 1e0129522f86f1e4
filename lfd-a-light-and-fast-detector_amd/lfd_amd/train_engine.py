"""Training-mode forward / backward on the hand-written gfx950 kernels (csrc/train.hip + the MFMA conv of
csrc/conv.hip), bridged into autograd as ONE node per model that the loss (and whatever torch modules are left behind it) drives.
Four nodes, each the widest one its model admits:
    BackboneTrainFunction   the LFDResNet backbone alone (`supported`); neck and head stay PyTorch-ROCm modules under autograd
    NetworkTrainFunction    backbone + SimpleNeck + LFDHead, the whole network (`network_supported`; level-concatenated head)
    PyramidTrainFunction    backbone + FPN / SimpleFPN (`pyramid_supported`)
    DetectorTrainFunction   that pyramid + FCOSHead or LFDHead (`fcos_head_supported` / `lfd_head_supported`): ONE plan class,
                            forward, backward and Function for both heads; what is head-specific is the builder of the plan and a
                            glue adapter around the output convs (_FCOSGlue: csrc/fcos_out.hip, _LFDGlue: csrc/lfd_out.hip)
All of them run the same unit step (_unit_forward / _unit_backward), the same units-last-to-first loop (_units_backward) and the
same two weight-gradient forms (_wgrad_accumulate: straight into the parameter's gradient; _wgrad_partials: partial sums into a
persistent buffer, summed with all others of the iteration by one launch).

Reference semantics of the backbone: LFDResNet.forward in train mode (lfd/model/backbone/lfd_resnet.py:488-501) over
nn.Conv2d(bias=False) -> nn.BatchNorm2d (batch statistics, running statistics updated) -> ReLU units, residual
blocks `relu(norm(conv(..)) + identity)` (:96-154), identity = norm(conv1x1 s2(x)) for the first block of a stage
(:458-468).  Numerics here: NHWC fp16 activations / activation gradients (gradients carry a power-of-two loss
scale), fp32 accumulation on MFMA, fp32 statistics, parameters and parameter gradients.

The backward is a hand-written schedule over the recorded units (no autograd inside):
    g, dy = bn_bwd(dz)  ->  dW = wgrad(x, dy)  ->  dx = conv(dy, W^T flipped) (+ gradient already collected for x)
"""
import collections
import itertools
import os

import torch
import torch.nn as nn

from . import engine_resnet, netdesc, ops

LOSS_SCALE = 1024.0   # initial value; power of two; activation gradients are stored as fp16 * loss_scale()
_scale_state = {'value': LOSS_SCALE}


def loss_scale():
    """the loss scale the next backward pass multiplies the prediction gradients with (fp16 activation gradients carry it,
    the weight-gradient / norm kernels divide it out again: parameter gradients are unscaled fp32)"""
    return _scale_state['value']


def set_loss_scale(v):
    """power of two in [1, 65536] (lfd_amd.train.DynamicLossScale drives this from the gradient norm's finiteness)"""
    v = float(v)
    if not (1.0 <= v <= 65536.0) or v != 2.0 ** round(__import__('math').log2(v)):
        raise ValueError('loss scale must be a power of two in [1, 65536]')
    _scale_state['value'] = v


_SchedSwitches = collections.namedtuple('_Switches', 'conv_bn_stats dgrad_s2 out_fused bn_levels head_out_levels bn_apply_in_conv '
                                                     'bn_sums_in_dgrad conv0_bn_wgrad')


class _Switches(_SchedSwitches):
    """the eight switches of the training schedules (the tuple: what a pass hands down) and, beside them, hip_neck / hip_head: the
    ROUTING switches of the pyramid-neck node and of the detector node on top of it, read by the models when they choose a route
    and by no schedule"""
    hip_neck = True
    hip_head = True


def switches():
    """The A/B switches of the training schedules (all on by default; what '0' runs instead stands beside each), read from the
    environment at every call: the public entries call this once per pass and hand the record down.  `.hip_neck`
    (LFD_HIP_NECK, default on): FPN / SimpleFPN necks run inside the backbone's autograd node (PyramidTrainFunction); '0'
    restores the backbone node with the neck as PyTorch-ROCm modules under autograd.  `.hip_head` (LFD_HIP_HEAD, default on): an
    FCOSHead or an LFDHead behind such a neck runs inside the same node (DetectorTrainFunction); '0'
    keeps the pyramid node with the head under autograd.  The head node sits on the pyramid node: LFD_HIP_NECK=0 turns both off."""
    sw = _Switches(
        conv_bn_stats=os.environ.get('LFD_CONV_BN_STATS', '1') == '1',           # conv, then a statistics pass over y
        dgrad_s2=os.environ.get('LFD_DGRAD_S2', '1') == '1',                     # zero_insert2 + stride-1 conv (3x3 stride-2 dgrad)
        out_fused=os.environ.get('LFD_OUT_FUSED', '1') == '1',                   # output-conv glue as PyTorch ops (serial API only)
        bn_levels=os.environ.get('LFD_BN_LEVELS', '1') == '1',                   # neck BatchNorm passes level after level
        head_out_levels=os.environ.get('LFD_HEAD_OUT_LEVELS', '1') == '1',       # output-conv glue level after level
        bn_apply_in_conv=not os.environ.get('LFD_BN_APPLY_IN_CONV', '1') != '1',  # every unit stores its activation
        bn_sums_in_dgrad=os.environ.get('LFD_BN_SUMS_IN_DGRAD', '1') == '1',     # every BatchNorm backward sums for itself
        conv0_bn_wgrad=os.environ.get('LFD_CONV0_BN_WGRAD', '1') == '1')         # first unit: norm backward, then weight gradient
    sw.hip_neck = os.environ.get('LFD_HIP_NECK', '1') == '1'
    sw.hip_head = os.environ.get('LFD_HIP_HEAD', '1') == '1'
    return sw


class _Unit(object):
    # eval_norm: the unit's BatchNorm2d is in eval mode inside the training model (running statistics, nothing updated);
    # frozen: eval_norm and none of its parameters takes a gradient -- forward only, never visited by the backward
    __slots__ = ('conv', 'norm', 'relu', 'src', 'res', 'dst', 'first', 'level', 'frozen', 'eval_norm')


class _Out(object):
    """Output convs of one pyramid level: cls conv1x1 (+bias) and reg conv1x1 (+bias) x Scale (lfd_head.py:107-111,
    :176-180).  With a merged tower both read the same activation and run as ONE conv (rows concatenated, padded to 32)."""
    __slots__ = ('level', 'convs', 'src', 'scale')


def _conv_ok(m, first=False):
    """first: the backbone's first stem conv, which may also read ONE input plane (a grayscale model, csrc/stem_gray_train.hip)"""
    if first and m.in_channels == 1:
        return True
    return m.in_channels == 3 or (m.in_channels in (32, 64, 128) and m.out_channels in (32, 64, 128))


def frozen_modules(backbone):
    """the modules LFDResNet.train() freezes for its frozen_stages (lfd_resnet.py:476-487): the stem and stage0 .. stage{k-1}"""
    k = backbone._frozen_stages
    return [backbone._stem] + [getattr(backbone, 'stage%d' % i) for i in range(k)] if k > 0 else []


def supported(backbone):
    """The HIP training path covers BatchNorm2d + ReLU backbones with 32/64/128-channel convs; RGB or grayscale
    (input_channels 3 or 1).  Frozen parameters and eval-mode norms: exactly what the backbone's own frozen_stages /
    norm_eval produce in train() -- the stem and the first stages frozen (forward only), every BatchNorm2d on its running
    statistics."""
    if not engine_resnet.is_lfd_resnet(backbone):
        return False          # the torchvision-style ResNet (7x7 stem, max-pool): PyTorch-ROCm autograd, its attributes unread
    if backbone._norm_cfg is None or backbone._norm_cfg.get('type') != 'BatchNorm2d':
        return False
    if backbone._activation_cfg.get('type') != 'ReLU' or not backbone.training:
        return False
    if backbone._input_channels not in (1, 3):
        return False
    # the hand-written backward accumulates into every parameter's .grad but those of the frozen stages: any OTHER frozen
    # parameter (requires_grad=False, however it was frozen), or a thawed one inside a frozen stage, sends the module through
    # PyTorch-ROCm autograd instead; the same for a norm layer whose mode is not the one train() gives it
    fz_params, fz_mods = set(), set()
    for fm in frozen_modules(backbone):
        fz_params.update(id(p) for p in fm.parameters())
        fz_mods.update(id(m) for m in fm.modules())
    if not all(p.requires_grad == (id(p) not in fz_params) for p in backbone.parameters()):
        return False
    first = backbone._stem[0]
    for m in backbone.modules():
        if isinstance(m, nn.Conv2d) and not _conv_ok(m, m is first):
            return False
        if isinstance(m, nn.BatchNorm2d) and (m.momentum is None or not m.affine or not m.track_running_stats
                                              or m.training == (backbone._norm_eval or id(m) in fz_mods)):
            return False          # incl. norm layers switched to eval() by hand inside a training model
    return (first.in_channels == backbone._input_channels and first.out_channels in (32, 64) and first.kernel_size == (3, 3)
            and first.stride == (2, 2))


def check_train_input(backbone, x):
    """The HIP training path reads an NCHW float32 batch of the model's input_channels; an RGB batch for a gray model (or the
    reverse) raises here, before any kernel reads it."""
    c = backbone._input_channels
    if x.dim() != 4 or x.dtype != torch.float32 or x.size(1) != c:
        raise RuntimeError('training input: expected an NCHW float32 batch [N,%d,H,W] for an input_channels=%d model, got %s %s'
                           % (c, c, x.dtype, tuple(x.shape)))


def network_supported(model):
    """+ SimpleNeck with BatchNorm2d, LFDHead with 1x1 convs and GroupNorm groups of 8 channels, and output convs that fit the
    padded 1x1 conv of a level (_out_weight: 64 or 128 rows, the two instantiations of csrc/head_out.hip):
      - cls and reg conv reading the same activation (merge_path_flag, or no tower layers) run as ONE conv:
        num_cls_channels + 4 <= 128  (<= 60: the 64-row kernels; 61..124: the 128-row ones)
      - separate towers, one conv each: num_cls_channels <= 128
    The convs on both sides exist for every admitted shape: forward {64, 128} -> {64, 128} rows and data gradient
    {64, 128} rows -> {64, 128} channels are instances of csrc/conv.hip, the weight gradient tiles any multiple of 64."""
    bb, neck, head = model._backbone, model._neck, model._head
    if type(neck).__name__ != 'SimpleNeck' or type(head).__name__ != 'LFDHead':
        return False          # FPN / SimpleFPN necks, LFDHeadV1, FCOSHead: PyTorch-ROCm autograd behind the HIP backbone
    if not supported(bb):
        return False
    if not all(p.requires_grad for p in list(neck.parameters()) + list(head.parameters())):
        return False
    if neck._norm_cfg is None or neck._norm_cfg.get('type') != 'BatchNorm2d' or neck._activation_cfg.get('type') != 'ReLU':
        return False
    if head._norm_cfg is None or head._norm_cfg.get('type') != 'GroupNorm' or head._activation_cfg.get('type') != 'ReLU':
        return False
    if head._conv_kernel_size != 1 or head._num_head_channels != 8 * head._norm_cfg.get('num_groups', 0):
        return False
    if neck._num_neck_channels not in (64, 128) or head._num_head_channels not in (64, 128):
        return False
    for m in head.modules():
        if isinstance(m, nn.GroupNorm) and not m.affine:
            return False
    for m in neck.modules():
        if isinstance(m, nn.BatchNorm2d) and (m.momentum is None or not m.affine or not m.track_running_stats
                                              or not m.training):
            return False
        if isinstance(m, nn.Conv2d) and not _conv_ok(m):
            return False
    one_conv = head._merge_path_flag or head._num_conv_layers == 0
    return head.num_cls_channels + (4 if one_conv else 0) <= 128


class _Builder(object):
    def __init__(self):
        self.units, self.n_act, self.level = [], 1, None

    def add(self, conv, norm, relu, src, res=None):
        u = _Unit()
        u.conv, u.norm, u.relu, u.src, u.res, u.dst, u.first = conv, norm, relu, src, res, self.n_act, src == 0
        u.level = self.level            # None: backbone; i: the neck / tower chain of pyramid level i
        u.eval_norm = isinstance(norm, nn.BatchNorm2d) and not norm.training
        u.frozen = u.eval_norm and not any(p.requires_grad for p in (conv.weight, norm.weight, norm.bias))
        self.units.append(u)
        self.n_act += 1
        return u.dst


def _build_backbone(b, backbone):
    net = netdesc.backbone_layers(backbone)
    cur = _tower(b, net.stem, 0)
    taps = []
    for blk in net.blocks:
        ident = cur if blk.downsample is None else _tower(b, [blk.downsample], cur)
        for l in blk.convs:
            cur = b.add(l.conv, l.norm, l.relu, cur, ident if l is blk.convs[-1] else None)
        if blk.tap:
            taps.append(cur)
    return taps


def build_units(backbone):
    """-> (units, tap activation indices).  Activation 0 is the input image."""
    b = _Builder()
    taps = _build_backbone(b, backbone)
    return b.units, taps


def _tower(b, layers, cur):
    """a chain of netdesc.Layers as units from activation `cur` on -> the last activation"""
    for l in layers:
        cur = b.add(l.conv, l.norm, l.relu, cur)
    return cur


def _out(level, convs, src, scale):
    o = _Out()
    o.level, o.convs, o.src, o.scale = level, convs, src, scale
    return o


def _lfd_head_level(b, d, i, src):
    """level i of an LFDHead (netdesc.Level `d`) on activation `src` (lfd_head.py:164-185): the merge path's units, the two
    towers' units -> the level's _Out records: ONE (rows of both output convs) when they read the same activation, else two"""
    cur = _tower(b, d.merge, src)
    csrc, rsrc = _tower(b, d.cls, cur), _tower(b, d.reg, cur)
    if csrc == rsrc:
        return [_out(i, [('cls', d.cls_out), ('reg', d.reg_out)], csrc, d.scale)]
    return [_out(i, [('cls', d.cls_out)], csrc, d.scale), _out(i, [('reg', d.reg_out)], rsrc, d.scale)]


def build_network(model):
    """-> (units, outs): backbone + neck + head towers as conv/norm/ReLU units, and the per-level output convs."""
    b = _Builder()
    taps = _build_backbone(b, model._backbone)
    outs = []
    for i, (tap, d) in enumerate(zip(taps, netdesc.lfd_head_levels(model._neck, model._head))):
        b.level = i
        outs += _lfd_head_level(b, d, i, _tower(b, [d.neck], tap))
    return b.units, outs


def _unique(params):
    """the parameters (or modules) in their order, each object once"""
    seen, out = set(), []
    for p in params:
        if id(p) not in seen:
            seen.add(id(p))
            out.append(p)
    return out


def backbone_params(units):
    """the parameters the backward accumulates gradients into: those of the units that are not frozen"""
    ps = []
    for u in units:
        if not u.frozen:
            ps += [u.conv.weight, u.norm.weight, u.norm.bias]
    return _unique(ps)


def dead_activations(units):
    """activations nobody needs a gradient for: the input image and the outputs of the frozen units (a frozen activation that
    is a pyramid tap or feeds a trainable unit is read; the gradient that would flow into it is never formed)"""
    return {0} | {u.dst for u in units if u.frozen}


def _plan_params(base, units, outs):
    """the parameters of a plan in the order its Function receives them: `base` (what the plan is built on), then the units'
    that are not frozen, then per output record its convs' weight and bias and its Scale; every parameter once"""
    ps = list(base) + backbone_params(units)
    for o in outs:
        for _, conv in o.convs:
            ps += [conv.weight, conv.bias]
        if o.scale is not None:
            ps.append(o.scale._scale)
    return _unique(ps)


def network_params(units, outs):
    return _plan_params((), units, outs)


def _dgrad_weight(w):
    """weights of the conv that maps dL/dy to dL/dx: swap the channel roles, flip the taps"""
    return ops.pack_conv_weight_train(w, data_gradient=True)


_pack_batches = {}


class _Packs(object):
    """fp16 fragment packs of the conv weights of a pass.  With `units` given, every distinct conv weight of the schedule
    is packed by ONE launch up front (ops.PackBatch, job table cached per schedule); other weights (the concatenated
    output convs) are packed individually on first use.  Shared by the pyramid levels within a pass."""

    def __init__(self, units=None, data_gradient=False):
        self.c = {}
        if units:
            ws, seen = [], set()
            for u in units:
                w = u.conv.weight
                if not u.first and not u.frozen and id(w) not in seen:
                    seen.add(id(w))
                    ws.append(w.detach())
            if ws:
                key = (id(units), data_gradient)
                pb = _pack_batches.pop(key, None)
                if pb is None or not pb.matches(ws):
                    # least recently used first: clearing the whole cache here could drop the OTHER pass of the schedule
                    # just packed eagerly, and rebuild its job table (a host -> device copy) inside a graph capture
                    while len(_pack_batches) >= 32:
                        _pack_batches.pop(next(iter(_pack_batches)))
                    pb = ops.PackBatch(ws, data_gradient)
                _pack_batches[key] = pb
                for w, out in zip(ws, pb.run()):
                    self.c[(w.data_ptr(), data_gradient)] = out

    def __call__(self, w, data_gradient=False):
        k = (w.data_ptr(), data_gradient)
        if k not in self.c:
            self.c[k] = ops.pack_conv_weight_train(w, data_gradient=data_gradient)
        return self.c[k]


class _EvalNorms(object):
    """What the eval-mode norms of a plan need per iteration: rows[id(norm)] = the (mean, rstd) row of its running statistics
    (ops.BnEvalRows, one launch) and folded[unit index] = (packed weight, bias) of every frozen unit but the first conv
    (ops.FoldBatch, two launches); both cached by the tensors' version counters.  Kept on the plan's owner."""

    def __init__(self):
        self.rows_batch = self.fold_batch = None

    def run(self, units):
        self.rows, self.folded = {}, {}
        norms = _unique([u.norm for u in units if u.eval_norm])
        if not norms:
            return self
        if self.rows_batch is None or not self.rows_batch.matches(norms):
            self.rows_batch = ops.BnEvalRows(norms)
        rows, fresh = self.rows_batch.run()
        self.rows = {id(m): r for m, r in zip(norms, rows)}
        fz = [(ui, u) for ui, u in enumerate(units) if u.frozen and not u.first]
        if fz:
            items = [(u.conv.weight.detach(), u.norm.weight.detach(), u.norm.bias.detach(), self.rows[id(u.norm)]) for _, u in fz]
            if self.fold_batch is None or not self.fold_batch.matches(items):
                self.fold_batch = ops.FoldBatch(items)
                fresh = True
            packed, biases = self.fold_batch.run(fresh)
            self.folded = {ui: (wp, b) for (ui, _), wp, b in zip(fz, packed, biases)}
        return self


def _eval_norms(owner, units):
    ev = owner.__dict__.get('_lfd_eval_norms')
    if ev is None:
        ev = owner.__dict__['_lfd_eval_norms'] = _EvalNorms()
    return ev.run(units)


def _frozen_forward(ui, u, acts, ev):
    """a frozen unit: relu?(conv(x, w') + b' (+ residual)) in one launch on the folded weights; the first conv (3 or 1 input
    channels) through its training forward kernel and an apply pass on the running statistics.  Nothing is kept for a backward."""
    conv, norm = u.conv, u.norm
    res = acts[u.res] if u.res is not None else None
    if u.first:
        y = ops.stem_conv0_train_fwd(acts[u.src], conv.weight)
        return ops.bn_train_apply(y, ev.rows[id(norm)], norm.weight.detach(), norm.bias.detach(), res, u.relu)
    wp, bias = ev.folded[ui]
    return ops.conv2d_nhwc(acts[u.src], wp, bias, conv.in_channels, conv.out_channels, conv.kernel_size[0], conv.stride[0], u.relu,
                           residual=res)


def _count_batches(units):
    """num_batches_tracked += 1 for the training-mode norms (an eval-mode BatchNorm2d updates nothing)"""
    nbt = [u.norm.num_batches_tracked for u in units if isinstance(u.norm, nn.BatchNorm2d) and not u.eval_norm]
    if nbt:
        torch._foreach_add_(nbt, 1)


_zero_cache = {}


class _Zeros(object):
    """zero bias vectors (the units' convs have none): persistent per device -- nobody writes them"""

    def __init__(self, dev):
        self.dev = dev

    def __call__(self, n):
        k = (self.dev.type, self.dev.index, n)
        if k not in _zero_cache:
            _zero_cache[k] = torch.zeros(n, dtype=torch.float32, device=self.dev)
        return _zero_cache[k]


def _unit_forward(ui, u, acts, packs, zeros, sw, ev=None, store=True, producer=None):
    """conv -> norm (batch / group / running statistics) -> (+ residual) -> ReLU of one unit on the current stream: the one unit
    forward of both schedules.  -> what the backward needs, (y, stats); None for a frozen unit (one launch on the folded weights).
    ev: the _EvalNorms of the pass (plans with eval-mode norms).  store=False: the activation is not written (_deferred_units:
    its consumer forms it from (y, stats)); producer = (unit, (y, stats)) of such an input."""
    if u.frozen:
        acts[u.dst] = _frozen_forward(ui, u, acts, ev)
        return None
    conv, norm = u.conv, u.norm
    xin = acts[u.src]
    ks, st, cout = conv.kernel_size[0], conv.stride[0], conv.out_channels
    # the batch statistics come out of the conv's epilogue: no separate read of y (csrc/conv_stats.hip)
    conv_stats = sw.conv_bn_stats and isinstance(norm, nn.BatchNorm2d) and not u.eval_norm
    stats = None
    if producer is not None:
        pu, (py, pstats) = producer
        y, stats = ops.conv1x1_of_bn_relu_bn_stats(py, pstats, pu.norm.weight.detach(), pu.norm.bias.detach(), packs(conv.weight),
                                                   zeros(cout), cout, norm.eps, norm.momentum, norm.running_mean, norm.running_var)
    elif u.first and conv_stats:
        y, stats = ops.stem_conv0_train_fwd_bn_stats(xin, conv.weight, norm.eps, norm.momentum, norm.running_mean,
                                                     norm.running_var)
    elif u.first:
        y = ops.stem_conv0_train_fwd(xin, conv.weight)
    elif conv_stats:
        y, stats = ops.conv2d_bn_stats(xin, packs(conv.weight), zeros(cout), conv.in_channels, cout, ks, st, norm.eps,
                                       norm.momentum, norm.running_mean, norm.running_var)
    else:
        y = ops.conv2d_nhwc(xin, packs(conv.weight), zeros(cout), conv.in_channels, cout, ks, st, False)
    if isinstance(norm, nn.GroupNorm):
        stats, z = ops.gn_train_stats_apply(y, norm.num_groups, norm.eps, norm.weight.detach(), norm.bias.detach(), u.relu)
    else:
        if u.eval_norm:       # the row of the running statistics; the backward is one pass (ops.bn_eval_backward)
            stats = ev.rows[id(norm)]
        elif stats is None:
            stats = ops.bn_train_stats(y, norm.eps, norm.momentum, norm.running_mean, norm.running_var)
        z = ops.bn_train_apply(y, stats, norm.weight.detach(), norm.bias.detach(),
                               acts[u.res] if u.res is not None else None, u.relu) if store else None
    acts[u.dst] = z
    return y, stats


def forward(units, tap_ids, x, owner=None):
    """x: NCHW fp32 image batch (as LFD.forward receives it, lfd.py:511).  -> (requested activations NHWC fp16, saved).
    owner: the module that keeps the plan (the per-iteration state of eval-mode norms lives on it)."""
    sw = switches()
    acts = {0: x}
    zeros = _Zeros(x.device)
    packs = _Packs(units, False)
    ev = None
    if any(u.eval_norm for u in units):
        ev = _eval_norms(owner, units) if owner is not None else _EvalNorms().run(units)
    tape = [_unit_forward(ui, u, acts, packs, zeros, sw, ev) for ui, u in enumerate(units)]
    _count_batches(units)
    return [acts[t] for t in tap_ids], (acts, tape)


class _GradStore(object):
    """Where the fp32 parameter gradients go.  in_place: straight into `p.grad` (created zeroed when missing) -- the
    kernels `+=` into it, which is autograd's AccumulateGrad semantics without one temporary + one add per tensor (the
    autograd node then reports no gradient for the parameters).  Otherwise: private zero-initialised buffers by
    parameter identity (tests).  Shared modules (the head towers of all levels) accumulate either way."""

    def __init__(self, in_place=False):
        self.g, self.in_place = {}, in_place

    def target(self, p):
        """the buffer every kernel accumulates this parameter's gradient into"""
        if self.in_place:
            if p.grad is None:
                p.grad = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
            return p.grad
        k = id(p)
        if k not in self.g:
            self.g[k] = torch.zeros_like(p, dtype=torch.float32, memory_format=torch.contiguous_format)
        return self.g[k]

    def add(self, p, grad):
        self.target(p).add_(grad.reshape(p.shape))

    def get(self, p):
        return p.grad if self.in_place else self.g.get(id(p))


def _data_gradient(conv, dy, h, w, residual, packs, zeros, sw):
    """dL/dx [N, h, w, cin] (+ residual: the gradient already collected for x) of a unit's conv from dL/dy"""
    ks, st, cin, cout = conv.kernel_size[0], conv.stride[0], conv.in_channels, conv.out_channels
    if st == 2 and ks == 3 and cin == 64 and cout == 64 and sw.dgrad_s2:
        # per output parity, 9 tap-products per 2 x 2 pixels instead of 36 and no zero-inserted tensor (csrc/dgrad_s2.hip)
        return ops.conv3x3s2_dgrad(dy, packs(conv.weight, True), h, w, residual=residual)
    if st == 2:
        dy = ops.zero_insert2(dy, h, w)
    return ops.conv2d_nhwc(dy, packs(conv.weight, True), zeros(cin), cout, cin, ks, 1, False, residual=residual)


# what only the whole-network schedule does in a unit's backward: fed = {1x1 conv unit: the unit in front of it, whose BatchNorm
# backward sums that conv's data gradient leaves behind}, sum_rows = {unit: the rows of such sums} (filled on the way)
_Fusions = collections.namedtuple('_Fusions', 'fed sum_rows')


def _unit_backward(ui, u, dz, units, saved, grads, dead, store, packs, zeros, inv, sw, wgrad, fus=None, trace=None):
    """The backward of unit ui from dz = dL/d(its activation): norm backward, residual hand-off, weight gradient, data gradient
    (added to what `grads` holds for the unit's input; none for an input in `dead`).  The one unit backward of both schedules:
    wgrad(xin, dy, ks, st, inv, targets, producer) forms the conv's weight gradient (_wgrad_accumulate, or the whole-network
    schedule's partial sums; targets as ops.WgradFinals.add_wgrad);
    fus: the _Fusions of the whole-network schedule, which also takes the first unit's one-launch shortcut and re-forms inputs
    that were never stored; trace: optional list that receives this unit's tensors."""
    acts, tape = saved
    conv, norm = u.conv, u.norm
    y, stats = tape[ui]
    z = acts[u.dst] if u.relu else None
    g = None
    gamma, beta = norm.weight.detach(), norm.bias.detach()
    dgamma, dbeta = store.target(norm.weight), store.target(norm.bias)
    snap = [t.clone() for t in (dgamma, dbeta, store.target(conv.weight))] if trace is not None else None
    if (fus is not None and u.first and isinstance(norm, nn.BatchNorm2d) and not u.eval_norm and u.relu and u.res is None
            and conv.out_channels == 64 and sw.conv0_bn_wgrad):
        # the first unit has no data gradient: BatchNorm's sums, then the weight gradient straight from dz and y (no dy tensor)
        ops.stem_conv0_bn_bwd_wgrad(acts[u.src], dz, y, stats, gamma, beta, inv, dgamma, dbeta, store.target(conv.weight),
                                    sum_rows=fus.sum_rows.get(ui, 0))
        return
    if isinstance(norm, nn.GroupNorm):
        dy = ops.gn_train_backward(dz, y, z, norm.num_groups, stats, gamma, inv, dgamma, dbeta, True)
    elif u.eval_norm:
        # constant statistics: dy does not wait for the sums -- one pass over (dz, y) instead of two
        dy, g = ops.bn_eval_backward(dz, y, z if u.res is not None else None, stats, gamma, inv, dgamma, dbeta,
                                     want_g=u.res is not None and u.res not in dead, accumulate=True, relu=u.relu, beta=beta)
    elif fus is not None and ui in fus.sum_rows:
        dy = ops.bn_train_backward_rows(dz, y, stats, gamma, beta, inv, dgamma, dbeta, fus.sum_rows[ui])
    else:
        # without a residual input the ReLU mask is recomputed from y (one tensor less to read in both passes)
        dy, g = ops.bn_train_backward(dz, y, z if u.res is not None else None, stats, gamma, inv, dgamma, dbeta,
                                      want_g=u.res is not None, accumulate=True, relu=u.relu, beta=beta)
    if u.res is not None and u.res not in dead:
        grads[u.res] = g if u.res not in grads else grads[u.res] + g
    xin = acts[u.src]
    rec = dict(ui=ui, dz=dz, dy=dy, g=g, dx_prev=grads.get(u.src), dx=None) if trace is not None else None
    dw = store.target(conv.weight)
    if u.first:
        ops.stem_conv0_wgrad(xin, dy, inv, out=dw, accumulate=True)
    else:
        producer = None
        if xin is None:         # the input activation was never stored (_deferred_units): re-formed from its producer's y
            pi = [i for i, p_ in enumerate(units) if p_.dst == u.src][0]
            producer = (units[pi], tape[pi])
            xin = tape[pi][0]
        wgrad(xin, dy, conv.kernel_size[0], conv.stride[0], inv, [(dw, 0, conv.out_channels)], producer)
        if u.src in dead:          # the input is a frozen activation: no data gradient
            pass
        elif fus is not None and ui in fus.fed and u.src not in grads:       # (a 1x1 stride-1 conv)
            pu, (py, pstats) = units[fus.fed[ui]], tape[fus.fed[ui]]
            grads[u.src], fus.sum_rows[fus.fed[ui]] = ops.conv1x1_dgrad_bn_bwd_sums(
                dy, packs(conv.weight, True), zeros(conv.in_channels), py, pstats, pu.norm.weight.detach(), pu.norm.bias.detach())
        else:
            grads[u.src] = _data_gradient(conv, dy, xin.size(1), xin.size(2), grads.get(u.src), packs, zeros, sw)
        if rec is not None:
            rec['dx'] = grads.get(u.src)
    if rec is not None:      # this unit's own contribution (the buffers accumulate over shared modules)
        rec.update(dgamma=dgamma - snap[0], dbeta=dbeta - snap[1], dw=dw - snap[2])
        trace.append(rec)


def _wgrad_accumulate(xin, dy, ks, st, inv, targets, producer=None):
    """the conv's weight gradient, formed now and added into its target (the parameter's gradient buffer)"""
    ops.conv_wgrad(xin, dy, ks, st, inv, out=targets[0][0], accumulate=True)


def _units_backward(units, order, saved, grads, dead, store, packs, zeros, inv, sw, trace=None):
    """the backward of the units `order` (indices into `units`, last to first) whose activation has a gradient in `grads`: the
    serial path of the backbone, of the pyramid neck's units and of the detector heads.  A missing gradient buffer is zero-filled
    before the unit's first kernel (the whole-network schedule fills it where it is used)."""
    for ui in order:
        u = units[ui]
        dz = grads.pop(u.dst, None)
        if dz is None or u.frozen:
            continue
        for p in (u.norm.weight, u.norm.bias, u.conv.weight):
            store.target(p)
        _unit_backward(ui, u, dz, units, saved, grads, dead, store, packs, zeros, inv, sw, _wgrad_accumulate, trace=trace)


def backward(units, saved, grads, scale=None, store=None, trace=None):
    """grads: {activation index: dL/dact NHWC fp16 multiplied by `scale`} for the activations consumed outside the units
    (taps for the backbone alone, tower outputs for the whole network).  -> _GradStore of fp32 parameter gradients.
    trace: optional list that receives the per-unit tensors (tests check every unit against PyTorch given the same
    inputs)."""
    sw = switches()
    scale = loss_scale() if scale is None else scale
    inv = 1.0 / scale
    grads = dict(grads)
    store = store if store is not None else _GradStore()
    zeros = _Zeros(saved[0][0].device)
    packs = _Packs(units, True)
    _units_backward(units, reversed(range(len(units))), saved, grads, dead_activations(units), store, packs, zeros, inv, sw, trace)
    return store


# ---------------------------------------------------------------------------------------------- output convs
def _out_weight(o):
    """rows of the level's output convs concatenated and zero-padded to 64 (the narrowest 1x1 conv shape instantiated
    for 128 input channels, forward and data gradient) or, above 64 rows, to 128: [rows, C, 1, 1], bias [rows]"""
    w = torch.cat([c.weight.detach() for _, c in o.convs], 0)
    bias = torch.cat([c.bias.detach() for _, c in o.convs], 0)
    rows = -(-w.size(0) // 64) * 64
    wp = torch.zeros((rows,) + tuple(w.shape[1:]), dtype=torch.float32, device=w.device)
    wp[:w.size(0)] = w
    bp = torch.zeros(rows, dtype=torch.float32, device=w.device)
    bp[:bias.numel()] = bias
    return wp, bp


def _fused_outputs():
    """A/B switch: LFD_OUT_FUSED=0 runs the glue around the output convs as PyTorch ops (~25 launches per level)"""
    return switches().out_fused


def _out_segs(o):
    segs, r0 = [], 0
    for kind, conv in o.convs:
        segs.append(dict(kind=kind, conv=conv, channels=conv.out_channels, row0=r0,
                         scale=o.scale._scale.detach() if (kind == 'reg' and o.scale is not None) else None))
        r0 += conv.out_channels
    return segs


def out_row_ranges(o):
    """[(conv, first row, end row)] of an output record's convs inside its padded conv"""
    return [(sg['conv'], sg['row0'], sg['row0'] + sg['channels']) for sg in _out_segs(o)]


def _out_targets(o, store):
    """where the rows of the padded conv's weight gradient go (as ops.WgradFinals.add_wgrad takes them): a padded buffer never
    reaches a parameter gradient"""
    return [(store.target(cv.weight), lo, hi) for cv, lo, hi in out_row_ranges(o)]


def _level_starts(sizes):
    """-> (first point of every pyramid level in the level-concatenated [N, P, C] layout, P)"""
    starts, p = [], 0
    for h, w_ in sizes:
        starts.append(p)
        p += h * w_
    return starts, p


def _alloc_full(outs, n, p, dev):
    """the level-concatenated fp32 prediction tensors {'cls': [N, P, C'], 'reg': [N, P, 4]}"""
    width = {}
    for o in outs:
        for kind, conv in o.convs:
            width[kind] = conv.out_channels
    return {k: torch.empty((n, p, c), dtype=torch.float32, device=dev) for k, c in width.items()}


def _out_forward(o, x, wp, bp, wpk, full, start):
    """the padded conv of one level's output convs, then one launch (ops.head_out_split) that writes its rows straight into the
    level-concatenated tensors; -> y, kept for the backward"""
    y = ops.conv2d_nhwc(x, wpk, bp, x.size(3), wp.size(0), 1, 1, False)
    segs = _out_segs(o)
    ops.head_out_split(y, segs, [full[sg['kind']] for sg in segs], start)
    return y


def _out_backward(o, x, y, wp, dpack, full, start, store, scale, zeros, wgrad, grads):
    """the backward of _out_forward: bias / Scale gradients and dy in one launch, wgrad(o, wp, x, dy) for the padded weight, the
    data gradient (dpack(): the padded weight's data-gradient pack) added to what `grads` holds for the level's activation"""
    segs = _out_segs(o)
    for sg in segs:
        sg['dbias'] = store.target(sg['conv'].bias)
        sg['dscale'] = store.target(o.scale._scale) if sg['scale'] is not None else None
    dy = ops.head_out_grad(y, segs, [full[sg['kind']] for sg in segs], start, scale)
    wgrad(o, wp, x, dy)
    c = x.size(3)
    grads[o.src] = ops.conv2d_nhwc(dy, dpack(), zeros(c), wp.size(0), c, 1, 1, False, residual=grads.get(o.src))


def _outputs_forward_fused(outs, acts, num_levels):
    """outputs_forward with one launch per level behind the padded conv writing straight into the level-concatenated tensors"""
    sizes = [None] * num_levels
    for o in outs:
        sizes[o.level] = tuple(acts[o.src].shape[1:3])
    starts, p = _level_starts(sizes)
    x0 = acts[outs[0].src]
    full = _alloc_full(outs, x0.size(0), p, x0.device)
    cache, saved = {}, []
    for o in outs:
        key = tuple(id(cv) for _, cv in o.convs)
        if key not in cache:
            wp, bp = _out_weight(o)
            cache[key] = (wp, bp, ops.pack_conv_weight_train(wp))
        wp, bp, wpk = cache[key]
        saved.append((wp, _out_forward(o, acts[o.src], wp, bp, wpk, full, starts[o.level])))
    return full['cls'], full['reg'], sizes, saved


def _outputs_backward_fused(outs, acts, saved, sizes, dcls, dreg, store, scale):
    grads = {}
    inv = 1.0 / scale
    starts, _ = _level_starts(sizes)
    zeros = _Zeros(dcls.device)
    packs = _Packs()
    full = {'cls': dcls.contiguous(), 'reg': dreg.contiguous()}
    dws = {}

    def wgrad(o, wp, x, dy):
        key = tuple(id(cv) for _, cv in o.convs)
        if key not in dws:         # one padded weight-gradient buffer per set of (possibly shared) output convs
            dws[key] = (torch.zeros_like(wp), o)
        ops.conv_wgrad(x, dy, 1, 1, inv, out=dws[key][0], accumulate=True)

    for o, (wp, y) in zip(outs, saved):
        _out_backward(o, acts[o.src], y, wp, lambda: packs(wp, True), full, starts[o.level], store, scale, zeros, wgrad, grads)
    for dw, o in dws.values():
        r0 = 0
        for _, conv in o.convs:
            store.add(conv.weight, dw[r0:r0 + conv.out_channels])
            r0 += conv.out_channels
    return grads


def outputs_forward(outs, acts, num_levels):
    """-> (cls [N,P,C'], reg [N,P,4]) fp32 in the level-concatenated layout of LFD.forward (lfd.py:526-542), sizes per level,
    and what the backward needs."""
    if switches().out_fused:
        return _outputs_forward_fused(outs, acts, num_levels)
    cls_l, reg_l, sizes, saved = [None] * num_levels, [None] * num_levels, [None] * num_levels, []
    cache = {}
    for o in outs:
        x = acts[o.src]
        n, h, w_, c = x.shape
        key = tuple(id(cv) for _, cv in o.convs)           # shared heads: one concatenation + pack for all levels
        if key not in cache:
            wp, bp = _out_weight(o)
            cache[key] = (wp, bp, ops.pack_conv_weight_train(wp))
        wp, bp, wpk = cache[key]
        y = ops.conv2d_nhwc(x, wpk, bp, c, wp.size(0), 1, 1, False).view(n, h * w_, wp.size(0))
        r0 = 0
        raw = None
        for kind, conv in o.convs:
            t = y[..., r0:r0 + conv.out_channels].float()
            r0 += conv.out_channels
            if kind == 'cls':
                cls_l[o.level] = t
            else:
                raw = t
                reg_l[o.level] = t * o.scale._scale.detach() if o.scale is not None else t
        sizes[o.level] = (h, w_)
        saved.append((wp, raw))
    return torch.cat(cls_l, 1), torch.cat(reg_l, 1), sizes, saved


def outputs_backward(outs, acts, saved, sizes, dcls, dreg, store, scale=None):
    """-> {activation index: scaled fp16 gradient} for the tower outputs; parameter gradients go to `store`."""
    grads = {}
    scale = loss_scale() if scale is None else scale
    if saved and saved[0][1] is not None and saved[0][1].dtype == torch.float16:      # saved by _outputs_forward_fused
        return _outputs_backward_fused(outs, acts, saved, sizes, dcls, dreg, store, scale)
    inv = 1.0 / scale
    starts, _ = _level_starts(sizes)
    zeros = _Zeros(dcls.device)
    packs = _Packs()
    for o, (wp, raw) in zip(outs, saved):
        x = acts[o.src]
        n, h, w_, c = x.shape
        lo, hi = starts[o.level], starts[o.level] + h * w_
        parts = []
        for kind, conv in o.convs:
            if kind == 'cls':
                d = dcls[:, lo:hi]
            else:
                d = dreg[:, lo:hi]
                if o.scale is not None:
                    store.add(o.scale._scale, (d * raw).sum())
                    d = d * o.scale._scale.detach()
            store.add(conv.bias, d.sum((0, 1)))
            parts.append(d)
        rows = wp.size(0)
        dy = torch.zeros((n, h, w_, rows), dtype=torch.float16, device=x.device)
        r0 = 0
        for d in parts:
            dy.view(n, h * w_, rows)[..., r0:r0 + d.size(2)] = (d * scale).half()
            r0 += d.size(2)
        dw = ops.conv_wgrad(x, dy, 1, 1, inv)
        r0 = 0
        for _, conv in o.convs:
            store.add(conv.weight, dw[r0:r0 + conv.out_channels])
            r0 += conv.out_channels
        grads[o.src] = ops.conv2d_nhwc(dy, packs(wp, True), zeros(c), rows, c, 1, 1, False, residual=grads.get(o.src))
    return grads


# ---------------------------------------------------------------------------------------------- whole-network schedule
# Round 4.  An iteration of the shipped configurations was ~500 launches of which ~360 ran for less than 12 us (small maps,
# one-wave finals): 2.3 ms of a 7.4 ms iteration as ONE dependent chain (tools/timing/train_trace.py).  What this schedule does
# about it, on ONE stream (side streams inside a HIP graph measured slower: tools/negative_results/train_streams.py.txt):
#   * a weight gradient is needed by nobody until the optimizer: every k_wgrad writes its per-workgroup partial sums into its
#     OWN persistent buffer and ONE launch sums all of them at the end (ops.WgradFinals) -- 49 final launches become one; a conv
#     shared by the pyramid levels is a chain of partial sets summed with one rounding;
#   * the shared head runs level-concatenated (below): 150 launches per iteration become ~70.


class _Sched(object):
    """persistent buffers and job tables of one training plan on one device"""

    def __init__(self, dev):
        self.dev = dev
        self.bufs = {}
        self.finals = ops.WgradFinals(dev)
        self.gather = ops.WgradFinals(dev)      # (its row-sum table with one source row = a batched copy)

    def buf(self, key, numel, dtype=torch.float32):
        """a buffer that keeps its address from iteration to iteration (partial sums of the weight gradients).  One buffer per
        (key, size): captured training graphs and the job tables of the batched finals hold these addresses, and a batch of
        another shape (the short last batch of an epoch goes through the eager train_step on the same model) must not free
        what a later replay writes into -- it gets its own buffers, both sets stay."""
        k = (key, int(numel), dtype)
        t = self.bufs.get(k)
        if t is None:
            t = torch.empty(numel, dtype=dtype, device=self.dev)
            self.bufs[k] = t
        return t


def _sched(plan_owner, dev):
    sc = plan_owner.__dict__.get('_lfd_train_sched')
    if sc is None or sc.dev != dev:
        sc = _Sched(dev)
        plan_owner.__dict__['_lfd_train_sched'] = sc
    return sc


def _wgrad_partials(sc, key, xin, dy, ks, st, inv, targets, producer=None):
    """the per-workgroup partial sums of a conv's weight gradient into the conv's own persistent buffer sc.buf(key, ..); ONE
    launch sums the partials of all convs registered this way (sc.finals.launch()) and routes their rows to `targets` (as
    ops.WgradFinals.add_wgrad).  producer = (unit, (y, stats)): xin is that unit's pre-normalisation output, its activation was
    never stored (_deferred_units)"""
    floats, nwg, nblk = ops.conv_wgrad_partial_floats(xin, dy, ks, st)
    part = sc.buf(key, floats)
    if producer is not None:
        pu, (_, pstats) = producer
        ops.conv1x1_wgrad_partials_of_bn_relu(xin, pstats, pu.norm.weight.detach(), pu.norm.bias.detach(), dy, part)
    else:
        ops.conv_wgrad_partials(xin, dy, ks, st, part)
    sc.finals.add_wgrad(part, nwg, nblk, xin.size(3), dy.size(3), ks * ks, inv, targets)


def _out_packs(sc, outs, rows=None):
    """{ids of a level's output convs: (padded weight [rows, C, k, k], padded bias [rows], forward pack, data-gradient pack), rows
    64 or 128; k = 1 for LFDHead, 3 for FCOSHead}: the
    rows of the convs are gathered into persistent zero-padded buffers by ONE launch (lfd_rows_sum_batched_f32 with one source
    row = a batched copy), then packed; shared heads: once for all levels.  rows: one row count for every conv (the LFD detector
    node, whose glue takes both convs of a level in one launch) instead of each conv's own"""
    cache, jobs = {}, []
    for o in outs:
        key = tuple(id(cv) for _, cv in o.convs)
        if key in cache:
            continue
        c = o.convs[0][1].in_channels
        nrows = rows or -(-sum(cv.out_channels for _, cv in o.convs) // 64) * 64
        wp = sc.bufs.get(('outw', key))
        if wp is None:
            wp = torch.zeros((nrows,) + tuple(o.convs[0][1].weight.shape[1:]), dtype=torch.float32, device=sc.dev)
            sc.bufs[('outw', key)] = wp
            sc.bufs[('outb', key)] = torch.zeros(nrows, dtype=torch.float32, device=sc.dev)
        bp = sc.bufs[('outb', key)]
        r0 = 0
        for _, cv in o.convs:
            n_ = cv.out_channels
            jobs.append((cv.weight.detach(), wp[r0:r0 + n_]))
            jobs.append((cv.bias.detach(), bp[r0:r0 + n_]))
            r0 += n_
        cache[key] = [wp, bp]
    fin = sc.gather
    fin.reset()
    for src, dst in jobs:
        fin.add_rowsum(src, 1, src.numel(), src.numel(), dst, False)
    fin.launch()
    for v in cache.values():
        v.extend((ops.pack_conv_weight_train(v[0]), ops.pack_conv_weight_train(v[0], data_gradient=True)))
    return cache


def _out_pack(o, cache):
    return cache[tuple(id(cv) for _, cv in o.convs)]


# Level-concatenated head (round 4).  The shipped heads apply the SAME tower modules to every pyramid level (lfd_head.py:67-82,
# :164-185).  Per level that is 11 launches forward and 19 backward, 150 per iteration, most of them ~5 us kernels on the small
# levels.  With the levels of an image stored back to back -- [N, P, C], the point order LFD.forward returns anyway (lfd.py:526-542)
# -- a shared 1x1 conv, its weight gradient and its data gradient are ONE launch over all levels (a 1x1 conv does not care which
# pixel belongs to which level), GroupNorm takes its statistics per (image, level) segment (ops.gn_train_*_seg), and only the
# per-level modules stay per level: the neck units (own weights / BatchNorm; they write into / read from the concatenated tensor)
# and the glue of the output convs (per-level Scale).  Used when the head has this structure (every shipped configuration);
# CONCAT_HEAD = False, or a head whose levels do not share their towers, runs the same launches level by level.
CONCAT_HEAD = True


def _concat_layout(units, outs, nlev):
    """-> None, or the structure of a head whose towers and output convs are shared by all levels"""
    lv_units = [[ui for ui, u in enumerate(units) if u.level == l] for l in range(nlev)]
    k = len(lv_units[0]) if lv_units else 0
    if nlev < 2 or k < 2 or any(len(v) != k for v in lv_units):
        return None
    pos_of = [dict((units[ui].dst, p_) for p_, ui in enumerate(lv_units[l])) for l in range(nlev)]
    for p_ in range(k):
        u0 = units[lv_units[0][p_]]
        for l in range(nlev):
            u = units[lv_units[l][p_]]
            if u.res is not None or u.first or tuple(u.conv.kernel_size) != (1, 1) or tuple(u.conv.stride) != (1, 1) or not u.relu:
                return None
            if p_ == 0:      # the level's own neck unit on its backbone tap
                if not isinstance(u.norm, nn.BatchNorm2d) or u.src in pos_of[l] or u.conv.out_channels != u0.conv.out_channels:
                    return None
            else:
                if u.conv is not u0.conv or u.norm is not u0.norm or not isinstance(u.norm, nn.GroupNorm):
                    return None
                if pos_of[l].get(u.src) is None or pos_of[l].get(u.src) != pos_of[0].get(u0.src):
                    return None
    lv_outs = [[o for o in outs if o.level == l] for l in range(nlev)]
    m = len(lv_outs[0])
    if m < 1 or any(len(v) != m for v in lv_outs):
        return None
    for j in range(m):
        o0 = lv_outs[0][j]
        for l in range(nlev):
            o = lv_outs[l][j]
            if [id(cv) for _, cv in o.convs] != [id(cv) for _, cv in o0.convs]:
                return None
            if pos_of[l].get(o.src) is None or pos_of[l].get(o.src) != pos_of[0].get(o0.src):
                return None
    return dict(lv_units=lv_units, npos=k, src_pos=[None] + [pos_of[0][units[lv_units[0][p_]].src] for p_ in range(1, k)],
                out_src=[pos_of[0][lv_outs[0][j].src] for j in range(m)], lv_outs=lv_outs)


def _as_image(t):
    """[N, P, C] -> [1, H, W, C] view with N * P = H * W: how a 1x1 conv kernel sees the concatenated pixels (None: no usable W)"""
    total = t.size(0) * t.size(1)
    for w_ in (256, 128, 64, 32, 16):
        if total % w_ == 0:
            return t.view(1, total // w_, w_, t.size(2))
    return None


def _concat_forward(cl, units, outs, acts, tape, packs, opk, zeros, sw, full, sizes, starts, n, dev, sc=None):
    """neck units per level into A[0]; shared tower units over all levels; output convs over all levels + per-level slices"""
    seg_hw = [h_ * w_ for h_, w_ in sizes]
    ptot = sum(seg_hw)
    A, Y = [None] * cl['npos'], [None] * cl['npos']
    c0 = units[cl['lv_units'][0][0]].conv.out_channels
    A[0] = torch.empty((n, ptot, c0), dtype=torch.float16, device=dev)
    if _as_image(A[0]) is None:
        return None
    # the neck units: independent of each other -- every conv leaves its statistics rows in a buffer of its own, then TWO launches
    # finish all levels (per-channel finals; apply passes into A[0]) instead of two per level (LFD_BN_LEVELS=0; the same values)
    pending = []
    batched = sw.conv_bn_stats and sc is not None and sw.bn_levels
    for l in range(len(sizes)):
        ui = cl['lv_units'][l][0]
        u = units[ui]
        conv, norm = u.conv, u.norm
        xin = acts[u.src]
        if batched and all(id(norm) != id(units[q[1]].norm) for q in pending):      # (a norm shared by two levels: one after the other)
            rows = sc.buf(('bnrows', l), 512 * 2 * conv.out_channels)
            r = ops.conv2d_bn_partials(xin, packs(conv.weight), zeros(conv.out_channels), conv.in_channels, conv.out_channels, 1, 1, rows)
            if r is not None:
                pending.append((l, ui, (starts[l], r[0], rows, r[1], norm.eps, norm.momentum, norm.running_mean, norm.running_var,
                                        norm.weight.detach(), norm.bias.detach())))
                continue
        if sw.conv_bn_stats:
            y, stats = ops.conv2d_bn_stats(xin, packs(conv.weight), zeros(conv.out_channels), conv.in_channels, conv.out_channels, 1, 1,
                                           norm.eps, norm.momentum, norm.running_mean, norm.running_var)
        else:
            y = ops.conv2d_nhwc(xin, packs(conv.weight), zeros(conv.out_channels), conv.in_channels, conv.out_channels, 1, 1, False)
            stats = ops.bn_train_stats(y, norm.eps, norm.momentum, norm.running_mean, norm.running_var)
        ops.bn_train_apply_into(y, stats, norm.weight.detach(), norm.bias.detach(), True, A[0], starts[l])
        tape[ui] = (y, stats)
    if pending:
        sts = ops.bn_train_finish_into_levels([t[2] for t in pending], n, True, A[0])
        for (l, ui, lvl), st_ in zip(pending, sts):
            tape[ui] = (lvl[1], st_)
    for p_ in range(1, cl['npos']):
        u = units[cl['lv_units'][0][p_]]
        conv, norm = u.conv, u.norm
        xin = _as_image(A[cl['src_pos'][p_]])
        y = ops.conv2d_nhwc(xin, packs(conv.weight), zeros(conv.out_channels), conv.in_channels, conv.out_channels, 1, 1, False)
        y = y.view(n, ptot, conv.out_channels)
        stats, A[p_] = ops.gn_train_stats_apply_seg(y, seg_hw, norm.num_groups, norm.eps, norm.weight.detach(), norm.bias.detach(), True)
        Y[p_] = (y, stats)
    yo = []
    for j, sp in enumerate(cl['out_src']):
        o0 = cl['lv_outs'][0][j]
        wp, bp, wpk, _ = _out_pack(o0, opk)
        xin = _as_image(A[sp])
        y = ops.conv2d_nhwc(xin, wpk, bp, xin.size(3), wp.size(0), 1, 1, False).view(n, ptot, wp.size(0))
        lv = []
        for l in range(len(sizes)):
            segs = _out_segs(cl['lv_outs'][l][j])
            lv.append((seg_hw[l], starts[l], segs, [full[sg['kind']] for sg in segs]))
        if sw.head_out_levels:
            ops.head_out_split_levels(y, lv)          # all levels (their own Scale each) in one launch
        else:
            for hw_, p0_, segs, outs_ in lv:
                ops.head_out_split_concat(y, hw_, segs, outs_, p0_)
        yo.append(y)
    return dict(A=A, Y=Y, yo=yo, seg_hw=seg_hw, ptot=ptot)


def _concat_backward(cl, cs, units, acts, tape, packs, opk, zeros, sw, full, starts, store, wgrad, grads, scale, inv, n, dev, dead=()):
    """the backward of _concat_forward; leaves the gradients of the backbone taps in `grads` (none for a tap in `dead`: the
    output of a frozen unit)"""
    A, Y, seg_hw, ptot = cs['A'], cs['Y'], cs['seg_hw'], cs['ptot']
    dA = [None] * cl['npos']
    nlev = len(seg_hw)
    for j, sp in enumerate(cl['out_src']):
        o0 = cl['lv_outs'][0][j]
        wp = _out_pack(o0, opk)[0]
        y = cs['yo'][j]
        dyo = torch.empty_like(y)
        lv = []
        for l in range(nlev):
            o = cl['lv_outs'][l][j]
            segs = _out_segs(o)
            for sg in segs:
                sg['dbias'] = store.target(sg['conv'].bias)
                sg['dscale'] = store.target(o.scale._scale) if sg['scale'] is not None else None
            lv.append((seg_hw[l], starts[l], segs, [full[sg['kind']] for sg in segs]))
        if sw.head_out_levels:
            ops.head_out_grad_levels(y, lv, scale, dyo)        # all levels in one launch + one final
        else:
            for hw_, p0_, segs, grads_ in lv:
                ops.head_out_grad_concat(y, hw_, segs, grads_, p0_, scale, dyo)
        xin, dy4 = _as_image(A[sp]), _as_image(dyo)
        wgrad(xin, dy4, 1, 1, inv, _out_targets(o0, store))
        c = xin.size(3)
        res = _as_image(dA[sp]) if dA[sp] is not None else None
        dA[sp] = ops.conv2d_nhwc(dy4, _out_pack(o0, opk)[3], zeros(c), wp.size(0), c, 1, 1, False, residual=res).view(n, ptot, c)
    for p_ in range(cl['npos'] - 1, 0, -1):
        if dA[p_] is None:
            continue
        u = units[cl['lv_units'][0][p_]]
        conv, norm = u.conv, u.norm
        y, stats = Y[p_]
        dy = ops.gn_train_backward_seg(dA[p_], y, A[p_], seg_hw, norm.num_groups, stats, norm.weight.detach(), inv,
                                       store.target(norm.weight), store.target(norm.bias), True)
        dA[p_] = None
        sp = cl['src_pos'][p_]
        xin, dy4 = _as_image(A[sp]), _as_image(dy)
        wgrad(xin, dy4, 1, 1, inv, [(store.target(conv.weight), 0, conv.out_channels)])
        cin = conv.in_channels
        res = _as_image(dA[sp]) if dA[sp] is not None else None
        dA[sp] = ops.conv2d_nhwc(dy4, packs(conv.weight, True), zeros(cin), conv.out_channels, cin, 1, 1, False,
                                 residual=res).view(n, ptot, cin)
    # the neck units' BatchNorm backward: the levels are independent of each other -- three launches for all of them
    # (LFD_BN_LEVELS=0: three per level; the same values)
    dys = None
    if sw.bn_levels:
        lv = []
        for l in range(nlev):
            u = units[cl['lv_units'][l][0]]
            y, stats = tape[cl['lv_units'][l][0]]
            lv.append((starts[l], y, stats, u.norm.weight.detach(), u.norm.bias.detach(), store.target(u.norm.weight),
                       store.target(u.norm.bias)))
        if len({t[5].data_ptr() for t in lv}) == len(lv):       # (levels sharing one norm module would race on its gradient)
            dys = ops.bn_train_backward_from_levels(dA[0], lv, inv, relu=True, accumulate=True)
    for l in range(nlev - 1, -1, -1):
        ui = cl['lv_units'][l][0]
        u = units[ui]
        conv, norm = u.conv, u.norm
        y, stats = tape[ui]
        dy = dys[l] if dys is not None else ops.bn_train_backward_from(
            dA[0], starts[l], y, stats, norm.weight.detach(), norm.bias.detach(), inv, store.target(norm.weight),
            store.target(norm.bias), relu=True, accumulate=True)
        xin = acts[u.src]
        wgrad(xin, dy, 1, 1, inv, [(store.target(conv.weight), 0, conv.out_channels)])
        cin = conv.in_channels
        if u.src in dead:
            continue
        grads[u.src] = ops.conv2d_nhwc(dy, packs(conv.weight, True), zeros(cin), conv.out_channels, cin, 1, 1, False,
                                       residual=grads.get(u.src))


def _deferred_units(units, outs, sw=None):
    """-> {index of a unit whose activation is never stored: index of its only consumer}.  A BatchNorm + ReLU unit without a
    residual whose output feeds exactly one 1x1 stride-1 conv unit (the first conv of each stem pair, lfd_resnet.py:376-413):
    the consumer normalises its operand inside the conv kernel (ops.conv1x1_of_bn_relu_bn_stats) and its weight gradient
    re-forms it (ops.conv1x1_wgrad_partials_of_bn_relu) -- one write and one read of the largest tensors of the iteration less.
    LFD_BN_APPLY_IN_CONV=0: every unit stores its activation."""
    if not (sw or switches()).bn_apply_in_conv:
        return {}
    return _stem_pairs(units, outs)


def _stem_pairs(units, outs):
    """the structural part of _deferred_units: {producer unit index: index of its only consumer, a 1x1 stride-1 conv unit}"""
    out = {}
    for ui, vi in _single_consumers(units, outs).items():
        v = units[vi]
        if units[ui].frozen or units[ui].eval_norm or v.frozen or v.eval_norm:
            continue             # the pair fusions take batch statistics from the conv epilogues: training-mode norms only
        if (isinstance(v.norm, nn.BatchNorm2d) and v.conv.kernel_size[0] == 1 and v.conv.stride[0] == 1
                and v.conv.in_channels == 64 and v.conv.out_channels in (64, 128)):     # (the kernel's two instances: ADVICE r4)
            out[ui] = vi
    return out


def _single_consumers(units, outs):
    """{index of a BatchNorm + ReLU unit without residual: index of the ONE unit that reads its activation} (backbone / neck
    units only; activations that are also pyramid taps, residual inputs or output-conv inputs do not qualify)"""
    uses = {}
    for vi, v in enumerate(units):
        uses.setdefault(v.src, []).append(vi)
        if v.res is not None:
            uses.setdefault(v.res, []).append(-1)
    for o in outs:
        uses.setdefault(o.src, []).append(-1)
    out = {}
    for ui, u in enumerate(units):
        if not (isinstance(u.norm, nn.BatchNorm2d) and u.relu and u.res is None and u.level is None):
            continue
        cons = uses.get(u.dst, [])
        if len(cons) != 1 or cons[0] < 0:
            continue
        v = units[cons[0]]
        if v.level is None and not v.first:
            out[ui] = cons[0]
    return out


def network_forward(model, plan, x):
    """-> (cls [N,P,C'], reg [N,P,4], sizes, saved): LFD.forward in train mode (lfd.py:511-542) over the unit schedule"""
    sw = switches()
    units, outs, nlev = plan
    dev = x.device
    sc = _sched(model, dev)
    acts, tape = {0: x}, [None] * len(units)
    zeros = _Zeros(dev)
    packs = _Packs(units, False)
    opk = _out_packs(sc, outs)
    hw = {0: (x.size(2), x.size(3))}
    for u in units:
        k, st_ = u.conv.kernel_size[0], u.conv.stride[0]
        h_, w_ = hw[u.src]
        hw[u.dst] = ((h_ + 2 * (k // 2) - k) // st_ + 1, (w_ + 2 * (k // 2) - k) // st_ + 1)
    sizes = [None] * nlev
    for o in outs:
        sizes[o.level] = hw[o.src]
    starts, p = _level_starts(sizes)
    full = _alloc_full(outs, x.size(0), p, dev)
    cl = None
    if CONCAT_HEAD:
        cl = model.__dict__.get('_lfd_concat_layout', 0)
        if cl == 0:
            cl = _concat_layout(units, outs, nlev)
            model.__dict__['_lfd_concat_layout'] = cl
    cs = None
    defer = _deferred_units(units, outs, sw) if sw.conv_bn_stats else {}
    fed = {v: u for u, v in defer.items()}
    ev = _eval_norms(model, units) if any(u.eval_norm for u in units) else None
    for ui, u in enumerate(units):
        if u.level is None:
            tape[ui] = _unit_forward(ui, u, acts, packs, zeros, sw, ev, store=ui not in defer,
                                     producer=(units[fed[ui]], tape[fed[ui]]) if ui in fed else None)
    if cl is not None:
        cs = _concat_forward(cl, units, outs, acts, tape, packs, opk, zeros, sw, full, sizes, starts, x.size(0), dev, sc)
    osaved = cs
    if cs is None:     # level by level: heads that do not share their towers, or no usable image view of N * P pixels
        for ui, u in enumerate(units):
            if u.level is not None:
                tape[ui] = _unit_forward(ui, u, acts, packs, zeros, sw, ev)
        osaved = []
        for o in outs:
            wp, bp, wpk, _ = _out_pack(o, opk)
            osaved.append((wp, _out_forward(o, acts[o.src], wp, bp, wpk, full, starts[o.level])))
    _count_batches(units)
    return full['cls'], full['reg'], sizes, ((acts, tape), osaved, opk)


def network_backward(model, plan, saved, sizes, dcls, dreg, scale):
    """the backward of network_forward: parameter gradients accumulate into `.grad` (created zeroed when missing)."""
    sw = switches()
    units, outs, nlev = plan
    (acts, tape), osaved, opk = saved
    dev = dcls.device
    sc = _sched(model, dev)
    inv = 1.0 / scale
    store = _GradStore(in_place=True)
    fin = sc.finals
    fin.reset()
    zeros = _Zeros(dev)
    packs = _Packs(units, True)
    dcls, dreg = dcls.contiguous(), dreg.contiguous()
    full = {'cls': dcls, 'reg': dreg}
    starts, _ = _level_starts(sizes)
    nj = itertools.count()

    def wgrad(xin, dy, ks, st, inv, targets, producer=None):      # the schedule's j-th weight gradient: buffer ('wg', j)
        _wgrad_partials(sc, ('wg', next(nj)), xin, dy, ks, st, inv, targets, producer)

    def out_wgrad(o, wp, xo, dy):
        wgrad(xo, dy, 1, 1, inv, _out_targets(o, store))

    grads = {}
    # stem pairs (_stem_pairs, adjacent units only: nothing else may touch the training workspace in between): the 1x1 conv's
    # data gradient leaves the BatchNorm backward sums of the unit in front of it behind (LFD_BN_SUMS_IN_DGRAD=0: separate pass)
    fed = {}
    if sw.bn_sums_in_dgrad and sw.conv_bn_stats:
        fed = {v: u_ for u_, v in _stem_pairs(units, outs).items()
               if v == u_ + 1 and units[u_].conv.out_channels == 64 and units[v].conv.out_channels == 64}
    fus = _Fusions(fed, {})
    concat = isinstance(osaved, dict)
    dead = dead_activations(units)
    if concat:
        _concat_backward(model.__dict__['_lfd_concat_layout'], osaved, units, acts, tape, packs, opk, zeros, sw, full, starts, store,
                         wgrad, grads, scale, inv, dcls.size(0), dev, dead)
    # ---- output convs, level by level
    for o, (wp, y) in (() if concat else zip(outs, osaved)):
        _out_backward(o, acts[o.src], y, wp, lambda: _out_pack(o, opk)[3], full, starts[o.level], store, scale, zeros, out_wgrad, grads)
    # ---- conv / norm / ReLU units, last to first
    for ui in range(len(units) - 1, -1, -1):
        u = units[ui]
        if u.dst not in grads or (concat and u.level is not None):
            continue
        dz = grads.pop(u.dst)
        if not u.frozen:
            _unit_backward(ui, u, dz, units, (acts, tape), grads, dead, store, packs, zeros, inv, sw, wgrad, fus)
    fin.launch()


class BackboneTrainFunction(torch.autograd.Function):
    """taps (NCHW fp32) = backbone(x) as one autograd node (used when neck / head are not covered by network_supported)."""

    @staticmethod
    def forward(ctx, plan, x, *params):
        units, tap_ids = plan[:2]
        taps, saved = forward(units, tap_ids, x, plan[2] if len(plan) > 2 else None)
        ctx.plan, ctx.saved = plan, saved
        return tuple(t.permute(0, 3, 1, 2).float() for t in taps)

    @staticmethod
    def backward(ctx, *tap_grads):
        units, tap_ids = ctx.plan[:2]
        grads = {}
        scale = loss_scale()
        for t, g in zip(tap_ids, tap_grads):
            if g is not None:
                g16 = (g * scale).permute(0, 2, 3, 1).contiguous().half()
                grads[t] = g16 if t not in grads else grads[t] + g16
        backward(units, ctx.saved, grads, scale=scale, store=_GradStore(in_place=True))
        ctx.saved = None
        return (None, None) + (None,) * len(backbone_params(units))     # gradients were accumulated into .grad directly


class NetworkTrainFunction(torch.autograd.Function):
    """(cls [N,P,C'], reg [N,P,4]) = LFD.forward(x) in train mode as ONE autograd node: every conv / norm / ReLU of
    backbone, neck and head runs forward and backward on the hand-written kernels (network_forward / network_backward).
    sizes_out: the caller's list, which receives [(h, w)] per level."""

    @staticmethod
    def forward(ctx, model, plan, x, sizes_out, *params):
        cls, reg, sizes, saved = network_forward(model, plan, x)
        ctx.model, ctx.plan, ctx.saved, ctx.sizes = model, plan, saved, sizes
        ctx.shapes = (cls.shape, reg.shape)
        sizes_out.extend(sizes)
        return cls, reg

    @staticmethod
    def backward(ctx, dcls, dreg):
        units, outs, _ = ctx.plan
        dev = ctx.saved[0][0][0].device
        if dcls is None:
            dcls = torch.zeros(ctx.shapes[0], dtype=torch.float32, device=dev)
        if dreg is None:
            dreg = torch.zeros(ctx.shapes[1], dtype=torch.float32, device=dev)
        network_backward(ctx.model, ctx.plan, ctx.saved, ctx.sizes, dcls, dreg, loss_scale())
        ctx.saved = None
        return (None,) * (4 + len(network_params(units, outs)))   # accumulated into .grad directly


def backbone_train_forward(backbone, x):
    check_train_input(backbone, x)
    plan = backbone.__dict__.get('_lfd_train_plan')
    if plan is None:
        plan = build_units(backbone) + (backbone,)
        backbone.__dict__['_lfd_train_plan'] = plan
    return BackboneTrainFunction.apply(plan, x, *backbone_params(plan[0]))


def network_train_forward(model, x):
    """-> (cls, reg, [(h, w)] per level)"""
    check_train_input(model._backbone, x)
    plan = model.__dict__.get('_lfd_train_plan')
    if plan is None:
        units, outs = build_network(model)
        plan = (units, outs, model._num_heads)
        model.__dict__['_lfd_train_plan'] = plan
    sizes = []
    cls, reg = NetworkTrainFunction.apply(model, plan, x, sizes, *network_params(plan[0], plan[1]))
    return cls, reg, sizes


# ---------------------------------------------------------------------------------------------- backbone + pyramid neck
# FPN / SimpleFPN (lfd/model/neck/fpn.py:127-152, simple_fpn.py:141-172) behind the backbone in ONE autograd node: the taps stay
# NHWC fp16, the neck's convs / norms run on the kernels of the units, its element-wise operators on csrc/sibling.hip forward
# and csrc/sibling_train.hip backward.  The plan is a list of steps over activation indices (the units' numbering goes on):
#   ('unit', ui)                 lateral conv (no bias) -> norm -> ReLU?: a _Unit, through _unit_forward / _unit_backward
#   ('conv', _NeckConv)          conv + bias (-> ReLU): laterals without a norm, FPN's 3x3 smoothing convs, 'conv' extra levels
#   ('merge', dst, src, new)     new = dst + nearest_upsample(src), written over dst (a copy of dst is kept only when its
#                                producer's backward needs its own output as the ReLU mask)
#   ('relu', a, new)             nn.ReLU(inplace=True) in front of an extra level: a's tensor is rewritten, so EVERY consumer of
#                                it -- the head, which gets the previous output level -- sees relu(a)
#   ('pool', src, dst)           'pooling' extra level, MaxPool2d(3, 2, 1)
class _NeckConv(object):
    __slots__ = ('conv', 'relu', 'src', 'dst')
    first = frozen = False           # (what _Packs asks of a unit)


class _PyramidPlan(object):
    # n_act: the first activation index the plan does not use (the detector plan numbers the head's activations from it)
    __slots__ = ('bb_units', 'units', 'tap_ids', 'steps', 'out_ids', 'convs', 'params', 'owner', 'n_act')


def _lateral_parts(neck, i):
    """-> (conv, norm | None, relu) of lateral{i}: Sequential(conv, [norm], [ReLU])"""
    mods = list(getattr(neck, 'lateral%d' % i))
    norm = mods[1] if len(mods) > 1 and isinstance(mods[1], (nn.BatchNorm2d, nn.GroupNorm)) else None
    return mods[0], norm, isinstance(mods[-1], nn.ReLU)


def pyramid_supported(backbone, neck):
    """backbone + neck as one node (PyramidTrainFunction): a `supported` backbone under an FPN or a SimpleFPN (top-down or
    neighbouring_mode) whose taps and outputs have 64 or 128 channels, every parameter taking a gradient.  Lateral norm: none, a
    train-mode affine BatchNorm2d that tracks its statistics, or an affine GroupNorm in groups of 8 channels -- with or without
    relu_on_lateral: the GroupNorm backward kernel takes its ReLU mask from an optional stored output, so it has a form
    without a ReLU (lfd_gn_train_bwd_f16 with z == NULL) and nothing is refused on that account.  The combination autograd
    refuses -- ReLU laterals re-ReLU'd in place in front of an extra level -- is admitted: the second ReLU is the identity on
    values and its mask equals the first one's.  Everything else keeps the backbone node with the neck under autograd."""
    if type(neck).__name__ not in ('FPN', 'SimpleFPN') or not neck.training or not supported(backbone):
        return False
    chans = list(neck._num_input_channels_list) + [neck._num_output_channels]
    if any(c not in (64, 128) for c in chans) or list(backbone.num_output_channels_list) != list(neck._num_input_channels_list):
        return False
    if not all(p.requires_grad for p in neck.parameters()):
        return False
    for m in neck.modules():
        if isinstance(m, nn.Conv2d) and not (_conv_ok(m) and m.in_channels in (64, 128) and m.out_channels in (64, 128)):
            return False
    for i in range(neck._num_inputs):
        conv, norm, _ = _lateral_parts(neck, i)
        if (norm is None) != (conv.bias is not None):
            return False
        if isinstance(norm, nn.BatchNorm2d) and (norm.momentum is None or not norm.affine or not norm.track_running_stats
                                                 or not norm.training):
            return False
        if isinstance(norm, nn.GroupNorm) and (not norm.affine or norm.num_channels != 8 * norm.num_groups):
            return False
    return True


def build_pyramid(backbone, neck):
    """-> _PyramidPlan: the backbone's units, then the neck's steps in the order FPN.forward / SimpleFPN.forward run them"""
    b = _Builder()
    taps = _build_backbone(b, backbone)
    p = _PyramidPlan()
    p.bb_units, p.tap_ids, p.steps, p.convs, p.owner = list(b.units), taps, [], [], backbone

    def new_act():
        b.n_act += 1
        return b.n_act - 1

    def conv_step(conv, relu, src):
        nc = _NeckConv()
        nc.conv, nc.relu, nc.src, nc.dst = conv, relu, src, new_act()
        p.steps.append(('conv', nc))
        p.convs.append(nc)
        return nc.dst

    L = neck._num_inputs
    lat = []
    for i, tap in enumerate(taps):
        conv, norm, relu = _lateral_parts(neck, i)
        if norm is not None:
            lat.append(b.add(conv, norm, relu, tap))
            p.steps.append(('unit', len(b.units) - 1))
            p.convs.append(b.units[-1])
        else:
            lat.append(conv_step(conv, relu, tap))
    for i in (range(L - 1) if neck._bottom_up else range(L - 1, 0, -1)):
        dst, src = (i, i + 1) if neck._bottom_up else (i - 1, i)
        # top-down lat[src] is already merged, bottom-up it is not yet (its own merge is the next step): the index says which
        merged = new_act()
        p.steps.append(('merge', lat[dst], lat[src], merged))
        lat[dst] = merged
    outs = []
    for i in range(neck._num_outputs):
        mods = list(getattr(neck, 'fpn_out%d' % i))
        if i < L:
            outs.append(conv_step(mods[0], False, lat[i]) if mods else lat[i])
            continue
        from_input = i == L and neck._extra_on_input
        src = taps[-1] if from_input else outs[-1]
        if isinstance(mods[0], nn.ReLU):
            mods = mods[1:]
            if not from_input:          # (a backbone tap left a ReLU: the in-place ReLU changes neither it nor its gradient)
                r = new_act()
                p.steps.append(('relu', src, r))
                outs[-1] = src = r
        if isinstance(mods[0], nn.Conv2d):
            outs.append(conv_step(mods[0], False, src))
        else:
            d = new_act()
            p.steps.append(('pool', src, d))
            outs.append(d)
    p.units, p.out_ids, p.n_act = b.units, outs, b.n_act
    ps = backbone_params(b.units)
    for kind, *a in p.steps:
        if kind == 'conv':
            ps += [a[0].conv.weight, a[0].conv.bias]
    p.params = _unique(ps)
    return p


def _needs_own_output(plan, act):
    """does the backward of the step that produced `act` read act's own values (the ReLU mask)?  A BatchNorm unit recomputes the
    mask from its conv output; a GroupNorm unit and a conv + bias + ReLU step read the stored output."""
    for kind, *a in plan.steps:
        if kind == 'unit' and plan.units[a[0]].dst == act:
            u = plan.units[a[0]]
            return u.relu and isinstance(u.norm, nn.GroupNorm)
        if kind == 'conv' and a[0].dst == act:
            return a[0].relu
    return False


def pyramid_forward(plan, x):
    """-> (neck outputs NHWC fp16, saved)"""
    sw = switches()
    n_bb = len(plan.bb_units)
    _, (acts, tape) = forward(plan.bb_units, plan.tap_ids, x, plan.owner)
    tape = tape + [None] * (len(plan.units) - n_bb)
    zeros = _Zeros(x.device)
    packs = _Packs(plan.convs, False)
    for kind, *a in plan.steps:
        if kind == 'unit':
            tape[a[0]] = _unit_forward(a[0], plan.units[a[0]], acts, packs, zeros, sw)
        elif kind == 'conv':
            nc, cv = a[0], a[0].conv
            acts[nc.dst] = ops.conv2d_nhwc(acts[nc.src], packs(cv.weight), cv.bias.detach(), cv.in_channels, cv.out_channels,
                                           cv.kernel_size[0], cv.stride[0], nc.relu)
        elif kind == 'merge':
            dst, src, new = a
            t = acts[dst].clone() if _needs_own_output(plan, dst) else acts[dst]
            acts[new] = ops.upsample_nearest_add_(t, acts[src])
        elif kind == 'relu':
            acts[a[1]] = ops.relu_(acts[a[0]])
        else:
            acts[a[1]] = ops.maxpool3x3s2(acts[a[0]])
    _count_batches(plan.units[n_bb:])
    return [acts[o] for o in plan.out_ids], (acts, tape)


def pyramid_backward(plan, saved, grads, scale=None, store=None):
    """grads: {activation index: dL/d(neck output) NHWC fp16 times `scale`}.  The neck's steps last to first, then the backbone's
    units (backward); parameter gradients go to `store`."""
    sw = switches()
    scale = loss_scale() if scale is None else scale
    inv = 1.0 / scale
    acts, tape = saved
    grads = dict(grads)
    store = store if store is not None else _GradStore()
    zeros = _Zeros(acts[0].device)
    packs = _Packs(plan.convs, True)
    dead = dead_activations(plan.units)
    relu_made = {a[1] for kind, *a in plan.steps if kind == 'relu'}
    side = {}          # {ReLU'd activation: the gradient of the extra level behind it}: joined with the head's by the ReLU backward
    for kind, *a in reversed(plan.steps):
        if kind == 'unit':
            _units_backward(plan.units, a, saved, grads, dead, store, packs, zeros, inv, sw)       # (a: [the unit's index])
        elif kind == 'conv':
            nc, cv = a[0], a[0].conv
            dz = grads.pop(nc.dst, None)
            if dz is None:
                continue
            if nc.relu:
                dz = ops.relu_backward_add(acts[nc.dst], dz)
            xin = acts[nc.src]
            ops.bias_grad_(dz, inv, store.target(cv.bias))
            _wgrad_accumulate(xin, dz, cv.kernel_size[0], cv.stride[0], inv, [(store.target(cv.weight), 0, cv.out_channels)])
            if nc.src in dead:
                continue
            prev = None if nc.src in relu_made else grads.get(nc.src)
            gx = _data_gradient(cv, dz, xin.size(1), xin.size(2), prev, packs, zeros, sw)
            (side if nc.src in relu_made else grads)[nc.src] = gx
        elif kind == 'merge':
            dst, src, new = a
            g = grads.pop(new, None)
            if g is None:
                continue
            grads[dst] = g          # (dst has no other consumer: its tensor became `new`)
            if src not in grads:
                grads[src] = torch.zeros_like(acts[src])
            ops.upsample_nearest_add_backward_(grads[src], g)
        elif kind == 'relu':
            src, r = a
            g, gb = grads.pop(r, None), side.pop(r, None)
            if g is None and gb is None:
                continue
            if g is None:
                g, gb = gb, None
            grads[src] = ops.relu_backward_add(acts[r], g, gb, out=g)
        else:
            src, d = a
            g = grads.pop(d, None)
            if g is None:
                continue
            if src in relu_made:
                side[src] = ops.maxpool3x3s2_backward(acts[src], g)
            elif src not in dead:
                grads[src] = ops.maxpool3x3s2_backward(acts[src], g, grads.get(src))
    n_bb = len(plan.bb_units)
    return backward(plan.bb_units, (acts, tape[:n_bb]), grads, scale=scale, store=store)


class PyramidTrainFunction(torch.autograd.Function):
    """neck outputs (NCHW fp32) = neck(backbone(x)) as one autograd node: the taps never leave NHWC fp16 (used when the head is not
    covered by network_supported and pyramid_supported holds)."""

    @staticmethod
    def forward(ctx, plan, x, *params):
        outs, saved = pyramid_forward(plan, x)
        ctx.plan, ctx.saved = plan, saved
        return tuple(t.permute(0, 3, 1, 2).float() for t in outs)

    @staticmethod
    def backward(ctx, *out_grads):
        plan = ctx.plan
        grads = {}
        scale = loss_scale()
        for o, g in zip(plan.out_ids, out_grads):
            if g is not None:
                grads[o] = (g * scale).permute(0, 2, 3, 1).contiguous().half()
        pyramid_backward(plan, ctx.saved, grads, scale=scale, store=_GradStore(in_place=True))
        ctx.saved = None
        return (None, None) + (None,) * len(plan.params)     # gradients were accumulated into .grad directly


def backbone_neck_train_forward(backbone, neck, x):
    """-> the neck's outputs, NCHW fp32 (what `neck(backbone taps)` returns under autograd)"""
    check_train_input(backbone, x)
    plan = _pyramid_plan(backbone, neck)
    return PyramidTrainFunction.apply(plan, x, *plan.params)


def _pyramid_plan(backbone, neck):
    plan = neck.__dict__.get('_lfd_pyramid_plan')
    if plan is None or plan.owner is not backbone:
        plan = build_pyramid(backbone, neck)
        neck.__dict__['_lfd_pyramid_plan'] = plan
    return plan


# ---------------------------------------------------------------------------------------------- backbone + pyramid neck + head
# The detector node: an FCOSHead or an LFDHead behind the pyramid node, in the SAME autograd node.  One plan class, one forward,
# one backward, one Function (at the end of this file); a head brings its `*_head_supported`, the builder of its plan and its
# glue adapter: pack(plan, starts, raws, full) from the output convs' fp32 outputs into the node's level-concatenated outputs
# (-> what its backward keeps), grad(plan, starts, kept, read, dfull, dys, store, scale) back from the outputs' gradients to the
# convs' fp16 output gradients, the bias and the Scale gradients.
class _DetectorPlan(object):
    """The plan of the detector node, for both heads.  pyramid: the _PyramidPlan; units: the head's units of all levels (their own
    list: tape indices are positions in it, activation indices go on from the pyramid's); outs: the levels' _Out records in
    forward order; rows: the row count every output conv is padded to; ks: the output convs' kernel size; widths: {kind: channels}
    of the node's output tensors, in the order it returns them; glue: the adapter around the output convs (_FCOSGlue / _LFDGlue)"""
    __slots__ = ('pyramid', 'units', 'outs', 'rows', 'ks', 'widths', 'params', 'head', 'glue')


def _build_detector(backbone, neck, head, glue, ks, widths, level):
    """-> _DetectorPlan on the pyramid plan; level(b, i, src) adds the head's units of level i on the neck's output `src` to the
    builder and -> the level's _Out records"""
    pp = _pyramid_plan(backbone, neck)
    b = _Builder()
    b.n_act = pp.n_act
    d = _DetectorPlan()
    d.pyramid, d.outs, d.head, d.glue, d.ks, d.widths = pp, [], head, glue, ks, widths
    for i, src in enumerate(pp.out_ids):
        b.level = i
        d.outs += level(b, i, src)
    d.units = b.units
    d.rows = max(-(-sum(cv.out_channels for _, cv in o.convs) // 64) * 64 for o in d.outs)
    d.params = _plan_params(pp.params, d.units, d.outs)
    return d


# ---- FCOSHead (lfd/model/head/fcos_head.py:20-154): two towers of 3x3 conv ->
# GroupNorm -> ReLU units shared by all levels (through _unit_forward / _unit_backward: shared weights are packed once, every
# parameter gradient accumulates over the levels), then per level two output convs padded to FCOS_OUT_ROWS rows with fp32
# outputs (ops.conv2d_nhwc_f32out) -- rows [0, C) `_classification` and row C `_centerness` on the classification tower, rows
# [0, 4) `_regression` on the regression tower -- and csrc/fcos_out.hip on both sides of them.  The node returns what
# FCOS.get_loss reads: (cls [N,P,C], reg [N,P,4], ctr [N,P,1]) fp32, level-concatenated.
FCOS_OUT_ROWS = 64       # both tower widths: forward 128 -> 64 and 64 -> 64 are instances of csrc/conv_acc32.hip, the data gradient
#                          64 -> 128 and 64 -> 64 (3x3 stride 1) of csrc/conv.hip; the glue also has a 32-row form


def fcos_head_supported(backbone, neck, head):
    """backbone + neck + head as one node (DetectorTrainFunction): pyramid_supported(backbone, neck) and a training-mode FCOSHead
    with one Scale per neck output whose towers are num_layers >= 1 units of 3x3 conv -> affine GroupNorm in groups of 8
    channels -> ReLU, 64 or 128 input and head channels, every parameter taking a gradient, and
    num_classes + 1 <= FCOS_OUT_ROWS (classification and centerness share one padded conv).  NOT admitted -- these keep the
    pyramid node with the head under PyTorch-ROCm autograd: norm_cfg=None, BatchNorm towers (a BatchNorm shared by the levels
    updates its running statistics level after level: its own piece of work), num_layers == 0 and more classes.  (An LFDHead
    behind such a neck enters the same node through lfd_head_supported; LFDHeadV1 has none.)"""
    if type(head).__name__ != 'FCOSHead' or not head.training:
        return False
    if not pyramid_supported(backbone, neck) or len(head._scales) != neck._num_outputs:
        return False
    cfg = head._norm_cfg
    if cfg is None or cfg.get('type') != 'GroupNorm' or head._num_head_channels != 8 * cfg.get('num_groups', 0):
        return False
    if head._num_layers < 1 or head._num_input_channels not in (64, 128) or head._num_head_channels not in (64, 128):
        return False
    if head._num_input_channels != neck._num_output_channels:
        return False
    if any(isinstance(m, nn.GroupNorm) and not m.affine for m in head.modules()):
        return False
    if not all(p.requires_grad for p in head.parameters()):
        return False
    return head._num_classes + 1 <= FCOS_OUT_ROWS


def build_detector(backbone, neck, head):
    """-> _DetectorPlan of an FCOSHead: per level, in FCOSHead.forward's order (fcos_head.py:129-150), the classification tower's
    units, the regression tower's units and two output records, (cls + ctr) then (reg, with the level's Scale); 3x3 output convs
    of FCOS_OUT_ROWS rows (what fcos_head_supported admits fits them)"""
    try:
        cls_t, reg_t = netdesc.split_sequential(head._classification_path), netdesc.split_sequential(head._regression_path)
    except netdesc.UnknownModule as e:      # (fcos_head_supported admits conv -> GroupNorm -> ReLU towers only)
        raise RuntimeError('build_detector: %s' % e)

    def level(b, i, src):
        csrc, rsrc = _tower(b, cls_t, src), _tower(b, reg_t, src)
        return [_out(i, [('cls', head._classification), ('ctr', head._centerness)], csrc, None),
                _out(i, [('reg', head._regression)], rsrc, head._scales[i])]

    return _build_detector(backbone, neck, head, _FCOSGlue, 3, dict(cls=head._num_classes, reg=4, ctr=1), level)


class _FCOSGlue(object):
    """csrc/fcos_out.hip on both sides of FCOSHead's output convs: rows [0, C) `_classification` and row C `_centerness` of the
    classification tower's conv, rows [0, 4) `_regression` of the regression tower's; reg = expf(raw * Scale_i)"""
    reads = ('reg',)         # the node's outputs the backward reads

    @staticmethod
    def pack(plan, starts, raws, full):
        """raws[j]: the fp32 output of plan.outs[j]'s conv -> what the backward keeps: the levels' raw regression outputs"""
        raw_cls, raw_reg = raws[0::2], raws[1::2]
        ops.fcos_out_pack_levels([dict(raw_cls=raw_cls[l], raw_reg=raw_reg[l], scale=plan.outs[2 * l + 1].scale._scale.detach(),
                                       point0=starts[l]) for l in range(len(starts))], full['cls'], full['reg'], full['ctr'])
        return raw_reg

    @staticmethod
    def grad(plan, starts, raw_reg, read, dfull, dys, store, scale):
        """dfull: the gradients of the node's outputs; writes dys[j], the fp16 output gradient of plan.outs[j]'s conv, and
        accumulates the bias and Scale gradients; read: {kind: the node's output} for the kinds in `reads`"""
        head = plan.head
        levels = []
        for l, o in enumerate(plan.outs[1::2]):
            levels.append(dict(raw_reg=raw_reg[l], scale=o.scale._scale.detach(), point0=starts[l], dscale=store.target(o.scale._scale),
                               dy_cls=dys[2 * l], dy_reg=dys[2 * l + 1]))
        ops.fcos_out_grad_levels(levels, dfull['cls'].contiguous(), dfull['reg'].contiguous(), dfull['ctr'].contiguous(), read['reg'],
                                 scale, store.target(head._classification.bias), store.target(head._centerness.bias),
                                 store.target(head._regression.bias))


# ---- LFDHead (lfd/model/head/lfd_head.py:30-185), level by level: the merge path's
# units, then the classification and regression towers' units (1x1 or 3x3 conv -> GroupNorm -> ReLU through _unit_forward /
# _unit_backward; modules shared by the levels are packed once and their gradients accumulate over the levels), then the level's
# output convs as build_network forms them -- ONE 1x1 conv with the rows of both when they read the same activation, else two --
# padded to 64 or 128 rows with fp32 outputs (ops.conv2d_nhwc_f32out), and csrc/lfd_out.hip on both sides of them.  The node
# returns what LFD.forward returns in train mode: (cls [N,P,C'], reg [N,P,4]) fp32, level-concatenated; reg = raw * Scale_i (the
# loss applies `exp` where distance_to_bbox_mode asks for it).  A 3x3 head runs here although the level-concatenated schedule
# of network_forward cannot take it: every level keeps its own map.
def lfd_head_supported(backbone, neck, head):
    """backbone + neck + head as one node (DetectorTrainFunction): pyramid_supported(backbone, neck) and a training-mode LFDHead
    with one head per neck output, 64 or 128 input (= the neck's output) and head channels, 1x1 or 3x3 tower convs, any number of
    tower layers (0: the output convs read the neck's outputs), ReLU, affine GroupNorm in groups of 8 channels, every parameter
    taking a gradient, a Scale per level exactly when the regression loss is of the IoU family, shared or per-level towers, merged
    or separate, and output rows that fit the padded conv (_out_weight): num_cls_channels + 4 <= 128 where both convs read the
    same activation, num_cls_channels <= 128 with separate towers.  NOT admitted -- these keep the pyramid node with the head
    under PyTorch-ROCm autograd: LFDHeadV1, BatchNorm towers, norm_cfg=None, a frozen head parameter, other GroupNorm group
    sizes, an eval-mode head."""
    if type(head).__name__ != 'LFDHead' or not head.training:
        return False
    if not pyramid_supported(backbone, neck) or head._num_heads != neck._num_outputs:
        return False
    if head._num_input_channels != neck._num_output_channels or head._num_input_channels not in (64, 128):
        return False
    if head._num_head_channels not in (64, 128) or head._conv_kernel_size not in (1, 3) or head._num_conv_layers < 0:
        return False
    if head._num_conv_layers == 0 and head._num_head_channels != head._num_input_channels:
        return False          # (the output convs are built on num_head_channels: lfd_head.py:107-111)
    if head._activation_cfg.get('type') != 'ReLU':
        return False
    cfg = head._norm_cfg
    if cfg is None or cfg.get('type') != 'GroupNorm' or head._num_head_channels != 8 * cfg.get('num_groups', 0):
        return False
    if any(isinstance(m, nn.GroupNorm) and not m.affine for m in head.modules()):
        return False
    if not all(p.requires_grad for p in head.parameters()):
        return False
    union = head._regression_loss_type in ('IoULoss', 'GIoULoss', 'DIoULoss', 'CIoULoss')
    if hasattr(head, '_scales') != union or (union and len(head._scales) != head._num_heads):
        return False
    one_conv = head._merge_path_flag or head._num_conv_layers == 0
    return head.num_cls_channels + (4 if one_conv else 0) <= 128


def build_lfd_detector(backbone, neck, head):
    """-> _DetectorPlan of an LFDHead: per level, in LFD._forward_train's order (lfd.py:526-542), the merge path's units, the two
    towers' units and the output records exactly as build_network forms them; 1x1 output convs of 64 or 128 rows"""
    levels = netdesc.lfd_head_levels(None, head)
    return _build_detector(backbone, neck, head, _LFDGlue, 1, dict(cls=head.num_cls_channels, reg=4),
                           lambda b, i, src: _lfd_head_level(b, levels[i], i, src))


def _lfd_out_levels(plan, starts, raws, dys=None, store=None):
    """the level records of ops.lfdhead_out_pack_levels (raws: {index into plan.outs: the conv's fp32 output}) and, with dys (per
    plan.outs record) and the gradient store, of ops.lfdhead_out_grad_levels"""
    levels = [dict(point0=p0, convs=[], scale=None) for p0 in starts]
    for j, o in enumerate(plan.outs):
        lv = levels[o.level]
        cv = dict(raw=raws.get(j), segs=[dict(kind=sg['kind'], row0=sg['row0'], channels=sg['channels']) for sg in _out_segs(o)])
        if dys is not None:
            cv['dy'] = dys[j]
            for d, sg in zip(cv['segs'], _out_segs(o)):
                d['dbias'] = store.target(sg['conv'].bias)
        lv['convs'].append(cv)
        if o.scale is not None and lv['scale'] is None:
            lv['scale'] = o.scale._scale.detach()
            if dys is not None:
                lv['dscale'] = store.target(o.scale._scale)
    return levels


class _LFDGlue(object):
    """csrc/lfd_out.hip on both sides of LFDHead's output convs (one conv per level with the rows of both, or two): cls a copy of
    the classification rows, reg = raw * Scale_i (a copy without a Scale)"""
    reads = ()

    @staticmethod
    def pack(plan, starts, raws, full):
        ops.lfdhead_out_pack_levels(_lfd_out_levels(plan, starts, dict(enumerate(raws))), full['cls'], full['reg'])
        # the backward reads a raw output for the Scale gradient alone: the conv that holds a Scale'd level's regression rows
        return {j: raws[j] for j, o in enumerate(plan.outs) if o.scale is not None and any(k == 'reg' for k, _ in o.convs)}

    @staticmethod
    def grad(plan, starts, keep, read, dfull, dys, store, scale):
        ops.lfdhead_out_grad_levels(_lfd_out_levels(plan, starts, keep, dys, store), dfull['cls'].contiguous(), dfull['reg'].contiguous(),
                                    scale)


# ---- the node of both heads
def detector_forward(plan, x):
    """-> ({kind: [N,P,width] fp32} in plan.widths' order, [(h, w)] per level, saved): FCOS.forward / LFD.forward in train mode"""
    sw = switches()
    feats, (acts, tape) = pyramid_forward(plan.pyramid, x)
    dev = x.device
    zeros = _Zeros(dev)
    packs = _Packs(plan.units, False)
    htape = [_unit_forward(ui, u, acts, packs, zeros, sw) for ui, u in enumerate(plan.units)]
    sizes = [tuple(f.shape[1:3]) for f in feats]
    starts, p = _level_starts(sizes)
    opk = _out_packs(_sched(plan.head, dev), plan.outs, plan.rows)
    raws = []
    for o in plan.outs:
        wp, bp, wpk, _ = _out_pack(o, opk)
        xin = acts[o.src]
        raws.append(ops.conv2d_nhwc_f32out(xin, wpk, bp, xin.size(3), wp.size(0), plan.ks, 1))
    full = {k: torch.empty((x.size(0), p, c), dtype=torch.float32, device=dev) for k, c in plan.widths.items()}
    kept = plan.glue.pack(plan, starts, raws, full)
    return full, sizes, ((acts, tape), htape, opk, kept, starts, sizes)


def detector_backward(plan, saved, read, dfull, scale):
    """the backward of detector_forward from dfull = {kind: gradient of that output}: the output-conv glue (+ the bias / Scale
    finals), the output convs' weight gradients (partial sums, their rows routed to the parameters by ONE final launch) and data
    gradients (chains ending in the same activation take the earlier gradient as the conv kernel's residual), the head's units
    last to first, then pyramid_backward with the gradients collected at the neck's outputs.  Parameter gradients accumulate into
    `.grad` (created zeroed when missing)."""
    sw = switches()
    pp, ks = plan.pyramid, plan.ks
    (acts, tape), htape, opk, kept, starts, sizes = saved
    dev = acts[0].device
    inv = 1.0 / scale
    store = _GradStore(in_place=True)
    sc = _sched(plan.head, dev)
    sc.finals.reset()
    zeros = _Zeros(dev)
    packs = _Packs(plan.units, True)
    dead = dead_activations(pp.units)
    dys = [torch.empty((acts[0].size(0),) + sizes[o.level] + (plan.rows,), dtype=torch.float16, device=dev) for o in plan.outs]
    plan.glue.grad(plan, starts, kept, read, dfull, dys, store, scale)
    grads = {}
    for j, o in enumerate(plan.outs):
        wp = _out_pack(o, opk)
        xin, dy = acts[o.src], dys[j]
        _wgrad_partials(sc, ('wg', j), xin, dy, ks, 1, inv, _out_targets(o, store))
        c = xin.size(3)
        grads[o.src] = ops.conv2d_nhwc(dy, wp[3], zeros(c), wp[0].size(0), c, ks, 1, False, residual=grads.get(o.src))
    sc.finals.launch()
    _units_backward(plan.units, reversed(range(len(plan.units))), (acts, htape), grads, dead, store, packs, zeros, inv, sw)
    pyramid_backward(pp, (acts, tape), {o: grads[o] for o in pp.out_ids if o in grads}, scale=scale, store=store)


class DetectorTrainFunction(torch.autograd.Function):
    """FCOS.forward(x) = (cls [N,P,C], reg [N,P,4], ctr [N,P,1]) or, with an LFDHead, LFD.forward(x) = (cls [N,P,C'], reg [N,P,4])
    in train mode as ONE autograd node: backbone, pyramid neck and head forward and backward on the hand-written kernels
    (detector_forward / detector_backward).  sizes_out: the caller's list, which receives [(h, w)] per level."""

    @staticmethod
    def forward(ctx, plan, x, sizes_out, *params):
        full, sizes, saved = detector_forward(plan, x)
        ctx.plan, ctx.saved = plan, saved
        ctx.shapes = [t.shape for t in full.values()]
        ctx.save_for_backward(*(full[k] for k in plan.glue.reads))
        sizes_out.extend(sizes)
        return tuple(full.values())

    @staticmethod
    def backward(ctx, *douts):
        plan = ctx.plan
        dev = ctx.saved[0][0][0].device
        dfull = {k: torch.zeros(s, dtype=torch.float32, device=dev) if g is None else g
                 for k, s, g in zip(plan.widths, ctx.shapes, douts)}
        read = {k: t.detach() for k, t in zip(plan.glue.reads, ctx.saved_tensors)}
        detector_backward(plan, ctx.saved, read, dfull, loss_scale())
        ctx.saved = None
        return (None,) * (3 + len(plan.params))     # gradients were accumulated into .grad directly


def detector_train_forward(backbone, neck, head, x):
    """-> (cls, reg, ctr, [(h, w)] per level) for an FCOSHead, (cls, reg, [(h, w)] per level) for an LFDHead"""
    check_train_input(backbone, x)
    plan = head.__dict__.get('_lfd_detector_plan')
    if plan is None or plan.pyramid is not neck.__dict__.get('_lfd_pyramid_plan') or plan.pyramid.owner is not backbone:
        plan = (build_detector if type(head).__name__ == 'FCOSHead' else build_lfd_detector)(backbone, neck, head)
        head.__dict__['_lfd_detector_plan'] = plan
    sizes = []
    return DetectorTrainFunction.apply(plan, x, sizes, *plan.params) + (sizes,)


lfd_detector_train_forward = detector_train_forward
