"""Inference engine: turns an `LFD` (or a bare `LFDResNet`) module tree into a plan of gfx950
kernel launches behind the C ABI and runs it on the current HIP stream.

Host-side responsibilities only (tensor plumbing, no arithmetic on activations):
  * fold eval-mode BatchNorm into conv weights / bias (fp32, once per parameter version);
  * re-pack OIHW fp32 weights into MFMA fragment order, fp16 (ops.pack_conv_weight);
  * allocate NHWC fp16 activation buffers per input shape and keep them resident;
  * order the launches: stem pair -> [stem pair 2] -> residual blocks -> per-level neck+head
    (3 GroupNorm-recompute passes), outputs written directly as [N, P, C'] / [N, P, 4] fp32;
  * optionally capture the whole forward in a HIP graph (torch.cuda.CUDAGraph as the graph
    plumbing) so a forward is one replay (~55 launches -> one submission).

Unsupported module configurations raise RuntimeError: there is no PyTorch fallback for
inference (the reference's own cuDNN path is what this replaces).
"""
import ctypes as C
import os

import torch
import torch.nn as nn

from . import _lib, netdesc, ops
from ._lib import check, lib, ptr, stream_ptr

IN_NCHW_F32, IN_NHWC_F16, IN_NHWC_U8 = 0, 1, 2


MAX_FINAL_ROWS = 128     # final conv rows of one tower (4 regression rows + class channels when merged): lfd_head_forward_wide_f16


class Unsupported(RuntimeError):
    """a module configuration the fused plan does not cover (a RuntimeError, so callers that expect the reference's error
    type keep working); anything else -- HIP out of memory, a library load failure -- is NOT this type"""


def _unsupported(msg):
    raise Unsupported('lfd_amd engine: unsupported configuration: %s (no PyTorch fallback for inference)' % msg)


# ---------------------------------------------------------------------------- weight preparation
def pad_channels(c):
    """The MFMA kernels are instantiated for 32 / 64 / 128 channels.  Any other width (TL_LFD_S: a 48-channel stem and first
    stage, TrafficLight_train/TL_LFD_S.py) runs zero-padded to the next one: padded output channels have zero weights and a
    zero bias, so they stay exactly 0 through ReLU / residual adds and meet zero weights in every consumer -- the real
    channels are bit-identical to an unpadded evaluation.  3 and 1 (an RGB / a grayscale image) are left alone.
    256 and 512 (the last stages of LFDResNet's own 'fast' / 'faster' body presets, lfd_resnet.py:222-231) are the widths of
    csrc/conv_wide.hip, in the 'fp16' mode only (require_narrow guards the fp32_storage plans): backbone convs, and at 256 the
    necks and heads of the sibling engine (engine_sibling.MAX_WIDTH; csrc/conv256.hip on their large maps).  The fused LFD plan's
    necks and heads stay at 128."""
    if c in (1, 3):
        return c
    for a in (32, 64, 128, 256, 512):
        if c <= a:
            return a
    _unsupported('more than 512 channels')


def wide_conv(cin, cout, ks, stride):
    """the (padded) layers conv_dispatch sends to csrc/conv_wide.hip -- everything above 128 channels and the four <= 128 layers
    of FastBlock / FastestBlock bodies without an instance of conv_impl.h -- which has neither the chained-1x1 nor the
    downsample-pair form: the plan launches those layers one by one"""
    return cin > 128 or cout > 128 or (cin, cout, ks, stride) in ((64, 32, 3, 2), (64, 32, 1, 2), (32, 64, 3, 1), (32, 32, 1, 2))


# (cin, cout) of the 3x3 stride-2 convs that carry their block's 1x1 stride-2 identity branch in the same launch
# (lfd_conv2d_downsample_nhwc_f16): the pairs every shipped configuration has.  Other first blocks -- the wide ones, 64 -> 32 and
# 32 -> 32 of a 'fastest' body -- launch the branch on its own.
_DS_PAIRS = ((64, 64), (64, 128), (128, 128), (32, 64))


def require_narrow(backbone, what):
    """the plans without kernels above 128 channels (precision='fp32_storage') say so instead of running untested widths"""
    for m in backbone.modules():
        if isinstance(m, nn.Conv2d) and max(m.in_channels, m.out_channels) > 128:
            _unsupported("more than 128 channels (conv %d -> %d) in %s: the 256 / 512-channel layers run in the 'fp16' mode only"
                         % (m.in_channels, m.out_channels, what))


def _pad_wb(w, b):
    co, ci = pad_channels(w.shape[0]), pad_channels(w.shape[1])
    if (co, ci) == tuple(w.shape[:2]):
        return w, b
    wp = torch.zeros((co, ci) + tuple(w.shape[2:]), dtype=w.dtype, device=w.device)
    wp[:w.shape[0], :w.shape[1]] = w
    bp = torch.zeros(co, dtype=b.dtype, device=b.device)
    bp[:b.shape[0]] = b
    return wp, bp


def _padded(layer):
    """(input, output) channels of a netdesc.Layer as the kernels see them"""
    return pad_channels(layer.conv.in_channels), pad_channels(layer.conv.out_channels)


def fold_conv_norm(conv, norm):
    """(conv, eval-mode BatchNorm2d | None) -> (weight fp32 OIHW, bias fp32), channels zero-padded (pad_channels)."""
    return _pad_wb(*_fold_conv_norm(conv, norm))


def _fold_conv_norm(conv, norm):
    w = conv.weight.detach().float()
    b = conv.bias.detach().float() if conv.bias is not None else torch.zeros(w.shape[0], device=w.device)
    if norm is None:
        return w, b
    if not isinstance(norm, nn.BatchNorm2d):
        _unsupported('only BatchNorm2d can be folded into a backbone/neck conv (got %s)' % type(norm).__name__)
    inv = (norm.running_var.detach().double() + norm.eps).rsqrt()
    g = norm.weight.detach().double() if norm.weight is not None else torch.ones_like(inv)
    beta = norm.bias.detach().double() if norm.bias is not None else torch.zeros_like(inv)
    s = g * inv
    w = (w.double() * s.view(-1, 1, 1, 1)).float()
    b = ((b.double() - norm.running_mean.detach().double()) * s + beta).float()
    return w, b


def _perm_head_weight(packed):
    """ops.pack_conv_weight layout [4][8][64 = (h, m)][8 = (jh, jl)] of a 128 -> 128 1x1 conv -> the K order k_head2 consumes the
    previous stage's accumulator registers in: element e = (eh, el) of lane (hk, m) = standard lane (eh, m), element 4 hk + el
    (csrc/head.hip `perm`)."""
    p = packed.view(4, 8, 2, 32, 2, 4).permute(0, 1, 4, 3, 2, 5).contiguous()
    return p.view(4, 8, 64, 8)


def pack_stem_weight(w):
    """[C,3,3,3] -> [C/32][2][64][8] fp16 in the k-slot order of csrc/stem.hip:
    step0: half0 = row0 e0..7, half1 = row1 e0..7; step1: half0 = row2 e0..7,
    half1 = (row0 e8, row1 e8, row2 e8, 0 x5);  e = 3*s + c."""
    c = w.shape[0]
    assert w.shape[1:] == (3, 3, 3) and c % 32 == 0
    wr = w.detach().float().permute(0, 2, 3, 1).reshape(c, 3, 9)      # [co][r][e = 3*s + c]
    out = torch.zeros(c // 32, 2, 2, 32, 8, dtype=torch.float32, device=w.device)  # [tile][step][half][co_l][j]
    wt = wr.reshape(c // 32, 32, 3, 9)
    out[:, 0, 0, :, :] = wt[:, :, 0, :8]
    out[:, 0, 1, :, :] = wt[:, :, 1, :8]
    out[:, 1, 0, :, :] = wt[:, :, 2, :8]
    out[:, 1, 1, :, 0] = wt[:, :, 0, 8]
    out[:, 1, 1, :, 1] = wt[:, :, 1, 8]
    out[:, 1, 1, :, 2] = wt[:, :, 2, 8]
    return out.reshape(c // 32, 2, 64, 8).half().contiguous()


def pack_stem_gray_weight(w):
    """[C,1,3,3] -> [C/32][64][8] fp16 in the k-slot order of csrc/stem_gray.hip (one k-step): lane (h, co) slot j holds tap
    k = 8 h + j, k = 3 ky + kx; slots k >= 9 are zero."""
    c = w.shape[0]
    assert tuple(w.shape[1:]) == (1, 3, 3) and c % 32 == 0
    out = torch.zeros(c // 32, 32, 16, dtype=torch.float32, device=w.device)     # [tile][co_l][k]
    out[:, :, :9] = w.detach().float().reshape(c // 32, 32, 9)
    return out.reshape(c // 32, 32, 2, 8).permute(0, 2, 1, 3).reshape(c // 32, 64, 8).half().contiguous()


def _pad_rows(w, b, rows):
    """pad a [cout, cin, 1, 1] conv (and bias) with zero rows up to `rows`."""
    cout = w.shape[0]
    if cout == rows:
        return w, b
    wp = torch.zeros((rows,) + tuple(w.shape[1:]), dtype=w.dtype, device=w.device)
    bp = torch.zeros(rows, dtype=b.dtype, device=b.device)
    wp[:cout] = w
    bp[:cout] = b
    return wp, bp


def _tail_supported(cin, cout, ks, stride):
    """chained-1x1 instantiations compiled in csrc/conv.hip"""
    return ks == 3 and stride == 2 and cin == cout and cin in (32, 64)


def _use_fused_down(n, h, w):
    """LFD_FUSED_DOWN: '0' never, '1' always, unset: on maps of at least 50,000 input pixels per launch, single images only from
    4K frames on (a 1080p frame alone gives a workgroup five output rows: the whole forward measured 2 us slower) -- per shape
    (tools/timing/down_time.py): 8 x 270 x 480: 57.6 vs 76 us for the two launches, 8 x 135 x 240: 20.0 vs 27.4, 8 x 68 x 120: 12.5
    vs 14.3, 1 x 270 x 480: 14.9 vs 15.9; at 1 x 135 x 240 the workgroups' prologue (three filters, five input rows) is most of
    the launch: 11.5 vs 11.1"""
    e = os.environ.get('LFD_FUSED_DOWN', '')
    if e == '0':
        return False
    if e == '1':
        return True
    return n * h * w >= 50000 and (n >= 2 or h * w >= 400000)


def _use_fused_block128(n, h, w):
    """LFD_FUSED_BLOCK128: '0' never; otherwise wherever the block's two launches would run the split-K kernel (n * h * w <=
    16384 pixels: the fused launch is bit-identical to that pair).  Per shape (tools/timing/block128_in_graph.py, one block in
    a graphed chain): 1 x 17 x 30: 9.4 vs 10.8 us, 8 x 17 x 30: 10.4 vs 13.5, 8 x 12 x 20: 9.8 vs 10.5, 1 x 34 x 60: 9.7 vs 11.1,
    16 x 23 x 40: 22.7 vs 31.1"""
    if os.environ.get('LFD_FUSED_BLOCK128', '') == '0':
        return False
    return n * h * w <= 16384


class _Conv(object):
    """one lfd_conv2d_nhwc_f16 launch"""
    __slots__ = ('cin', 'cout', 'ks', 'stride', 'relu', 'w', 'b', 'tail', 'src', 'dst', 'res', 'ds', 'ref_w', 'blk', 'down', 'blk128')


class _HeadLevel(object):
    __slots__ = ('cin', 'src', 'wn', 'bn', 'towers', 'hw', 'p_off')


class _Tower(object):
    __slots__ = ('w1', 'w2', 'wf', 'bf', 'norm1', 'norm2', 'reg_rows', 'cls_rows', 'scale', 'static_ab', 'w1p', 'w2p')


# ---------------------------------------------------------------------------- plan
class EnginePlan(object):
    """Compiled launch plan for one (module tree, parameter version)."""

    def __init__(self, backbone, neck=None, head=None, device=None):
        self.device = device
        self.backbone = backbone
        self.neck = neck
        self.head = head
        self.param_sig = _param_signature(backbone, neck, head)
        self._shape_cache = {}
        self._build_backbone()
        if head is not None:
            self._build_head()

    # ---- backbone
    def _build_backbone(self):
        bb = self.backbone
        dev = self.device
        if bb._input_channels not in (1, 3):
            _unsupported('input_channels not in (1, 3)')
        self.input_channels = bb._input_channels
        if bb._norm_cfg is not None and bb._norm_cfg['type'] != 'BatchNorm2d':
            _unsupported('backbone norm must be BatchNorm2d (or None)')
        net = netdesc.backbone_layers(bb)
        if not net.stem[0].relu:
            _unsupported('activation must be ReLU')
        stem_convs = [(l.ks, l.stride) + _padded(l) + fold_conv_norm(l.conv, l.norm) for l in net.stem]
        self.fuse_blocks = os.environ.get('LFD_FUSED_BLOCK', '1') == '1'
        self.stem_first = None   # (C, w1, b1, w2|None, b2|None)
        self.stem_ref = [(k, s, w, b) for (k, s, _ci, _co, w, b) in stem_convs]   # folded fp32 stem convs, in order
        self.convs = []          # list of _Conv over symbolic buffer ids
        nbuf = [0]

        def new_buf():
            nbuf[0] += 1
            return nbuf[0] - 1

        k, s, cin, c0, w, b = stem_convs[0]
        if c0 not in (32, 64):
            _unsupported('first stem conv must have 32 or 64 output channels')
        # the first unit: csrc/stem.hip on RGB frames, csrc/stem_gray.hip on one-channel frames
        w1 = (pack_stem_gray_weight(w) if self.input_channels == 1 else pack_stem_weight(w)).to(dev)
        idx = 1
        if len(stem_convs) > 1 and stem_convs[1][0] == 1:   # 'fast' / 'faster': chained 1x1
            _, _, _, c1, w2, b2 = stem_convs[1]
            if c1 != c0:
                _unsupported('stem 1x1 must keep the channel count')
            self.stem_first = (c0, w1, b.to(dev), ops.pack_conv_weight(w2).to(dev), b2.to(dev))
            idx = 2
        else:
            self.stem_first = (c0, w1, b.to(dev), None, None)
        cur = new_buf()
        self.stem_out = cur
        self.buf_channels = {cur: c0}
        self.buf_scale = {cur: 2}      # spatial stride of each buffer w.r.t. the input
        while idx < len(stem_convs):
            k, s, cin, cout, w, b = stem_convs[idx]
            tail = None
            if (idx + 1 < len(stem_convs) and stem_convs[idx + 1][0] == 1 and stem_convs[idx + 1][3] == cout and
                    _tail_supported(cin, cout, k, s)):
                _, _, _, _, w2, b2 = stem_convs[idx + 1]
                tail = (ops.pack_conv_weight(w2).to(dev), b2.to(dev), True, w2)
                idx += 1
            cur = self._add_conv(cur, new_buf, cin, cout, k, s, True, w, b, tail=tail)
            idx += 1
        # ---- whole 'faster' stem in one kernel when it has the fusable shape
        self.stem_fused = None
        self.stem_second = None
        # (RGB only: the one-launch stem gathers 3-channel frames; a gray 'faster' stem runs its second pair on lfd_conv2d)
        if (self.input_channels == 3 and bb._stem_mode == 'faster' and c0 in (32, 64) and self.stem_first[3] is not None and len(self.convs) == 1
                and self.convs[0].tail is not None and self.convs[0].cin == c0 and self.convs[0].cout == c0
                and os.environ.get('LFD_FUSED_STEM', '1') == '1'):
            # one kernel for the whole stem (csrc/stem_fused.hip, k_stem2x): the 540x960x64 intermediate never
            # reaches HBM.  Used for NHWC fp16 frames with 64 stem channels; other inputs run the two-kernel stem
            # (stem_second keeps its conv descriptor, its intermediate buffer is allocated on first use).
            cv = self.convs.pop(0)
            self.stem_second = cv
            self.stem_fused = (c0,) + tuple(self.stem_first[1:]) + (cv.w, cv.b, cv.tail[0], cv.tail[1], cv.dst)
        # ---- stages
        self._build_stages(net.blocks, cur, new_buf)
        self.num_bufs = nbuf[0]

    def _build_stages(self, blocks, cur, new_buf):
        """the residual stages (netdesc.Block records) behind buffer `cur`: fused 64-channel block, downsample pair, 128-channel
        block, wide layers one by one; fills taps / tap_channels / tap_ready_after (engine_resnet.ResNetPlan lowers its
        stages through here too)"""
        dev = self.device
        self.taps = []
        self.tap_channels = []
        self.tap_ready_after = []
        for blk in blocks:
            x_in = cur
            ident = x_in
            fuse_ds = None
            nconv = len(blk.convs)
            if blk.downsample is not None:
                dconv, c1 = blk.downsample.conv, blk.convs[0]
                w, b = fold_conv_norm(dconv, blk.downsample.norm)
                if (c1.ks == 3 and c1.stride == 2 and c1.conv.out_channels == dconv.out_channels and
                        c1.conv.in_channels == dconv.in_channels and nconv == 2 and _padded(c1) in _DS_PAIRS):
                    # identity branch rides on the block's 3x3 stride-2 conv (one launch, one input read)
                    ident = new_buf()
                    self.buf_channels[ident] = pad_channels(dconv.out_channels)
                    self.buf_scale[ident] = self.buf_scale[x_in] * 2
                    fuse_ds = (ops.pack_conv_weight(w).to(dev), b.to(dev).contiguous(), ident, w)
                else:
                    ident = self._add_conv(x_in, new_buf, *_padded(blk.downsample), 1, 2, False, w, b)
            y = x_in
            ci = 0
            if (self.fuse_blocks and blk.downsample is None and nconv == 2 and
                    all(l.ks == 3 and l.stride == 1 and _padded(l) == (64, 64) for l in blk.convs)):
                # whole residual block in one launch (csrc/block.hip): the intermediate map never reaches HBM
                (w1, b1), (w2, b2) = [fold_conv_norm(l.conv, l.norm) for l in blk.convs]
                y = self._add_conv(x_in, new_buf, 64, 64, 3, 1, True, w1, b1, res=x_in)
                self.convs[-1].blk = (ops.pack_conv_weight(w2).to(dev), b2.to(dev).contiguous(), w2)
                ci = nconv
            while ci < nconv:
                l = blk.convs[ci]
                w, b = fold_conv_norm(l.conv, l.norm)
                last = ci == nconv - 1
                tail = None
                if ci + 2 < nconv:
                    nxt = blk.convs[ci + 1]
                    if nxt.ks == 1 and nxt.conv.out_channels == l.conv.out_channels and _tail_supported(*_padded(l), l.ks, l.stride):
                        w2, b2 = fold_conv_norm(nxt.conv, nxt.norm)
                        tail = (ops.pack_conv_weight(w2).to(dev), b2.to(dev), True, w2)   # FastBlock 3x3 -> 1x1
                y = self._add_conv(y, new_buf, *_padded(l), l.ks, l.stride, True, w, b, tail=tail, res=ident if last else None,
                                   ds=fuse_ds if ci == 0 else None)
                if (fuse_ds is not None and ci == 1 and last and tail is None and l.ks == 3 and l.stride == 1
                        and len(self.convs) >= 2 and self.convs[-2].ds is fuse_ds and self.convs[-2].cin == 64
                        and self.convs[-2].cout == 64 and self.convs[-1].cin == 64 and self.convs[-1].cout == 64):
                    # the whole downsample block can run as ONE launch (csrc/down.hip): conv 1 + branch + this conv.  Both
                    # launches stay in the plan; run_backbone picks per shape (the fused kernel wins on the larger maps)
                    self.convs[-2].down = len(self.convs) - 1
                ci += 2 if tail is not None else 1
            if (blk.downsample is None and nconv == 2 and len(self.convs) >= 2 and
                    all(c_.cin == 128 and c_.cout == 128 and c_.ks == 3 and c_.stride == 1 and c_.tail is None and c_.ds is None
                        and c_.relu for c_ in self.convs[-2:])
                    and self.convs[-2].src == x_in and self.convs[-2].res is None and self.convs[-1].src == self.convs[-2].dst
                    and self.convs[-1].res == x_in and self.convs[-1].dst == y):
                # a 128-channel block without branch: ONE launch on small maps (csrc/block128.hip); both launches stay in
                # the plan, run_backbone picks per shape
                self.convs[-2].blk128 = len(self.convs) - 1
            cur = y
            if blk.tap:
                self.taps.append(cur)
                self.tap_channels.append(blk.convs[-1].conv.out_channels)
                self.tap_ready_after.append(len(self.convs))   # number of conv launches that must precede

    def _add_conv(self, src, new_buf, cin, cout, ks, stride, relu, w, b, tail=None, res=None, ds=None):
        c = _Conv()
        c.cin, c.cout, c.ks, c.stride, c.relu = cin, cout, ks, stride, relu
        c.w = ops.pack_conv_weight(w).to(self.device)
        c.blk = None         # (w2 packed, b2, w2 folded fp32): this launch is a whole fused FasterBlock (conv, conv2, + src)
        c.ref_w = w          # folded fp32 OIHW weight (tests re-derive every layer from the tensors the engine stored)
        c.b = b.to(self.device).contiguous()
        c.tail = tail
        c.ds = ds
        c.down = None        # index of the conv that closes this (downsample) block when the pair can run fused
        c.blk128 = None      # index of the conv that closes this 128-channel block without branch when the pair can run fused
        c.src = src
        c.dst = new_buf()
        c.res = res
        self.buf_channels[c.dst] = cout
        self.buf_scale[c.dst] = self.buf_scale[src] * stride
        self.convs.append(c)
        return c.dst

    # ---- neck + head
    def _build_head(self):
        neck, head, dev = self.neck, self.head, self.device
        if neck._num_neck_channels != 128 or head._num_head_channels != 128 or head._num_input_channels != 128:
            _unsupported('neck / head channels must be 128')
        if head._num_conv_layers != 2 or head._conv_kernel_size != 1:
            _unsupported('head towers must be 2 x conv1x1')
        if neck._norm_cfg is not None and neck._norm_cfg['type'] != 'BatchNorm2d':
            _unsupported('neck norm must be BatchNorm2d')
        ncfg = head._norm_cfg
        self.head_groups = 16
        if ncfg is not None and ncfg['type'] == 'GroupNorm':
            self.head_groups = int(ncfg['num_groups'])
            g = 128 // self.head_groups
            if g * self.head_groups != 128 or (g & (g - 1)) or g > 32:
                _unsupported('GroupNorm group size must be a power of two <= 32')
        self.head_gn = ncfg is not None and ncfg['type'] == 'GroupNorm'
        cc = head.num_cls_channels
        self.cls_channels = cc
        self.levels = []
        for i, d in enumerate(netdesc.lfd_head_levels(neck, head)):
            lv = _HeadLevel()
            wn, bn = fold_conv_norm(d.neck.conv, d.neck.norm)
            lv.cin = pad_channels(d.neck.conv.in_channels)
            if lv.cin not in (64, 128):
                _unsupported('backbone tap channels must be 64 or 128')
            lv.wn = ops.pack_conv_weight(wn).to(dev)
            lv.bn = bn.to(dev)
            lv.src = self.taps[i]
            scale = d.scale._scale if d.scale is not None else None
            towers = []

            def make_tower(layers, final_w, final_b, reg_rows, cls_rows, scale_p):
                t = _Tower()
                c1, c2 = layers[0].conv, layers[1].conv
                t.w1 = ops.pack_conv_weight(c1.weight.detach().float()).to(dev)
                t.w2 = ops.pack_conv_weight(c2.weight.detach().float()).to(dev)
                t.w1p = t.w2p = None
                t.norm1, t.norm2 = layers[0].norm, layers[1].norm
                t.static_ab = None
                if not self.head_gn:   # BatchNorm / no norm: per-channel affine known ahead of time
                    t.static_ab = [self._static_affine(c1, t.norm1), self._static_affine(c2, t.norm2)]
                rows = ((reg_rows + cls_rows + 31) // 32) * 32
                fw, fb = _pad_rows(final_w, final_b, rows)
                t.wf = ops.pack_conv_weight(fw).to(dev)
                t.bf = fb.to(dev).contiguous()
                t.reg_rows, t.cls_rows, t.scale = reg_rows, cls_rows, scale_p
                return t

            cconv, rconv = d.cls_out, d.reg_out
            if head._merge_path_flag:
                # final rows = [reg x4][cls xC']: the 4 reg rows land in one lane -> one float4 store
                fw = torch.cat([rconv.weight.detach().float(), cconv.weight.detach().float()], 0)
                fb = torch.cat([rconv.bias.detach().float(), cconv.bias.detach().float()], 0)
                if cc + 4 > MAX_FINAL_ROWS:
                    _unsupported('num classes + 4 > %d with a merged head (%d class channels)' % (MAX_FINAL_ROWS, cc))
                self._check_wide_rows(cc + 4)
                towers.append(make_tower(d.merge, fw, fb, 4, cc, scale))
            else:
                if cc > MAX_FINAL_ROWS:
                    _unsupported('more than %d classification channels (%d)' % (MAX_FINAL_ROWS, cc))
                self._check_wide_rows(cc)
                towers.append(make_tower(d.cls, cconv.weight.detach().float(), cconv.bias.detach().float(), 0, cc, None))
                towers.append(make_tower(d.reg, rconv.weight.detach().float(), rconv.bias.detach().float(), 4, 0, scale))
            lv.towers = towers
            self.levels.append(lv)

    def _check_wide_rows(self, rows):
        """more than 64 final rows run in lfd_head_forward_wide_f16, which only the wave-per-32-pixels kernel serves"""
        if rows > 64 and 128 // self.head_groups < 8:
            _unsupported('a head with more than 64 output rows (%d) needs GroupNorm groups of at least 8 channels, not %d '
                         '(GroupNorm(%d, 128))' % (rows, 128 // self.head_groups, self.head_groups))

    @staticmethod
    def _static_affine(conv, norm):
        """(scale, shift)[128] applied after a tower conv when the norm is BatchNorm2d or absent."""
        c = conv.out_channels
        dev = conv.weight.device
        bias = conv.bias.detach().double() if conv.bias is not None else torch.zeros(c, dtype=torch.double, device=dev)
        if norm is None:
            return torch.ones(c, dtype=torch.double, device=dev), bias
        inv = (norm.running_var.detach().double() + norm.eps).rsqrt()
        s = norm.weight.detach().double() * inv
        return s, (bias - norm.running_mean.detach().double()) * s + norm.bias.detach().double()

    # ---- shape-dependent state
    def state_for(self, n, h, w, slot=0):
        """`slot`: independent sets of activation / output buffers for the same shape, so that several batches can be in
        flight at once (one per HIP stream; bench.py keeps two)."""
        key = (n, h, w, slot)
        st = self._shape_cache.get(key)
        if st is None:
            st = _ShapeState(self, n, h, w)
            self._shape_cache[key] = st
        return st

    # ---- execution
    def run_backbone(self, x, fmt, st, after=None):
        """`after`: optional {number_of_convs_done: callable} hooks (used to fork the level-0 head)."""
        l = lib()
        sp = stream_ptr()
        if self.stem_fused is not None and not (fmt in (1, 2) and self.stem_fused[0] == 64):
            # two-kernel stem for the formats / widths k_stem2x does not cover (NCHW fp32 frames, 32-channel stems)
            c0, w1, b1, w2, b2 = self.stem_first
            mid = st.stem_mid(self)
            check(l.lfd_stem_conv_f16(ptr(x), fmt, st.n, st.h, st.w, c0, ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(mid), sp),
                  'lfd_stem_conv_f16')
            c = self.stem_second
            d = _lib.ConvDesc(st.n, mid.shape[1], mid.shape[2], c.cin, c.cout, c.ks, c.stride, int(c.relu), c.cout, 1)
            check(l.lfd_conv2d_nhwc_f16(C.byref(d), ptr(mid), ptr(st.bufs[c.dst]), ptr(c.w), ptr(c.b), None,
                                        ptr(c.tail[0]), ptr(c.tail[1]), ptr(ops.zero_line(self.device)), sp),
                  'lfd_conv2d_nhwc_f16')
        elif self.stem_fused is not None:
            c0, w1, b1, w2, b2, w3, b3, w4, b4, dst = self.stem_fused
            check(l.lfd_stem_faster_fused_f16(ptr(x), fmt, st.n, st.h, st.w, c0, ptr(w1), ptr(b1), ptr(w2), ptr(b2),
                                              ptr(w3), ptr(b3), ptr(w4), ptr(b4), ptr(st.bufs[dst]), sp),
                  'lfd_stem_faster_fused_f16')
        elif self.input_channels == 1:
            c0, w1, b1, w2, b2 = self.stem_first
            check(l.lfd_stem_gray_f16(ptr(x), fmt, st.n, st.h, st.w, c0, ptr(w1), ptr(b1), ptr(w2), ptr(b2),
                                      ptr(st.bufs[self.stem_out]), sp), 'lfd_stem_gray_f16')
        else:
            c0, w1, b1, w2, b2 = self.stem_first
            check(l.lfd_stem_conv_f16(ptr(x), fmt, st.n, st.h, st.w, c0, ptr(w1), ptr(b1), ptr(w2), ptr(b2),
                                      ptr(st.bufs[self.stem_out]), sp), 'lfd_stem_conv_f16')
        self._run_convs(st, after)

    def _run_convs(self, st, after=None):
        """the launches of self.convs in order, each in the form its shape selects (engine_resnet.ResNetPlan runs its stages
        through here too)"""
        l = lib()
        sp = stream_ptr()
        z = ops.zero_line(self.device)
        skip = -1
        for ci, c in enumerate(self.convs):
            if after and ci in after:
                after[ci]()
            if ci == skip:
                continue
            src = st.bufs[c.src]
            if c.down is not None and _use_fused_down(st.n, src.shape[1], src.shape[2]):
                c2 = self.convs[c.down]
                check(l.lfd_downblock_fused_f16(st.n, src.shape[1], src.shape[2], ptr(src), ptr(st.bufs[c2.dst]), ptr(c.w), ptr(c.b),
                                                ptr(c.ds[0]), ptr(c.ds[1]), ptr(c2.w), ptr(c2.b), ptr(z), sp), 'lfd_downblock_fused_f16')
                skip = c.down
                continue
            if c.blk is not None:
                check(l.lfd_fasterblock_fused_f16(st.n, src.shape[1], src.shape[2], ptr(src), ptr(st.bufs[c.dst]), ptr(c.w), ptr(c.b),
                                                  ptr(c.blk[0]), ptr(c.blk[1]), ptr(z), sp), 'lfd_fasterblock_fused_f16')
                continue
            if c.blk128 is not None and _use_fused_block128(st.n, src.shape[1], src.shape[2]):
                c2 = self.convs[c.blk128]
                check(l.lfd_fasterblock128_fused_f16(st.n, src.shape[1], src.shape[2], ptr(src), ptr(st.bufs[c2.dst]), ptr(c.w), ptr(c.b),
                                                     ptr(c2.w), ptr(c2.b), sp), 'lfd_fasterblock128_fused_f16')
                skip = c.blk128
                continue
            d = _lib.ConvDesc(st.n, src.shape[1], src.shape[2], c.cin, c.cout, c.ks, c.stride, int(c.relu),
                              c.cout if c.tail else 0, 1 if c.tail else 0)
            if c.ds is not None:
                check(l.lfd_conv2d_downsample_nhwc_f16(C.byref(d), ptr(src), ptr(st.bufs[c.dst]), ptr(c.w), ptr(c.b),
                                                       ptr(c.ds[0]), ptr(c.ds[1]), ptr(st.bufs[c.ds[2]]), ptr(z), sp),
                      'lfd_conv2d_downsample_nhwc_f16')
                continue
            check(l.lfd_conv2d_nhwc_f16(C.byref(d), ptr(src), ptr(st.bufs[c.dst]), ptr(c.w), ptr(c.b),
                                        ptr(st.bufs[c.res]) if c.res is not None else None,
                                        ptr(c.tail[0]) if c.tail else None, ptr(c.tail[1]) if c.tail else None,
                                        ptr(z), sp), 'lfd_conv2d_nhwc_f16')
        if after and len(self.convs) in after:
            after[len(self.convs)]()

    def decode_supported(self, st, desc):
        """the head's output pass can threshold + decode + append by itself (lfd_head_forward_decode_f16): one merged
        tower over all levels in one launch group, one foreground class with sigmoid scores"""
        if len(st.head_groups) != 1 or len(st.head_groups[0]) != 1 or os.environ.get('LFD_HEAD_DECODE', '1') == '0':
            return False
        d = st.head_groups[0][0]['desc']
        return (desc.num_classes == 1 and desc.num_cls_channels == 1 and desc.score_mode == 0 and d.cls_channels == 1
                and d.final_reg_rows == 4 and d.final_cls_rows == 1 and self.head_gn and self.head_groups <= 16)

    def run_head(self, st, groups=None, decode=None):
        """5 launches per (level group, tower): pass 1, finalize, pass 2, finalize, pass 3.
        decode = (detect desc, meta [N,3], ops.DetectOutputs): pass 3 appends the candidates itself and the logits are
        not written (decode_supported() must hold)."""
        l = lib()
        z = ops.zero_line(self.device)
        for gi in (range(len(st.head_groups)) if groups is None else groups):
            if len(st.head_groups[gi]) == 2 and decode is None and getattr(st, 'tower_overlap', False):
                # separate classification / regression towers (TT100K_LFD_L): independent launch chains of five that read the same
                # taps and write different tensors -- the second one runs on a side stream, so that each chain's two short
                # finalize launches fall beside the other chain's passes
                main = torch.cuda.current_stream()
                st.ev_tw0.record(main)
                with torch.cuda.stream(st.side_tw):
                    st.side_tw.wait_event(st.ev_tw0)
                    self._run_tower(st, st.head_groups[gi][1], None, l, z)
                    st.ev_tw1.record(st.side_tw)
                self._run_tower(st, st.head_groups[gi][0], None, l, z)
                main.wait_event(st.ev_tw1)
                continue
            for hs in st.head_groups[gi]:
                self._run_tower(st, hs, decode, l, z)

    def _run_tower(self, st, hs, decode, l, z):
        """the five launches of one tower on torch's current stream"""
        sp = stream_ptr()
        d, lv, ab1, ab2, part = hs['desc'], hs['levels'], hs['ab1'], hs['ab2'], hs['partial']
        if self.head_gn:
            for p, ab, gam, bet, eps in ((1, ab1, hs['g1'], hs['b1'], hs['eps1']), (2, ab2, hs['g2'], hs['b2'], hs['eps2'])):
                check(l.lfd_head_forward_f16(C.byref(d), p, lv, ptr(ab1), None, ptr(part), None, None, ptr(z), sp),
                      'lfd_head_forward_f16(pass %d)' % p)
                check(l.lfd_groupnorm_finalize_fold(C.byref(d), ptr(part), gam, bet, eps, ptr(ab), lv, p, sp),
                      'lfd_groupnorm_finalize_fold')
        if decode is not None:
            ddesc, meta, out = decode
            check(l.lfd_head_forward_decode_f16(C.byref(d), lv, ptr(ab1), ptr(ab2), None, None, ptr(z), C.byref(ddesc),
                                                ptr(meta), ptr(out.ws), out.ws.numel(), sp), 'lfd_head_forward_decode_f16')
            return
        if d.final_reg_rows + d.final_cls_rows > 64:      # 3 or 4 tiles of final rows: the wide output pass
            check(l.lfd_head_forward_wide_f16(C.byref(d), lv, ptr(ab1), ptr(ab2), ptr(st.cls), ptr(st.reg), ptr(z), sp),
                  'lfd_head_forward_wide_f16')
            return
        check(l.lfd_head_forward_f16(C.byref(d), 3, lv, ptr(ab1), ptr(ab2), None, ptr(st.cls), ptr(st.reg), ptr(z), sp),
              'lfd_head_forward_f16(pass 3)')

    def run_all(self, x, fmt, st, decode=None):
        """Whole forward.  The neck+head of the FIRST pyramid level (the largest, ~75 % of the head's
        pixels) only depends on the first backbone tap: it is forked onto a side stream as soon as that
        tap is written and overlaps with the remaining (small, latency-bound) backbone stages; the other
        levels follow on the main stream; joined at the end.  Works eagerly and under graph capture."""
        if self.head is None:
            return self.run_backbone(x, fmt, st)
        if getattr(st, 'split_head', False) and len(st.head_groups) > 1:
            self.run_backbone(x, fmt, st)
            main = torch.cuda.current_stream()
            st.ev_tap.record(main)
            with torch.cuda.stream(st.side):
                st.side.wait_event(st.ev_tap)
                self.run_head(st, groups=range(1, len(st.head_groups)))
                st.ev_done.record(st.side)
            self.run_head(st, groups=[0])
            main.wait_event(st.ev_done)
            return
        if not st.overlap or len(st.head_groups) < 2:
            self.run_backbone(x, fmt, st)
            return self.run_head(st, decode=decode)
        main = torch.cuda.current_stream()

        def fork():
            st.ev_tap.record(main)
            with torch.cuda.stream(st.side):
                st.side.wait_event(st.ev_tap)
                self.run_head(st, groups=[0])
                st.ev_done.record(st.side)

        self.run_backbone(x, fmt, st, after={self.tap_ready_after[0]: fork})
        self.run_head(st, groups=range(1, len(st.head_groups)))
        main.wait_event(st.ev_done)


class _ShapeState(object):
    """Activation buffers and outputs for one input shape."""

    def stem_mid(self, plan):
        """stride-2 stem intermediate, only materialised when the two-kernel stem has to run"""
        if self._stem_mid is None:
            self._stem_mid = torch.empty((self.n, (self.h + 1) // 2, (self.w + 1) // 2, plan.buf_channels[plan.stem_out]),
                                         dtype=torch.float16, device=plan.device)
        return self._stem_mid

    def __init__(self, plan, n, h, w):
        dev = plan.device
        self.n, self.h, self.w = n, h, w
        self.bufs = {}
        with torch.cuda.device(dev):
            dims = {}
            for b, sc in plan.buf_scale.items():
                if plan.stem_fused is not None and b == plan.stem_out:
                    continue      # the stride-2 stem intermediate never exists in HBM
                hh, ww = h, w
                s = sc
                while s > 1:
                    hh, ww = (hh + 1) // 2, (ww + 1) // 2   # conv k3 p1 s2 and k1 p0 s2 agree: ceil(x/2)
                    s //= 2
                dims[b] = (hh, ww)
                self.bufs[b] = torch.empty((n, hh, ww, plan.buf_channels[b]), dtype=torch.float16, device=dev)
            self.dims = dims
            self._stem_mid = None
            if plan.head is not None:
                self.sizes = [dims[t] for t in plan.taps]
                self.p_off = []
                p = 0
                for (hh, ww) in self.sizes:
                    self.p_off.append(p)
                    p += hh * ww
                self.P = p
                self.cls = torch.empty((n, p, plan.cls_channels), dtype=torch.float32, device=dev)
                self.reg = torch.empty((n, p, 4), dtype=torch.float32, device=dev)
                import os
                ntow = len(plan.levels[0].towers)
                nlv = len(plan.levels)
                # side-stream fork of the level-0 head: measured neutral on MI355X (both kernel families are
                # persistent and fill every CU), so it is opt-in
                self.overlap = nlv > 1 and os.environ.get('LFD_OVERLAP') == '1'
                # The 64- and the 128-channel pyramid levels run in different kernels (k_head2 / k_head) whose launches
                # are independent chains (pass 1 -> finalize -> pass 2 -> finalize -> pass 3).  The 128-channel
                # levels are tiny (a few dozen workgroups, latency bound): run their chain on a side stream next to
                # the big one instead of behind it.  Measured neutral (0.737 vs 0.738 ms per step): opt-in, LFD_SPLIT_HEAD=1.
                cins = sorted({plan.levels[li].cin for li in range(nlv)})
                self.split_head = (not self.overlap and len(cins) > 1 and os.environ.get('LFD_SPLIT_HEAD', '0') == '1')
                if self.overlap:
                    level_groups = [[0], list(range(1, nlv))]
                elif self.split_head:
                    level_groups = [[li for li in range(nlv) if plan.levels[li].cin == c] for c in cins]
                else:
                    level_groups = [list(range(nlv))]
                self.head_groups = []
                for lg in level_groups:
                    calls = []
                    for ti in range(ntow):
                        t0 = plan.levels[0].towers[ti]
                        nl = len(lg)
                        d = _lib.HeadDesc()
                        d.n, d.num_levels = n, nl
                        for k, li in enumerate(lg):
                            hh, ww = self.sizes[li]
                            d.level_hw[k], d.level_cin[k], d.level_point_offset[k] = hh * ww, plan.levels[li].cin, self.p_off[li]
                        d.head_channels, d.num_groups, d.total_points = 128, plan.head_groups, p
                        d.cls_channels, d.final_reg_rows, d.final_cls_rows = plan.cls_channels, t0.reg_rows, t0.cls_rows
                        lvp = (_lib.HeadLevelPtrs * nl)()
                        for k, li in enumerate(lg):
                            lv = plan.levels[li]
                            t = lv.towers[ti]
                            lvp[k].x = self.bufs[lv.src].data_ptr()
                            lvp[k].wn_packed, lvp[k].bn = lv.wn.data_ptr(), lv.bn.data_ptr()
                            lvp[k].w1_packed, lvp[k].w2_packed = t.w1.data_ptr(), t.w2.data_ptr()
                            if os.environ.get('LFD_HEAD_PERM', '1') != '0':
                                if getattr(t, 'w1p', None) is None:       # K-permuted copies, once per plan
                                    t.w1p, t.w2p = _perm_head_weight(t.w1), _perm_head_weight(t.w2)
                                lvp[k].w1_perm, lvp[k].w2_perm = t.w1p.data_ptr(), t.w2p.data_ptr()
                            lvp[k].wf_packed, lvp[k].bf = t.wf.data_ptr(), t.bf.data_ptr()
                            lvp[k].scale = t.scale.data_ptr() if t.scale is not None else None
                        call = dict(desc=d, levels=lvp)
                        if plan.head_gn and os.environ.get('LFD_HEAD_FOLD', '1') != '0':
                            # per-(level, image) GroupNorm-folded tower filters, written by the finalize launches
                            call['folded'] = torch.empty((nl, 2, n, _lib.HEAD_FOLDED_HALFS), dtype=torch.float16, device=dev)
                            for k in range(nl):
                                lvp[k].w1_folded, lvp[k].w2_folded = call['folded'][k, 0].data_ptr(), call['folded'][k, 1].data_ptr()
                            if os.environ.get('LFD_HEAD_A1', '1') != '0':
                                # ... and conv2's operands (tower-1 activations) handed from pass 2 to the output pass
                                call['tower1'] = []
                                for k, li in enumerate(lg):
                                    hh, ww = self.sizes[li]
                                    t1 = torch.empty((n, (hh * ww + 31) // 32, _lib.HEAD_TOWER1_GROUP_HALFS), dtype=torch.float16, device=dev)
                                    call['tower1'].append(t1)
                                    lvp[k].tower1_out = t1.data_ptr()
                        if plan.head_gn:
                            call['ab1'] = torch.empty((nl, n, 128, 2), dtype=torch.float32, device=dev)
                            call['ab2'] = torch.empty((nl, n, 128, 2), dtype=torch.float32, device=dev)
                            for tag, attr in (('1', 'norm1'), ('2', 'norm2')):
                                g = (C.c_void_p * nl)(*[getattr(plan.levels[li].towers[ti], attr).weight.data_ptr() for li in lg])
                                b_ = (C.c_void_p * nl)(*[getattr(plan.levels[li].towers[ti], attr).bias.data_ptr() for li in lg])
                                call['g' + tag], call['b' + tag] = g, b_
                                call['eps' + tag] = float(getattr(t0, attr).eps)
                        else:      # BatchNorm / no norm: static per-channel affine, replicated per level / image
                            for k in (0, 1):
                                ab = torch.stack([torch.stack(plan.levels[li].towers[ti].static_ab[k], -1).float() for li in lg], 0)
                                call['ab%d' % (k + 1)] = ab[:, None].expand(nl, n, 128, 2).contiguous().to(dev)
                        call['partial'] = torch.empty(max(int(lib().lfd_head_partial_floats(C.byref(d))), 1),
                                                      dtype=torch.float32, device=dev)
                        calls.append(call)
                    self.head_groups.append(calls)
                self.tower_overlap = ntow == 2 and os.environ.get('LFD_TOWER_OVERLAP', '1') == '1'
                if self.tower_overlap:
                    self.side_tw = torch.cuda.Stream(device=dev)
                    self.ev_tw0 = torch.cuda.Event()
                    self.ev_tw1 = torch.cuda.Event()
                if self.overlap or self.split_head:
                    self.side = torch.cuda.Stream(device=dev)
                    self.ev_tap = torch.cuda.Event()
                    self.ev_done = torch.cuda.Event()
        self.graph = None
        self.graph_input = None


def _param_signature(*mods):
    sig = []
    for m in mods:
        if m is None:
            continue
        for t in list(m.parameters()) + list(m.buffers()):
            sig.append((t.data_ptr(), t._version))
    return tuple(sig)


def version_sum(model):
    """Cheap change detector for the replay fast path: (number of tensors, sum of their in-place version counters, sum of
    their storage addresses) over the parameters and buffers of an LFD.  Versions only increase, so their sum changes iff a
    tensor was written in place; the address sum catches `p.data = other` and load_state_dict(assign=True), which swap
    storage without touching a version counter or going through _apply.  The tensor LIST is cached and refreshed whenever a
    submodule or parameter object is replaced (LFD.__setattr__ / the load_state_dict post-hook drop it) and, as a backstop,
    every 16th call (replacing a NESTED parameter object -- model._backbone.stage0[0]._conv1.weight = nn.Parameter(..)
    -- goes through neither hook; the new tensor's address differs from the old one's, so the sum over the refreshed list
    changes within 16 steps; clear model._step_graphs for an immediate effect)."""
    d = model.__dict__
    ts = d.get('_lfd_tensors')
    calls = d.get('_lfd_tensors_calls', 0) + 1
    if ts is None or calls >= 16:
        ts = []
        for m in (model._backbone, model._neck, model._head):
            if m is not None:
                ts += list(m.parameters()) + list(m.buffers())
        d['_lfd_tensors'] = ts
        calls = 0
    d['_lfd_tensors_calls'] = calls
    v = a = 0
    for t in ts:
        v += t._version
        a += t.data_ptr()
    return (len(ts), v, a)


# ---------------------------------------------------------------------------- entry points
def get_plan(owner, backbone, neck, head, device):
    """Plan cache on `owner` keyed by device; rebuilt when any parameter/buffer changed
    (in-place update bumps tensor._version; .to()/.cuda() changes data_ptr)."""
    cache = owner.__dict__.setdefault('_lfd_engine_cache', {})
    key = (device.type, device.index)
    plan = cache.get(key)
    sig = _param_signature(backbone, neck, head)
    if plan is None or plan.param_sig != sig:
        with torch.no_grad():
            plan = EnginePlan(backbone, neck, head, device)
        cache[key] = plan
    return plan


def _input_format(x, channels=3):
    """(in_format, n, h, w) of an image batch for a model with `channels` input channels (the backbone's input_channels).
    RGB: NCHW float32 [N,3,H,W], NHWC float16 / uint8 [N,H,W,3]; gray: float32 [N,1,H,W], float16 / uint8 [N,H,W,1] (for one
    channel NCHW and NHWC are the same bytes: the kernels read one [N,H,W] plane)."""
    if x.dim() != 4:
        raise RuntimeError('expected a 4-D image batch')
    if channels == 1:
        if x.dtype == torch.float32 and x.shape[1] == 1:
            return IN_NCHW_F32, x.shape[0], x.shape[2], x.shape[3]
        if x.dtype == torch.float16 and x.shape[3] == 1:
            return IN_NHWC_F16, x.shape[0], x.shape[1], x.shape[2]
        if x.dtype == torch.uint8 and x.shape[3] == 1:
            return IN_NHWC_U8, x.shape[0], x.shape[1], x.shape[2]
        raise RuntimeError('unsupported input for a one-channel (input_channels=1) model: float32 [N,1,H,W], '
                           'float16 [N,H,W,1] or uint8 [N,H,W,1] (got %s %s)' % (x.dtype, tuple(x.shape)))
    if channels != 3:
        _unsupported('input_channels not in (1, 3)')
    if x.dtype == torch.float32 and x.shape[1] == 3:
        return IN_NCHW_F32, x.shape[0], x.shape[2], x.shape[3]
    if x.dtype == torch.float16 and x.shape[3] == 3:
        return IN_NHWC_F16, x.shape[0], x.shape[1], x.shape[2]
    if x.dtype == torch.uint8 and x.shape[3] == 3:
        return IN_NHWC_U8, x.shape[0], x.shape[1], x.shape[2]
    if (x.dtype == torch.float32 and x.shape[1] == 1) or (x.dtype in (torch.float16, torch.uint8) and x.shape[3] == 1):
        raise RuntimeError('unsupported input: a one-channel batch %s %s for an RGB (input_channels=3) model; expected NCHW '
                           'float32 [N,3,H,W], NHWC float16 [N,H,W,3] or NHWC uint8 [N,H,W,3]' % (x.dtype, tuple(x.shape)))
    raise RuntimeError('unsupported input: NCHW float32 [N,3,H,W], NHWC float16 [N,H,W,3] or NHWC uint8 [N,H,W,3]')


def lfd_forward(model, x, use_graph=False, slot=0):
    """Full LFD forward on the engine.  Returns (cls [N,P,C'] fp32, reg [N,P,4] fp32, sizes).
    The returned tensors are engine-owned buffers, overwritten by the next forward of the same
    input shape and slot (clone() to keep them)."""
    _lib.require_cuda(x, 'LFD.forward')
    if not x.is_contiguous():
        x = x.contiguous()
    fmt, n, h, w = _input_format(x, model._backbone._input_channels)
    plan = get_plan(model, model._backbone, model._neck, model._head, x.device)
    st = plan.state_for(n, h, w, slot)
    with torch.cuda.device(x.device):
        if use_graph:
            _run_graphed(plan, st, x, fmt)
        else:
            plan.run_all(x, fmt, st)
    return st.cls, st.reg, st.sizes


def lfd_forward_detect(model, x, desc, meta, out, slot=0):
    """Forward whose last head pass appends the detection candidates to out.ws instead of writing logits, followed by
    sort + mask + scan (ops.detect_from_candidates).  Returns False -- nothing enqueued -- when this model / descriptor
    is not covered (EnginePlan.decode_supported); the caller then runs lfd_forward + ops.detect_batched."""
    _lib.require_cuda(x, 'LFD.forward')
    if not x.is_contiguous():
        x = x.contiguous()
    fmt, n, h, w = _input_format(x, model._backbone._input_channels)
    plan = get_plan(model, model._backbone, model._neck, model._head, x.device)
    st = plan.state_for(n, h, w, slot)
    if plan.head is None or not plan.decode_supported(st, desc):
        return False
    with torch.cuda.device(x.device):
        plan.run_all(x, fmt, st, decode=(desc, meta, out))
        ops.detect_from_candidates(desc, n, out)
    return True


def _run_graphed(plan, st, x, fmt):
    """One HIP graph per (input shape, input buffer): a caller that keeps its frames in a resident
    buffer (the bench, a video pipeline's ring slot) replays without any copy; a new buffer address
    gets its own capture (at most 4 kept)."""
    graphs = st.graph if isinstance(st.graph, dict) else {}
    st.graph = graphs
    key = (x.data_ptr(), fmt)
    ent = graphs.get(key)
    if ent is None:
        if len(graphs) >= 4:
            graphs.pop(next(iter(graphs)))
        # warm-up outside capture (sets kernel attributes, sizes workspaces)
        plan.run_all(x, fmt, st)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            plan.run_all(x, fmt, st)
        ent = (g, x)            # keep the captured input alive
        graphs[key] = ent
    ent[0].replay()


def backbone_only_forward(backbone, x):
    """LFDResNet.forward stand-alone: tuple of tapped maps as NCHW fp32 (reference return type,
    lfd_resnet.py:488-501).  The layout/precision conversion is plain tensor plumbing."""
    _lib.require_cuda(x, 'LFDResNet.forward')
    fmt, n, h, w = _input_format(x.contiguous(), backbone._input_channels)
    plan = get_plan(backbone, backbone, None, None, x.device)
    st = plan.state_for(n, h, w)
    with torch.cuda.device(x.device):
        plan.run_backbone(x.contiguous(), fmt, st)
    return tuple(st.bufs[t][..., :c].permute(0, 3, 1, 2).float() for t, c in zip(plan.taps, plan.tap_channels))
