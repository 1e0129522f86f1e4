"""Backbone plan of the torchvision-style ResNet (model/backbone/resnet.py) for the fp16 inference mode.

  stem     lfd_stem7_conv_f16 (csrc/stem7.hip: conv7x7 s2 p3 + folded BatchNorm + ReLU on the frame) -> lfd_maxpool3x3s2_nhwc_f16
  stages   engine.EnginePlan._build_stages / _run_convs: BasicBlock is the FasterBlock record of netdesc.Block, so stage 1
           runs as fused 64-channel blocks (csrc/block.hip), stage 2 as the 64 -> 128 downsample pair + 128-channel blocks,
           stages 3 / 4 (256 / 512 channels) layer by layer on csrc/conv_wide.hip

ResNetPlan offers what engine_sibling.SiblingPlan asks of a backbone plan -- taps, tap_channels, input_channels, state_for,
run_backbone -- and nothing else: ResNet models run layer by layer behind it (LFD._fused_plan_ok answers False).

Covered: depth 18 / 34, in_channels=3, base_channels=64, BatchNorm, strides (1, 2, 2, 2), dilations 1, the 7x7 stem, any valid
out_indices.  Everything else the constructor accepts raises engine.Unsupported naming the option (such models still build
and train under autograd); so does precision='fp32_storage' (require_fp16_mode): the 7x7 and the wide layers have no
fp32-tensor kernel.
"""
import os

import torch

from . import engine, netdesc
from ._lib import check, lib, ptr, stream_ptr

KSTEPS = 10          # 147 taps in ten 16-wide MFMA k-steps


_CLASSES = []


def _classes():
    """(ResNet, LFDResNet), imported on first use: model/lfd.py imports this module, and the models ask on every call"""
    if not _CLASSES:
        from .model.backbone.lfd_resnet import LFDResNet
        from .model.backbone.resnet import ResNet
        _CLASSES.extend((ResNet, LFDResNet))
    return _CLASSES


def is_resnet(backbone):
    """this package's torchvision-style ResNet or a subclass -- not whatever else is called ResNet (torchvision's own has other
    attributes and gets the foreign-backbone Unsupported of engine_sibling)"""
    return isinstance(backbone, _classes()[0])


def is_lfd_resnet(backbone):
    """an LFDResNet of this package or a subclass: the backbones engine.EnginePlan and train_engine read"""
    return isinstance(backbone, _classes()[1])


def require_fp16_mode(model):
    """precision='fp32_storage' on a ResNet model"""
    if is_resnet(model._backbone):
        engine._unsupported("precision='fp32_storage' with a ResNet backbone: its 7x7 stem conv and its 256 / 512-channel layers "
                            "have no fp32-tensor kernel; ResNet models run in the 'fp16' mode only")


def pack_stem7_weight(w):
    """folded conv1 weight [64, 3, 7, 7] fp32 -> [2][10][64][8] fp16, the fragment layout of csrc/stem7.hip: element j of lane
    (hk, co % 32) in k-step s of output-channel half co // 32 holds the filter value of tap slot k = 16 s + 8 hk + j,
      s < 7:   row ky = s, e = 8 hk + j                                          (e = 3 kx + c: 21 values per filter row)
      s >= 7:  i = k - 112 < 35: ky = i // 5, e = 16 + i % 5;  i >= 35: zero     (the five left-over values of each row)"""
    assert tuple(w.shape) == (64, 3, 7, 7)
    rows = w.detach().float().permute(0, 2, 3, 1).reshape(64, 7, 21)               # [co][ky][e]
    k = torch.zeros(64, 16 * KSTEPS, dtype=torch.float32, device=w.device)
    k[:, :112] = rows[:, :, :16].reshape(64, 112)
    k[:, 112:147] = rows[:, :, 16:].reshape(64, 35)
    out = k.reshape(2, 32, KSTEPS, 2, 8).permute(0, 2, 3, 1, 4).reshape(2, KSTEPS, 64, 8)
    return out.half().contiguous()


def check_covered(bb):
    """engine.Unsupported, naming the option, for every ResNet the plan has no kernels for"""
    u = engine._unsupported
    if bb.depth not in (18, 34):
        u('ResNet depth=%d: Bottleneck blocks (1024 / 2048-channel layers) have no kernel; depth 18 and 34 run' % bb.depth)
    if bb.deep_stem:
        u('ResNet deep_stem=True: the engine covers the 7x7 stem')
    if bb.avg_down:
        u('ResNet avg_down=True')
    if bb.dcn is not None:
        u('ResNet dcn')
    if bb.norm_cfg['type'] != 'BN':
        u("ResNet norm_cfg type %r: only 'BN' can be folded into the convs" % (bb.norm_cfg['type'],))
    if bb.conv1.in_channels != 3:
        u('ResNet in_channels=%d: the 7x7 stem kernel reads RGB frames' % bb.conv1.in_channels)
    if bb.base_channels != 64:
        u('ResNet base_channels=%d: the 7x7 stem kernel writes 64 channels' % bb.base_channels)
    if tuple(bb.strides) != (1, 2, 2, 2)[:bb.num_stages]:
        u('ResNet strides=%s: the engine covers (1, 2, 2, 2)' % (tuple(bb.strides),))
    if any(d != 1 for d in bb.dilations):
        u('ResNet dilations=%s: dilated convs have no kernel' % (tuple(bb.dilations),))


class ResNetPlan(engine.EnginePlan):
    """Compiled backbone launches of one (ResNet, parameter version); neck / head belong to engine_sibling.SiblingPlan."""

    def __init__(self, backbone, device):
        super().__init__(backbone, None, None, device)

    def _build_backbone(self):
        bb, dev = self.backbone, self.device
        check_covered(bb)
        self.input_channels = 3
        net = netdesc.resnet_layers(bb)
        first = net.stem[0]
        w, b = engine._fold_conv_norm(first.conv, first.norm)
        self.stem7 = (pack_stem7_weight(w).to(dev), b.to(dev).contiguous())
        self.stem_ref = [(7, 2, w, b)]
        self.fuse_blocks = os.environ.get('LFD_FUSED_BLOCK', '1') == '1'
        self.stem_first = self.stem_fused = self.stem_second = None
        self.convs = []
        nbuf = [2]

        def new_buf():
            nbuf[0] += 1
            return nbuf[0] - 1

        self.stem_out, self.pool_out = 0, 1
        self.buf_channels = {0: 64, 1: 64}
        self.buf_scale = {0: 2, 1: 4}        # conv k7 p3 s2 and pool k3 p1 s2: ceil(x / 2) each, like every stride-2 layer
        self._build_stages(net.blocks, self.pool_out, new_buf)
        self.num_bufs = nbuf[0]

    def run_backbone(self, x, fmt, st, after=None):
        l, sp = lib(), stream_ptr()
        y, p = st.bufs[self.stem_out], st.bufs[self.pool_out]
        check(l.lfd_stem7_conv_f16(ptr(x), fmt, st.n, st.h, st.w, ptr(self.stem7[0]), ptr(self.stem7[1]), ptr(y), sp),
              'lfd_stem7_conv_f16')
        check(l.lfd_maxpool3x3s2_nhwc_f16(ptr(y), ptr(p), st.n, y.shape[1], y.shape[2], 64, sp), 'lfd_maxpool3x3s2_nhwc_f16')
        self._run_convs(st, after)


def get_plan(backbone, device):
    """plan cache on the backbone keyed by device, rebuilt when a parameter / buffer changed (engine.get_plan's rule)"""
    cache = backbone.__dict__.setdefault('_lfd_engine_cache', {})
    key = (device.type, device.index)
    plan = cache.get(key)
    sig = engine._param_signature(backbone)
    if plan is None or plan.param_sig != sig:
        with torch.no_grad():
            plan = ResNetPlan(backbone, device)
        cache[key] = plan
    return plan
