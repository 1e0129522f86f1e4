"""What an LFD model's module tree consists of, as plain records: the one place that knows how LFDResNet, SimpleNeck and
LFDHead lay out their children (lfd_resnet.py:96-154, :354-501, simple_neck.py:35-47, lfd_head.py:86-149), and how the
torchvision-style ResNet does (resnet.py:17-76, :348-400; resnet_layers).

No device tensors, no folding, no kernel knowledge, and no opinion on what is supported: every launch plan (engine, engine_p2,
engine_p32, engine_sibling*, engine_g1), the training schedules (train_engine) and the PyTorch-ROCm training route
(model/lfd.py) iterate these records and keep their own lowering and their own refusals.
"""
import collections

import torch.nn as nn

_UNION = ('IoULoss', 'GIoULoss', 'DIoULoss', 'CIoULoss')     # the regression losses whose head has a Scale per level

# conv -> norm (None without one) -> ReLU when `relu`; ks / stride: the conv's (square) kernel size and stride; act: the module
# that follows conv and norm in the model (None: none), which `relu` is derived from
Layer = collections.namedtuple('Layer', 'conv norm relu ks stride act')
# one residual block, in execution order: `downsample` is the identity branch's Layer (None: the block's input);
# `relu` on the last of `convs` means "after the residual add" (lfd_resnet.py:140-152); tap: the block's output is a pyramid tap
Block = collections.namedtuple('Block', 'stage index downsample convs tap')
Backbone = collections.namedtuple('Backbone', 'stem blocks')
# one pyramid level: the neck's Layer (None: no neck given), the tower Layers (`merge`, or `cls` and `reg`), the output convs
# and the level's Scale module (None: the regression loss has none)
Level = collections.namedtuple('Level', 'neck merge cls reg cls_out reg_out scale')


class UnknownModule(ValueError):
    """split_sequential met a module it has no step for; callers turn this into their own error type"""


def layer(conv, norm=None, act=None):
    """the Layer of a conv, its norm and the module that follows them (a ReLU or not)"""
    return Layer(conv, norm, isinstance(act, nn.ReLU), conv.kernel_size[0], conv.stride[0], act)


def _groups(seq, n, has_norm):
    """the first n (conv, norm, activation) groups of a Sequential built with or without norms"""
    step = 3 if has_norm else 2
    return [layer(seq[i * step], seq[i * step + 1] if has_norm else None, seq[i * step + step - 1]) for i in range(n)]


def backbone_layers(bb):
    """LFDResNet -> Backbone(stem Layers, Blocks); the taps, in order, are those of bb._out_indices (sorted)"""
    has_norm = bb._norm_cfg is not None
    taps = [tuple(t) for t in bb._out_indices]
    blocks = []
    for i, nblk in enumerate(bb._body_architecture):
        for j in range(nblk):
            blk = getattr(bb, 'stage%d' % i)[j]
            ds = blk._downsample
            if ds is not None:
                ds = layer(ds[0], ds[1] if len(ds) > 1 else None, None)
            convs = [layer(getattr(blk, '_conv%d' % ci), getattr(blk, '_norm%d' % ci, None), blk._activation)
                     for ci in range(1, blk.num_convs + 1)]
            blocks.append(Block(i, j, ds, convs, (i, j) in taps))
    return Backbone(_groups(bb._stem, len(bb.stem_spec()), has_norm), blocks)


def resnet_layers(bb):
    """ResNet (model/backbone/resnet.py) -> Backbone: stem = [Layer(conv1, norm1, relu), 'pool'] (deep_stem: the Layers of
    bb.stem, then 'pool'); one Block per BasicBlock / Bottleneck with convs = [conv + norm + ReLU, ..., last conv + norm (ReLU
    after the add)] and downsample = Layer(1x1, norm) (avg_down: its AvgPool2d is NOT described -- callers that lower the
    records look at bb.avg_down).  Block.stage is 1-based like bb.out_indices, whose order the taps have."""
    taps = [tuple(t) for t in bb.out_indices]
    if bb.deep_stem:
        stem = _groups(bb.stem, 3, True) + ['pool']
    else:
        stem = [layer(bb.conv1, bb.norm1, bb.relu), 'pool']
    blocks = []
    for i in range(1, bb.num_stages + 1):
        for j in range(bb.stage_blocks[i - 1]):
            blk = getattr(bb, 'layer%d' % i)[j]
            ds = blk.downsample
            if ds is not None:
                ds = layer(ds[-2], ds[-1], None)
            nconv = 3 if hasattr(blk, 'conv3') else 2
            convs = [layer(getattr(blk, 'conv%d' % ci), getattr(blk, 'norm%d' % ci), blk.relu) for ci in range(1, nconv + 1)]
            blocks.append(Block(i, j, ds, convs, (i, j) in taps))
    return Backbone(stem, blocks)


def lfd_head_levels(neck, head):
    """(SimpleNeck | None, LFDHead | LFDHeadV1) -> [Level]; a shared head (share_head_flag) yields the same module
    objects for every level"""
    necks = [None if neck is None else _groups(getattr(neck, 'neck%d' % i), 1, neck._norm_cfg is not None)[0]
             for i in range(head._num_heads)]
    has_norm = head._norm_cfg is not None
    nl = head._num_conv_layers
    levels = []
    for i in range(head._num_heads):
        cls_path = getattr(head, 'head%d_classification_path' % i)
        reg_path = getattr(head, 'head%d_regression_path' % i)
        merge = cls = reg = ()
        if head._merge_path_flag:
            merge = _groups(getattr(head, 'head%d_merge_path' % i), nl, has_norm)
        else:
            cls, reg = _groups(cls_path, nl, has_norm), _groups(reg_path, nl, has_norm)
        if hasattr(head, '_classifiers'):      # LFDHeadV1: per-level output convs outside the (shared) towers
            cls_out, reg_out = head._classifiers[i], head._regressors[i]
        else:
            lstep = 3 if has_norm else 2
            cls_out, reg_out = cls_path[len(cls) * lstep], reg_path[len(reg) * lstep]
        levels.append(Level(necks[i], list(merge), list(cls), list(reg), cls_out, reg_out,
                            head._scales[i] if head._regression_loss_type in _UNION else None))
    return levels


def split_sequential(seq):
    """modules of [conv, (norm), (ReLU)] groups / bare ReLU / MaxPool2d -> list of Layer | 'relu' | 'pool' steps.  Layers that
    lfd_head_levels grouped by position pass through when the grouping here would have formed them, and raise alike otherwise"""
    mods = list(seq)
    steps, i = [], 0
    while i < len(mods):
        m = mods[i]
        if isinstance(m, Layer):
            for x, kinds in ((m.norm, (nn.BatchNorm2d, nn.GroupNorm)), (m.act, nn.ReLU)):
                if x is not None and not isinstance(x, kinds):
                    raise UnknownModule('module %s in a neck / head path' % type(x).__name__)
            steps.append(m)
            i += 1
        elif isinstance(m, nn.Conv2d):
            norm, act, j = None, None, i + 1
            if j < len(mods) and isinstance(mods[j], (nn.BatchNorm2d, nn.GroupNorm)):
                norm, j = mods[j], j + 1
            if j < len(mods) and isinstance(mods[j], nn.ReLU):
                act, j = mods[j], j + 1
            steps.append(layer(m, norm, act))
            i = j
        elif isinstance(m, nn.ReLU):
            steps.append('relu')
            i += 1
        elif isinstance(m, nn.MaxPool2d):
            if (m.kernel_size, m.stride, m.padding) != (3, 2, 1):
                raise UnknownModule('MaxPool2d %s' % (m,))
            steps.append('pool')
            i += 1
        else:
            raise UnknownModule('module %s in a neck / head path' % type(m).__name__)
    return steps
