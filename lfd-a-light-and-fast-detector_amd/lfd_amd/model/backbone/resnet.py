"""ResNet -- mirror of the reference's torchvision-style backbone (lfd/model/backbone/resnet.py: BasicBlock :17-76,
Bottleneck :79-191, ResNet :194-492), the one that takes ImageNet-pretrained weights (torchvision key names).

Same constructor signature, defaults and assertions, same public attributes, same parameter names / shapes /
registration order for every depth and option (`state_dict` round-trips with strict=True; `torch.manual_seed(s)` gives the
reference's initial weights), same init (kaiming_normal_ fan_out, zero_init_residual), same init_with_weight_file
(strict=False, the two warnings) and the same train() / frozen_stages / norm_eval behaviour.

Unlike LFDResNet's, `forward` here is plain torch ops in the reference's order: a model in .train() with this backbone runs
backbone, neck and head under PyTorch-ROCm autograd (train_engine.supported answers False).  In eval mode on the device the
models (LFD / LFDv2 / FCOS) do not call it: depth 18 / 34 with the default stem and widths run on the HIP kernels
(engine_resnet.ResNetPlan: csrc/stem7.hip, the max-pool, the block / conv kernels of engine.py); every other option raises
engine.Unsupported there.

Quirks kept from the reference:
  * train() returns None (resnet.py:485-492 has no return), so `ResNet(...).eval()` and `.train()` return None, not the
    module: `bb = ResNet(18).eval()` binds None;
  * norm_eval defaults to True: BatchNorm layers stay on their running statistics in train();
  * `(stage, block) in out_indices` compares tuples: out_indices given as lists tap nothing;
  * num_stages is the largest tapped stage: later stages are not built;
  * a Bottleneck's dcn dict loses its 'fallback_on_stride' entry (popped) on construction.
"""
import os

import torch
import torch.nn as nn

__all__ = ['ResNet']

_NORM_TYPES = (nn.BatchNorm2d, nn.GroupNorm)


def _norm(norm_cfg, channels):
    if norm_cfg['type'] == 'BN':
        return nn.BatchNorm2d(num_features=channels)
    return nn.GroupNorm(num_groups=norm_cfg['num_groups'], num_channels=channels)


def _named_norm(norm_cfg, channels, suffix):
    """('bn1' | 'gn2' | ..., module): the child's name carries the norm type, as the torchvision keys do for BN"""
    return norm_cfg['type'].lower() + str(suffix), _norm(norm_cfg, channels)


def _check_norm_cfg(norm_cfg):
    assert norm_cfg['type'] in ['BN', 'GN']
    if norm_cfg['type'] == 'GN':
        assert 'num_groups' in norm_cfg


class _Block(nn.Module):
    """children in the reference's registration order: norms, convs, relu, downsample"""

    def _add_norms(self, norm_cfg, widths):
        for i, c in enumerate(widths, 1):
            name, mod = _named_norm(norm_cfg, c, i)
            setattr(self, 'norm%d_name' % i, name)
            self.add_module(name, mod)

    @property
    def norm1(self):
        return getattr(self, self.norm1_name)

    @property
    def norm2(self):
        return getattr(self, self.norm2_name)


class BasicBlock(_Block):
    expansion = 1

    def __init__(self, num_input_channels, num_block_channels, stride=1, dilation=1, downsample=None, style='pytorch',
                 norm_cfg=dict(type='BN'), dcn=None, plugins=None):
        super(BasicBlock, self).__init__()
        assert dcn is None, 'Not implemented yet.'
        assert plugins is None, 'Not implemented yet.'
        _check_norm_cfg(norm_cfg)
        c = num_block_channels
        self._add_norms(norm_cfg, (c, c))
        self.conv1 = nn.Conv2d(num_input_channels, c, kernel_size=3, stride=stride, padding=dilation, dilation=dilation, bias=False)
        self.conv2 = nn.Conv2d(c, c, kernel_size=3, padding=1, bias=False)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride
        self.dilation = dilation

    def forward(self, x):
        out = self.relu(self.norm1(self.conv1(x)))
        out = self.norm2(self.conv2(out))
        identity = x if self.downsample is None else self.downsample(x)
        out += identity
        return self.relu(out)


class Bottleneck(_Block):
    expansion = 4

    def __init__(self, num_input_channels, num_block_channels, stride=1, dilation=1, downsample=None, style='pytorch',
                 norm_cfg=dict(type='BN'), dcn=None):
        """style 'pytorch': the 3x3 conv carries the stride; 'caffe': the first 1x1 does"""
        super(Bottleneck, self).__init__()
        assert style in ['pytorch', 'caffe']
        assert dcn is None or isinstance(dcn, dict)
        _check_norm_cfg(norm_cfg)
        c = num_block_channels
        self.num_input_channels = num_input_channels
        self.num_block_channels = c
        self.stride = stride
        self.dilation = dilation
        self.style = style
        self.dcn = dcn
        self.with_dcn = dcn is not None
        self.conv1_stride, self.conv2_stride = (1, stride) if style == 'pytorch' else (stride, 1)
        self._add_norms(norm_cfg, (c, c, c * self.expansion))
        self.conv1 = nn.Conv2d(num_input_channels, c, kernel_size=1, stride=self.conv1_stride, bias=False)
        fallback_on_stride = dcn.pop('fallback_on_stride', False) if self.with_dcn else False
        assert not self.with_dcn or fallback_on_stride, 'DCN is not supported currently.'
        self.conv2 = nn.Conv2d(c, c, kernel_size=3, stride=self.conv2_stride, padding=dilation, dilation=dilation, bias=False)
        self.conv3 = nn.Conv2d(c, c * self.expansion, kernel_size=1, bias=False)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample

    @property
    def norm3(self):
        return getattr(self, self.norm3_name)

    def forward(self, x):
        out = self.relu(self.norm1(self.conv1(x)))
        out = self.relu(self.norm2(self.conv2(out)))
        out = self.norm3(self.conv3(out))
        identity = x if self.downsample is None else self.downsample(x)
        out += identity
        return self.relu(out)


class ResNet(nn.Module):
    """depth in {18, 34, 50, 101, 152}; out_indices: (stage_index, block_index) pairs, the stage 1-based, the block 0-based,
    kept sorted; see the module docstring for what runs where."""

    arch_settings = {
        18: (BasicBlock, (2, 2, 2, 2)),
        34: (BasicBlock, (3, 4, 6, 3)),
        50: (Bottleneck, (3, 4, 6, 3)),
        101: (Bottleneck, (3, 4, 23, 3)),
        152: (Bottleneck, (3, 8, 36, 3)),
    }

    def __init__(self, depth, in_channels=3, base_channels=64, strides=(1, 2, 2, 2), dilations=(1, 1, 1, 1),
                 out_indices=((1, 1), (2, 1), (3, 1), (4, 1)), style='pytorch', deep_stem=False, avg_down=False,
                 frozen_stages=-1, norm_cfg=dict(type='BN', requires_grad=True), norm_eval=True, dcn=None,
                 stage_with_dcn=(False, False, False, False), with_cp=False, zero_init_residual=True,
                 init_with_weight_file=None):
        super(ResNet, self).__init__()
        assert depth in self.arch_settings, 'depth: %s is not supported!' % str(depth)
        _check_norm_cfg(norm_cfg)
        block, blocks_per_stage = self.arch_settings[depth]
        taps = sorted(out_indices, key=tuple)
        num_stages = max(stage for stage, _ in taps)           # only the stages up to the last tapped one are built
        assert 1 <= num_stages <= 4
        blocks_per_stage = blocks_per_stage[:num_stages]
        assert all(1 <= stage and 0 <= index < blocks_per_stage[stage - 1] for stage, index in taps)
        assert dcn is None or len(stage_with_dcn) == num_stages
        # the public attributes: the constructor's arguments under their own names, cut to the stages that exist
        for name, value in dict(depth=depth, base_channels=base_channels, num_stages=num_stages, strides=strides[:num_stages],
                                dilations=dilations[:num_stages], block=block, stage_blocks=blocks_per_stage, out_indices=taps,
                                style=style, deep_stem=deep_stem, avg_down=avg_down, frozen_stages=frozen_stages, norm_cfg=norm_cfg,
                                norm_eval=norm_eval, dcn=dcn, stage_with_dcn=stage_with_dcn, with_cp=with_cp,
                                zero_init_residual=zero_init_residual, init_with_weight_file=init_with_weight_file,
                                inplanes=base_channels).items():
            setattr(self, name, value)

        self._make_stem_layer(in_channels, base_channels)
        for i, num_blocks in enumerate(self.stage_blocks):
            planes = base_channels * 2 ** i
            self._make_stage(i + 1, num_blocks, self.inplanes, planes, self.strides[i], self.dilations[i],
                             self.dcn if self.stage_with_dcn[i] else None)
            self.inplanes = planes * self.block.expansion

        self._init_weights()
        if self.init_with_weight_file is not None:
            assert isinstance(self.init_with_weight_file, str), 'weight file must be the string path of the file!'
            self._init_with_pretrained_weights()

        self._num_output_channels_list = [self.block.expansion * self.base_channels * 2 ** (s - 1) for s, _ in self.out_indices]
        self._num_output_strides_list = [2 ** (s + 1) for s, _ in self.out_indices]

    @property
    def num_output_channels_list(self):
        return self._num_output_channels_list

    @property
    def num_output_strides_list(self):
        return self._num_output_strides_list

    @property
    def norm1(self):
        return getattr(self, self.norm1_name)

    def _make_stem_layer(self, in_channels, base_channels):
        if self.deep_stem:      # three 3x3 convs
            half = base_channels // 2
            mods = []
            for cin, cout, stride in ((in_channels, half, 2), (half, half, 1), (half, base_channels, 1)):
                mods += [nn.Conv2d(cin, cout, kernel_size=3, stride=stride, padding=1, bias=False), _norm(self.norm_cfg, cout),
                         nn.ReLU(inplace=True)]
            self.stem = nn.Sequential(*mods)
        else:
            self.conv1 = nn.Conv2d(in_channels, base_channels, kernel_size=7, stride=2, padding=3, bias=False)
            self.norm1_name, norm1 = _named_norm(self.norm_cfg, base_channels, 1)
            self.add_module(self.norm1_name, norm1)
            self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)

    def _make_stage(self, stage_index, num_blocks, inplanes, planes, stride, dilation, dcn):
        width = planes * self.block.expansion
        downsample = None
        if stride != 1 or inplanes != width:
            mods, conv_stride = [], stride
            if self.avg_down and stride != 1:
                conv_stride = 1
                mods.append(nn.AvgPool2d(kernel_size=stride, stride=stride, ceil_mode=True, count_include_pad=False))
            mods += [nn.Conv2d(inplanes, width, kernel_size=1, stride=conv_stride, bias=False), _norm(self.norm_cfg, width)]
            downsample = nn.Sequential(*mods)
        blocks = nn.ModuleList()
        blocks.append(self.block(inplanes, planes, stride=stride, dilation=dilation, style=self.style, downsample=downsample,
                                 dcn=dcn, norm_cfg=self.norm_cfg))
        for _ in range(1, num_blocks):
            blocks.append(self.block(width, planes, stride=1, dilation=dilation, style=self.style, dcn=dcn, norm_cfg=self.norm_cfg))
        setattr(self, 'layer%d' % stage_index, blocks)

    def _freeze_stages(self):
        """frozen_stages = k >= 0 freezes the stem, k >= 1 also layer1 .. layer{k}: eval mode and no gradients (conv1 has no mode
        of its own and keeps its flag); norm_cfg requires_grad=False stops the gradients of every norm layer"""
        frozen = []
        if not self.norm_cfg.get('requires_grad', True):
            frozen += [m for m in self.modules() if isinstance(m, _NORM_TYPES)]
        if self.frozen_stages >= 0:
            stem = [self.stem] if self.deep_stem else [self.conv1, self.norm1]
            stem[-1].eval()
            frozen += stem
        for stage in range(1, self.frozen_stages + 1):
            for blk in getattr(self, 'layer%d' % stage)[:self.stage_blocks[stage - 1]]:
                blk.eval()
                frozen.append(blk)
        for m in frozen:
            m.requires_grad_(False)

    def _init_with_pretrained_weights(self):
        assert os.path.isfile(self.init_with_weight_file), \
            'pretrained weight file [{}] does not exist!'.format(self.init_with_weight_file)
        weights = torch.load(self.init_with_weight_file)
        missing_keys, unexpected_keys = self.load_state_dict(weights['state_dict'], strict=False)
        for what, keys in (('missing', missing_keys), ('unexpected', unexpected_keys)):
            if keys:
                print('[WARNING: ResNet pretrained weights load] %s keys:' % what)
                print('\t'.join(keys))

    def _init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, _NORM_TYPES):
                if m.weight is not None:
                    nn.init.constant_(m.weight, 1)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
        if self.zero_init_residual:
            for m in self.modules():
                last = m.norm3 if isinstance(m, Bottleneck) else m.norm2 if isinstance(m, BasicBlock) else None
                if last is not None:
                    nn.init.constant_(last.weight, 0)
                    nn.init.constant_(last.bias, 0)

    def forward(self, x):
        x = self.stem(x) if self.deep_stem else self.relu(self.norm1(self.conv1(x)))
        x = self.maxpool(x)
        outs = []
        for i in range(1, self.num_stages + 1):
            for j in range(self.stage_blocks[i - 1]):
                x = getattr(self, 'layer%d' % i)[j](x)
                if (i, j) in self.out_indices:
                    outs.append(x)
        return tuple(outs)

    def train(self, mode=True):
        """nn.Module.train, then the frozen stages, then -- norm_eval -- every BatchNorm back on its running statistics.
        Returns None, like the reference's."""
        nn.Module.train(self, mode)
        self._freeze_stages()
        if not (mode and self.norm_eval):
            return
        for m in self.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eval()
