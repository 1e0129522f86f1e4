"""tests/golden/lfd_head_cases.py -- the LFD compositions over pyramid necks that the tests of the LFDHead training node share
(tests/test_lfd_head_train_host.py, tests/test_gpu_lfd_head_train.py): specs for configs.build_sibling_model."""
from lfd_amd import configs

FIVE_RANGES = ((4, 32), (32, 64), (64, 128), (128, 256), (256, 512))


def variant(head=None, neck=None, **top):
    """LFDV2_SFPN with head / neck / top-level keywords replaced (neck='FCOS_FPN': that composition's 128-channel, 5-output FPN)"""
    spec = dict(configs.SIBLINGS['LFDV2_SFPN'])
    spec['head'] = dict(spec['head'], **(head or {}))
    if neck == 'FCOS_FPN':
        spec['neck'] = dict(configs.SIBLINGS['FCOS_FPN']['neck'])
        spec['regression_ranges'] = FIVE_RANGES
    else:
        spec['neck'] = dict(spec['neck'], **(neck or {}))
    spec.update(top)
    return spec


# the compositions of the node tests: name -> spec
NODE_CASES = {
    'sfpn': configs.SIBLINGS['LFDV2_SFPN'],                                              # 3x3, separate towers, shared, 64 channels
    'merged1x1': variant(dict(conv_kernel_size=1, merge_path_flag=True)),
    'fpn128-ce': variant(dict(num_head_channels=128, norm_cfg=dict(type='GroupNorm', num_groups=16)), 'FCOS_FPN',
                         classification_loss_type='CrossEntropyLoss'),                  # C + 1 class channels
    'unshared': variant(dict(share_head_flag=False)),
    'no-layers': variant(dict(num_conv_layers=0)),
    'no-scale': variant(regression_loss_type='SmoothL1Loss', range_assign_mode='longer'),     # ('sqrt' asks for an IoU loss)
    # input channels != head channels (64 -> 128 first tower conv) and a merged path of 3x3 convs
    'wide-merged3x3': variant(dict(num_head_channels=128, norm_cfg=dict(type='GroupNorm', num_groups=16), merge_path_flag=True)),
}
V1_SPEC = variant(dict(configs.SIBLINGS['LFDV2_HEADV1']['head']))                       # LFDHeadV1 (BatchNorm towers) behind the SFPN
V1_SPEC['head'].pop('conv_kernel_size')
