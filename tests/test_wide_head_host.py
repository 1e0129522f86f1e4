"""Heads whose per-level output convs need more than 64 padded rows (a COCO-sized head: 80 class + 4 regression rows) on the
all-HIP training path: what the host side decides before any kernel runs -- train_engine.network_supported's rule, the segment
tables and padded weights of the 128-row conv, the `_w` entry points of the C ABI.  No GPU."""
import ctypes as C
import os

import pytest
import torch

from lfd_amd import _lib, configs
from lfd_amd import train_engine as te


def _sep(num_classes, loss):
    """TT100K_LFD_S (separate classification / regression towers) with another head"""
    return configs.build_model(dict(configs.ARCHS['TT100K_LFD_S'], num_classes=num_classes, classification_loss_type=loss)).train()


def test_build_model_takes_the_class_count():
    m = configs.build_model('WIDERFACE_LFD_S', num_classes=80)
    assert m._num_classes == 80 and m._head.num_cls_channels == 80
    assert configs.ARCHS['WIDERFACE_LFD_S']['num_classes'] == 1                   # the table itself is not edited
    assert configs.build_model('TT100K_LFD_S', num_classes=80)._head.num_cls_channels == 81      # CrossEntropyLoss: + background
    assert configs.build_model('WIDERFACE_LFD_S')._num_classes == 1
    with pytest.raises(ValueError):
        configs.build_model('WIDERFACE_LFD_S', num_classes=0)


def test_network_supported_admits_heads_up_to_128_padded_rows():
    """merged head (cls + reg rows in one conv): num_cls_channels + 4 <= 128; separate towers: num_cls_channels <= 128"""
    assert te.network_supported(configs.build_model('WIDERFACE_LFD_S', num_classes=80).train())
    assert te.network_supported(configs.build_model('WIDERFACE_LFD_S', num_classes=60).train())      # the last 64-row head
    assert te.network_supported(configs.build_model('WIDERFACE_LFD_S', num_classes=61).train())      # the first 128-row one
    assert te.network_supported(configs.build_model('WIDERFACE_LFD_S', num_classes=124).train())     # fills row 127
    assert not te.network_supported(configs.build_model('WIDERFACE_LFD_S', num_classes=125).train())
    assert not te.network_supported(configs.build_model('WIDERFACE_LFD_XS', num_classes=125).train())
    # separate towers: the class conv alone has to fit (TT100K's CrossEntropyLoss adds the background channel)
    assert te.network_supported(_sep(128, 'FocalLoss'))
    assert not te.network_supported(_sep(129, 'FocalLoss'))
    assert te.network_supported(_sep(127, 'CrossEntropyLoss'))
    assert not te.network_supported(_sep(128, 'CrossEntropyLoss'))
    assert te.network_supported(configs.build_model('TT100K_LFD_S', num_classes=80).train())


@pytest.mark.parametrize('name', ['WIDERFACE_LFD_L', 'WIDERFACE_LFD_M', 'WIDERFACE_LFD_S', 'WIDERFACE_LFD_XS', 'TT100K_LFD_L',
                                  'TT100K_LFD_S'])
def test_network_supported_is_unchanged_for_the_shipped_configs(name):
    m = configs.build_model(name).train()
    assert te.network_supported(m)
    _, outs = te.build_network(m)
    assert all(te._out_weight(o)[0].shape[0] == 64 for o in outs)          # and they stay on the 64-row kernels


def test_segment_tables_and_padded_weights_of_an_80_class_merged_head():
    m = configs.build_model('WIDERFACE_LFD_S', num_classes=80).train()
    configs.perturb_weights(m)
    with torch.no_grad():
        for p in m._head.parameters():
            if p.dim() == 1 and p.numel() in (80, 4):
                p.uniform_(-1, 1)               # the output convs' biases are zero at init
    _, outs = te.build_network(m)
    assert len(outs) == m._num_heads               # one conv per level
    for o in outs:
        segs = te._out_segs(o)
        assert [(sg['kind'], sg['row0'], sg['channels']) for sg in segs] == [('cls', 0, 80), ('reg', 80, 4)]
        assert segs[0]['scale'] is None and segs[1]['scale'].data_ptr() == o.scale._scale.data_ptr()
        wp, bp = te._out_weight(o)
        assert tuple(wp.shape) == (128, 128, 1, 1) and tuple(bp.shape) == (128,)
        assert torch.equal(wp[:80], o.convs[0][1].weight.detach()) and torch.equal(wp[80:84], o.convs[1][1].weight.detach())
        assert torch.equal(bp[:80], o.convs[0][1].bias.detach()) and torch.equal(bp[80:84], o.convs[1][1].bias.detach())
        assert bool(bp[:84].any()) and not bool(wp[84:].any()) and not bool(bp[84:].any())


def test_padded_rows_of_the_other_admitted_heads():
    for m, rows in ((configs.build_model('WIDERFACE_LFD_S', num_classes=124).train(), [128]),
                    (configs.build_model('WIDERFACE_LFD_S', num_classes=61).train(), [128]),
                    (_sep(128, 'FocalLoss'), [128, 64]),          # (class conv, regression conv) of a level
                    (configs.build_model('TT100K_LFD_S', num_classes=63).train(), [64, 64])):
        _, outs = te.build_network(m)
        per_level = [te._out_weight(o)[0].shape[0] for o in outs if o.level == 0]
        assert per_level == rows
        for o in outs:
            segs = te._out_segs(o)
            assert segs[-1]['row0'] + segs[-1]['channels'] <= te._out_weight(o)[0].shape[0]


_WIDE = ['lfd_head_out_split_w_f16', 'lfd_head_out_grad_w_f16', 'lfd_head_out_split_concat_w_f16', 'lfd_head_out_grad_concat_w_f16',
         'lfd_head_out_split_levels_w_f16', 'lfd_head_out_grad_levels_w_f16']


def test_the_python_binding_declares_the_wide_entry_points():
    assert set(_WIDE) <= set(_lib.declared_symbols())


@pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH), reason='liblfd_hip.so is not built')
def test_rows_outside_64_and_128_are_refused_on_the_host():
    l = _lib.lib()
    assert all(hasattr(l, s) for s in _WIDE)
    buf = (C.c_char * 64)()
    y = C.c_void_p((C.addressof(buf) + 15) & ~15)
    sg = (_lib.HeadOutSeg * 1)()
    sg[0].channels, sg[0].row0 = 4, 0
    sg[0].out = sg[0].grad = C.cast(y, C.c_void_p).value
    lv = (_lib.HeadOutLevel * 1)()
    lv[0].hw, lv[0].nsegs, lv[0].point0 = 1, 1, 0
    lv[0].segs[0] = sg[0]
    for rows in (0, 32, 96, 127, 129, 256, -64):
        assert l.lfd_head_out_split_w_f16(y, 1, 1, 1, 0, sg, 1, rows, None) == -1
        assert l.lfd_head_out_split_concat_w_f16(y, 1, 1, 1, 0, sg, 1, rows, None) == -1
        assert l.lfd_head_out_grad_w_f16(y, 1, 1, 1, 0, sg, 1, rows, 1.0, y, y, 1 << 20, None) == -1
        assert l.lfd_head_out_grad_concat_w_f16(y, 1, 1, 1, 0, sg, 1, rows, 1.0, y, y, 1 << 20, None) == -1
        assert l.lfd_head_out_split_levels_w_f16(y, 1, 1, lv, 1, rows, None) == -1
        assert l.lfd_head_out_grad_levels_w_f16(y, 1, 1, lv, 1, rows, 1.0, y, y, 1 << 20, None) == -1
    # 128 rows: a segment past row 127, a level that does not fit the point axis, a missing destination -- all before any launch
    sg[0].channels, sg[0].row0 = 4, 126
    assert l.lfd_head_out_split_w_f16(y, 1, 1, 1, 0, sg, 1, 128, None) == -1
    sg[0].row0 = 124
    assert l.lfd_head_out_split_w_f16(y, 1, 2, 1, 0, sg, 1, 128, None) == -1
    sg[0].out = None
    assert l.lfd_head_out_split_w_f16(y, 1, 1, 1, 0, sg, 1, 128, None) == -1
    # an undersized workspace is its own status (128 rows need 1 MB, 64 rows 512 KB)
    assert l.lfd_head_out_grad_w_f16(y, 1, 1, 1, 0, sg, 1, 128, 1.0, y, y, (1 << 20) - 1, None) == -2
    sg[0].row0 = 0
    assert l.lfd_head_out_grad_w_f16(y, 1, 1, 1, 0, sg, 1, 64, 1.0, y, y, (1 << 19) - 1, None) == -2
    assert l.lfd_head_out_grad_levels_w_f16(y, 1, 1, lv, 1, 128, 1.0, y, y, (1 << 20) - 1, None) == -2
