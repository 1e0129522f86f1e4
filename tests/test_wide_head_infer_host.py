"""CPU checks behind tests/test_gpu_wide_head_infer.py -- heads with more than 64 output rows in the 'fp16' inference mode:

  * the gates: for every case of tests/golden/wide_head_cases.py the float32 emulations of k_head2's form (two K orders, the
    instrument's own) stay within a quarter of the gate the device test applies -- head_cases.GATES['head2'], derived over narrower
    heads, or the case's own figure in wide_head_cases.CASE_GATES;
  * the integer instrument keeps its exactness conditions with up to 128 final rows, and the emulations equal float64 there;
  * the walk cases have the properties they are in the table for (from the launch geometry restated in head_cases.py);
  * the plan rule of engine.py without a device: which class counts the head plan takes, and what it says when it refuses;
  * the new export is declared, and the lines of head.hip that head_cases.py restates are still there.
Prints the figures (pytest -s)."""
import functools

import pytest
import torch

import head_cases as H
import wide_head_cases as W
import test_head_reference_host as base
from lfd_amd import _lib, configs, engine

NAMES = [c['name'] for c in W.CASES]
SMALL = [n for n in NAMES if n not in W.WALKS]


@functools.lru_cache(maxsize=None)
def _ops(name, kind):
    return H.operands(W.BY_NAME[name], kind)


# ------------------------------------------------------------------------------------------------ gates
@pytest.mark.parametrize('name', NAMES)
def test_emulations_stay_within_a_quarter_of_the_gate(name):
    c, O = W.BY_NAME[name], _ops(name, 'gauss')
    ref = H.chain(c, O, 'head')
    fig = {}
    for ks in (1, 2):
        e = H.chain(c, O, 'head2', torch.float32, kseed=ks)
        for k in H.GATES['head2']:
            fig[k] = max(fig.get(k, 0.0), H.deviation(e[k], ref[k]))
    for k in H.GATES['head2']:
        g = W.gate(name, k)
        print('%s %s: emulation %.3e  gate %.3e  (gate / figure %.2f)' % (name, k, fig[k], g, g / fig[k] if fig[k] else float('inf')))
    for k in H.GATES['head2']:
        assert fig[k] <= W.gate(name, k) / 4, '%s %s: an emulation exceeds a quarter of the gate' % (name, k)
    for k, g in W.CASE_GATES.get(name, {}).items():       # a case's own gate follows head_cases' rule: 4 x the figure, + a tenth at most
        assert g <= 4 * fig[k] * 1.1 + 1e-12, '%s %s: the gate is slacker than the derivation allows' % (name, k)


def test_case_table():
    assert set(H.final_tiles(c) for c in W.CASES) == {3, 4} and all(H.uses_head2(c) for c in W.CASES)
    rows = set((c['reg_rows'], c['cls_rows']) for c in W.CASES)
    assert {(4, 80), (4, 61), (4, 81), (4, 124), (0, 128), (0, 81)} == rows
    assert W.BY_NAME['w65']['reg_rows'] + W.BY_NAME['w65']['cls_rows'] == 65          # one live row in the third tile
    assert W.BY_NAME['w128']['reg_rows'] + W.BY_NAME['w128']['cls_rows'] == 128       # row 127 live
    assert W.BY_NAME['w84_g8']['groups'] == 8 and not set(W.CASE_GATES) - set(NAMES)
    assert set(W.VARIANTS) == set(H.VARIANTS)


# ------------------------------------------------------------------------------------------------ exactness conditions
@pytest.mark.parametrize('name', SMALL)
def test_exact_conditions_hold_with_wide_rows(name):
    c, O = W.BY_NAME[name], _ops(name, 'int')
    r = H.chain(c, O, 'head', ab=O['ab'], caps=True)
    assert r['round_err'] == 0.0 and r['cap'] < 2.0 ** 24
    for o in O['levels']:
        full, _ = H.hilo(o['bf'])
        assert torch.equal(full, o['bf'].double()) and o['bf'].shape[0] == c['reg_rows'] + c['cls_rows']
    for ks in (1, 2):
        e = H.chain(c, O, 'head2', torch.float32, kseed=ks, ab=O['ab'])
        for k in ('cls', 'reg'):
            assert H.equal(e[k], r[k]), '%s: head2 emulation (K order %d) differs from float64 in %s' % (name, ks, k)
    # a reference that lands the rows of the later tiles on channel `row` instead of `row - reg_rows` is rejected
    if c['reg_rows']:
        bad = H.chain(c, O, 'head2', ab=O['ab'], wrong='cls_shifted')
        assert not H.equal(bad['cls'], r['cls'])


# ------------------------------------------------------------------------------------------------ walk properties
def test_walk_cases_have_their_properties():
    props, w = base._h2_props(W.BY_NAME['w84_walk'])
    print('w84_walk: %d items on %d blocks: %s' % (w['nitems'], w['blocks'], sorted(props)))
    assert {'three_items', 'straddle', 'tail_group', 'chunk2'} <= props and w['nitems'] > 2 * H.H2_BLOCKS
    props, w = base._h2_props(W.BY_NAME['w84_switch'])
    print('w84_switch: %d items on %d blocks: %s' % (w['nitems'], w['blocks'], sorted(props)))
    assert w['nitems'] == 200 and 'level_switch' not in props          # fewer items than blocks: see wide_head_cases.py
    props, w = base._h2_props(W.BY_NAME['w84_switch4'])
    print('w84_switch4: %d items on %d blocks: %s' % (w['nitems'], w['blocks'], sorted(props)))
    assert {'level_switch', 'cin_switch', 'chunk2'} <= props and w['nitems'] > H.H2_BLOCKS


# ------------------------------------------------------------------------------------------------ the plan rule
def _plan(m):
    m.eval()
    return engine.EnginePlan(m._backbone, m._neck, m._head, device=torch.device('cpu'))


@pytest.mark.parametrize('classes,rows,tiles', [(60, 64, 2), (61, 65, 3), (80, 84, 3), (124, 128, 4)])
def test_merged_heads_up_to_124_classes_are_planned(classes, rows, tiles):
    p = _plan(configs.build_model('WIDERFACE_LFD_S', num_classes=classes))
    assert p.cls_channels == classes
    for lv in p.levels:
        (t,) = lv.towers
        assert (t.reg_rows, t.cls_rows) == (4, classes) and t.reg_rows + t.cls_rows == rows
        assert tuple(t.wf.shape) == (tiles, 8, 64, 8) and t.bf.numel() == 32 * tiles        # padded to whole tiles of 32 rows
        assert not bool(t.bf[rows:].any())


def test_separate_towers_up_to_128_class_channels_are_planned():
    for classes in (80, 127):        # CrossEntropyLoss: + the background channel
        p = _plan(configs.build_model(dict(configs.ARCHS['TT100K_LFD_S'], num_classes=classes)))
        assert p.cls_channels == classes + 1
        ct, rt = p.levels[0].towers
        assert (ct.reg_rows, ct.cls_rows, rt.reg_rows, rt.cls_rows) == (0, classes + 1, 4, 0)
        assert ct.wf.shape[0] == (classes + 1 + 31) // 32 and rt.wf.shape[0] == 1
    arch = dict(configs.ARCHS['TT100K_LFD_S'], num_classes=128, classification_loss_type='FocalLoss')     # 128 channels, no background
    if configs.build_model(arch)._head.num_cls_channels == 128:
        assert _plan(configs.build_model(arch)).levels[0].towers[0].wf.shape[0] == 4


def test_heads_past_the_limit_are_refused_by_name():
    with pytest.raises(engine.Unsupported, match=r'num classes \+ 4 > 128 with a merged head'):
        _plan(configs.build_model('WIDERFACE_LFD_S', num_classes=125))
    with pytest.raises(engine.Unsupported, match='more than 128 classification channels'):
        _plan(configs.build_model(dict(configs.ARCHS['TT100K_LFD_S'], num_classes=128)))        # 129 channels
    assert engine.MAX_FINAL_ROWS == 128


def test_a_wide_head_with_small_groups_is_refused_by_group_size():
    arch = dict(configs.ARCHS['WIDERFACE_LFD_S'], gn_groups=32)
    _plan(configs.build_model(arch, num_classes=60))          # 64 rows: the tile kernel serves groups of 4 channels
    with pytest.raises(engine.Unsupported, match=r'groups of at least 8 channels, not 4 \(GroupNorm\(32, 128\)\)'):
        _plan(configs.build_model(arch, num_classes=80))


# ------------------------------------------------------------------------------------------------ the sources
def test_the_export_is_declared_and_the_restated_lines_stand():
    assert 'lfd_head_forward_wide_f16' in _lib.declared_symbols() and 'lfd_head_forward_f16' in _lib.declared_symbols()
    base.test_restated_constants_match_the_sources()
