"""tests/golden/conv256_cases.py on the host: the launch geometry it restates against the constants of csrc/conv256.hip it
quotes, the walk property of the walk map, and max |ref| <= 2048 (the range in which fp16 holds every integer) for every case but
the larger walk maps."""
import os
import re

import pytest

import conv_cases as CC
import conv256_cases as K

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'lfd-a-light-and-fast-detector_amd', 'csrc',
                   'conv256.hip')


def _constant(text, pattern):
    m = re.search(pattern, text)
    assert m, pattern
    return [int(v) for v in m.groups()]


def test_the_geometry_restated_equals_the_kernel_source():
    text = open(SRC).read()
    assert _constant(text, r'static constexpr int TH = (\d+), TW = (\d+);') == [K.TH, K.TW]
    assert _constant(text, r'constexpr int C256_MAX_WORKGROUPS = (\d+);') == [K.MAX_WORKGROUPS]
    assert _constant(text, r'constexpr int C256_CIN = (\d+);') == [K.CIN]
    assert 'a.tiles_x = (w + 15) / 16;' in text and 'a.tiles_y = (h + 7) / 8;' in text
    assert 'if (a.cout > 128) return launch256<KS, 4, F32>(a, st);' in text
    assert 'if (a.cout > 64) return launch256<KS, 2, F32>(a, st);' in text
    assert [K.channel_groups(c) for c in (32, 64, 96, 128, 160, 256)] == [1, 1, 2, 2, 4, 4]
    assert K.launch(2, 9, 17) == (2, 2, 8, 8) and K.launch(1, 1, 1) == (1, 1, 1, 1)
    assert K.launch(8, 135, 240) == (15, 17, 2040, 512)


def test_the_cases_cover_what_the_kernel_branches_on():
    cs = K.cases()
    assert {c.cout for c in cs} == {256, 96, 32} and {c.ks for c in cs} == {1, 3}
    assert {K.channel_groups(c.cout) for c in cs} == {4, 2, 1}
    kinds = dict(K.MAPS)
    assert kinds['pixel'] == (1, 1, 1)
    n, h, w = kinds['small']
    assert n == 2 and h < K.TH and w < K.TW
    n, h, w = kinds['edge']
    assert n == 2 and h == K.TH + 1 and w == K.TW + 1          # one ragged row under and one ragged column beside a full tile
    assert len({K.case_seed(c) for c in cs}) == len(cs)


def test_some_workgroup_walks_two_tiles_in_two_images():
    n, h, w = K.walk_shape()
    tx, ty, nt, grid = K.launch(n, h, w)
    assert (tx, ty) == (3, 2) and grid == K.MAX_WORKGROUPS and grid < nt <= 2 * grid
    assert 1.4 <= nt / grid <= 1.6
    twice = [b for b in range(grid) if b + grid < nt]
    assert twice and len(twice) < grid                         # some workgroups run two tiles, some one
    per_image = tx * ty
    for b in twice:
        first, second = b, b + grid
        assert first // per_image != second // per_image       # in different images
        assert first % per_image != second % per_image         # at different places
    assert n * h * w * K.CIN * 2 < 64 * 2 ** 20                # tens of MB


@pytest.mark.parametrize('c', [c for c in K.cases() if c.kind != 'walk'], ids=K.case_id)
def test_integer_references_stay_in_the_exact_range(c):
    o = K.int_operands(c)
    assert float(o.x.abs().max()) <= K.X_HI and float(o.w.abs().max()) <= K.W_HI and float(o.b.abs().max()) <= K.BIAS_HI
    ref = K.case_ref(c, o, 0)
    assert float(ref.abs().max()) <= CC.F16_EXACT
    assert 2 * 9 * K.CIN + K.BIAS_HI < CC.F32_EXACT
