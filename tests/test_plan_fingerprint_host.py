"""Every launch plan and training schedule, for every configuration of tests/golden/plan_fingerprint.py, is what the builders
produced before the model walk moved into lfd_amd/netdesc.py: op and conv order, buffer numbering, every attribute and the
bytes of every folded / packed tensor (tests/golden/plan_fingerprints.json, recorded on CPU tensors; no GPU)."""
import json

import pytest

import plan_fingerprint as PF

RECORDED = json.load(open(PF.FIXTURE))


def test_every_configuration_and_plan_is_recorded():
    assert sorted(PF.keys()) == sorted(RECORDED)


@pytest.mark.parametrize('key', sorted(RECORDED))
def test_plan_fingerprint(key):
    got = PF.fingerprint(*key.split('/'))
    want = RECORDED[key]
    changed = [i for i, (a, b) in enumerate(zip(got, want)) if a != b]
    assert got == want, ('%s: %d lines (recorded %d), first changed line %s -- `python tests/golden/plan_fingerprint.py --lines %s` '
                         'at both commits shows it' % (key, len(got), len(want), changed[:1] or min(len(got), len(want)), key))
