"""Fingerprints of every launch plan and training schedule the host code builds from a model's module tree.

    python tests/golden/plan_fingerprint.py --write          record tests/golden/plan_fingerprints.json
    python tests/golden/plan_fingerprint.py --lines [KEY]    print the full lines (of one 'config/plan' key) for diffing

plan_fingerprints.json was recorded from the plan builders as they stood BEFORE the model walk moved into lfd_amd/netdesc.py
(this file imports nothing from it): tests/test_plan_fingerprint_host.py asserts that the builders still produce it.  A
difference is a changed plan -- op order, buffer numbering, an attribute, a folded or packed tensor -- never a fixture to
regenerate.

Weights: every parameter and buffer is filled by a closed-form integer rule (no RNG): element i of tensor number k is
((i * 2654435761 + 97 k) mod 257 - 128) / 256, a running_var 1 + (i mod 7) / 8; norm affine parameters are therefore
non-trivial, so a wrong norm, a wrong eps or a dropped bias changes the digests.  The plans are built on CPU tensors.

One line per op / conv / level / tower / path / unit / output record, in order, after one line of the plan's own scalar
attributes.  A line holds every attribute: scalars as they print, tensors as shape, dtype and the first 12 hex digits of the
sha256 of their bytes, modules as their qualified name in model.named_modules(), nested tuples and records flattened the same
way.  A plan's fingerprint is the list of the first 12 hex digits of the sha256 of its lines; a refused configuration is the
line 'raises <type>: <message>'.

The training schedules (train_engine.build_units / build_network) are built on the model in training mode, whether or not their
gates (train_engine.supported / network_supported) admit it.  WALK_CHANGES names the five schedules that cannot keep their record:
the old walk assumed a norm after every conv and LFDHead's output convs at the end of the paths, and failed there; the
description must not, so these build now.  Their line is a constant.
"""
import contextlib
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (ROOT, os.path.join(ROOT, 'lfd-a-light-and-fast-detector_amd')):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402
import torch.nn as nn  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'plan_fingerprints.json')
CPU = torch.device('cpu')
# plan attributes that are not part of what a plan computes: its inputs, caches and device
_SKIP = ('device', 'dev', 'backbone', 'neck', 'head', 'param_sig', 'bb_plan')
_SWITCHES = ('LFD_FUSED_BLOCK', 'LFD_FUSED_STEM', 'LFD_P32_TAIL', 'LFD_P32_MERGE', 'LFD_P32_PLANES', 'LFD_P2_STEM2X', 'LFD_P2_BLOCK',
             'LFD_P2_LEVELS', 'LFD_P2_FLATHEAD', 'LFD_P2_FORK', 'LFD_FUSED_DOWN', 'LFD_FUSED_BLOCK128', 'LFD_HEAD_DECODE')


# ---------------------------------------------------------------------------- weights
def fill(model):
    """closed-form values for every parameter and buffer, numbered in state_dict order (aliased tensors once)"""
    seen, k = set(), 0
    with torch.no_grad():
        for name, t in model.state_dict().items():
            if name.endswith('num_batches_tracked') or t.data_ptr() in seen:
                continue
            seen.add(t.data_ptr())
            i = torch.arange(t.numel(), dtype=torch.int64)
            if name.endswith('running_var'):
                v = 1 + (i % 7).double() / 8
            else:
                v = ((i * 2654435761 + 97 * k) % 257 - 128).double() / 256
            t.copy_(v.reshape(t.shape).to(t.dtype))
            k += 1
    return model


# ---------------------------------------------------------------------------- configurations
def _xs(**kw):
    from lfd_amd import configs
    return dict(configs.ARCHS['WIDERFACE_LFD_XS'], **kw)


def _variant(arch, backbone_norm=True, head_norm='GroupNorm'):
    """configs.build_model for `arch` with a norm-free backbone or BatchNorm head towers"""
    from lfd_amd import configs
    from lfd_amd.model.backbone import LFDResNet
    from lfd_amd.model.head import LFDHead
    from lfd_amd.model.lfd import LFD
    from lfd_amd.model.losses import CrossEntropyLoss, FocalLoss, IoULoss, QualityFocalLoss
    from lfd_amd.model.neck import SimpleNeck

    def bb(**kw):
        return LFDResNet(**(kw if backbone_norm else dict(kw, norm_cfg=None)))

    def head(**kw):
        return LFDHead(**(kw if head_norm == 'GroupNorm' else dict(kw, norm_cfg=dict(type=head_norm))))

    return configs.build_modules(arch, bb, SimpleNeck, head, LFD, FocalLoss, IoULoss, CrossEntropyLoss, 666, QualityFocalLoss)


def configurations():
    """{name: (builder, {environment switch: value})}"""
    from lfd_amd import configs
    c = {}
    for n in sorted(configs.ARCHS):
        c[n] = (lambda n=n: configs.build_model(n), {})
    for n in ('WIDERFACE_LFD_S', 'WIDERFACE_LFD_XS'):
        c[n + '_gray'] = (lambda n=n: configs.build_model(n, input_channels=1), {})
    for n in sorted(configs.PRESETS):
        c['preset_' + n] = (lambda n=n: configs.build_model(configs.PRESETS[n]), {})
    for n in sorted(configs.SIBLINGS):
        c['sibling_' + n] = (lambda n=n: configs.build_sibling_model(n), {})
    c['XS_backbone_without_norm'] = (lambda: _variant(_xs(), backbone_norm=False), {})
    c['XS_shared_head'] = (lambda: configs.build_model(_xs(share_head_flag=True)), {})
    c['XS_unshared_head'] = (lambda: configs.build_model(_xs(share_head_flag=False)), {})
    c['XS_two_towers'] = (lambda: configs.build_model(_xs(merge_path_flag=False)), {})
    c['XS_batchnorm_towers'] = (lambda: _variant(_xs(), head_norm='BatchNorm2d'), {})
    c['S_80_classes'] = (lambda: configs.build_model('WIDERFACE_LFD_S', num_classes=80), {})
    for sw in ('LFD_FUSED_BLOCK', 'LFD_FUSED_STEM', 'LFD_P32_TAIL'):
        c['WIDERFACE_LFD_S_%s_0' % sw] = (lambda: configs.build_model('WIDERFACE_LFD_S'), {sw: '0'})
    return c


# ---------------------------------------------------------------------------- plans
def _sibling_plan(m):
    from lfd_amd import engine_sibling
    with torch.no_grad():
        return engine_sibling.SiblingPlan(m._backbone, m._neck, m._head, CPU)


def _training(build):
    def run(m):
        m.train()
        try:
            return build(m)
        finally:
            m.eval()
    return run


# 'config/plan' -> why the schedule differs from what the builders gave before lfd_amd/netdesc.py (each raised there)
WALK_CHANGES = {
    'TL_LFD_L/train_network': 'norm-free head towers: the old walk strode over (conv, norm, ReLU) triples (IndexError)',
    'TL_LFD_S/train_network': 'norm-free head towers: the old walk strode over (conv, norm, ReLU) triples (IndexError)',
    'XS_backbone_without_norm/train_units': 'norm-free backbone: the old walk read a norm behind the downsample conv and every block conv (IndexError)',
    'XS_backbone_without_norm/train_network': 'norm-free backbone: the old walk read a norm behind the downsample conv and every block conv (IndexError)',
    'sibling_LFDV2_HEADV1/train_network': 'LFDHeadV1: the old walk took the output convs from the end of the paths (IndexError)',
}


def plans():
    """{name: model -> plan object, tuple of record lists, or a string}"""
    from lfd_amd import engine, engine_p2, engine_p32, engine_sibling_p32, train_engine as te

    def engine_plan(m, with_head):
        with torch.no_grad():
            return engine.EnginePlan(m._backbone, m._neck if with_head else None, m._head if with_head else None, CPU)

    return {
        'engine': lambda m: engine_plan(m, True),
        'engine_backbone': lambda m: engine_plan(m, False),
        'planes': lambda m: engine_p2.PlanesPlan(m, CPU),
        'precise': lambda m: engine_p32.PrecisePlan(m, CPU),
        'sibling_precise_merge': lambda m: engine_sibling_p32.SiblingPrecisePlan(m, CPU, merge=True),
        'sibling_precise_two_launches': lambda m: engine_sibling_p32.SiblingPrecisePlan(m, CPU, merge=False),
        'sibling': _sibling_plan,
        'train_units': _training(lambda m: te.build_units(m._backbone)),
        'train_network': _training(te.build_network),
    }


# ---------------------------------------------------------------------------- lines
def _is_record(v):
    return (not isinstance(v, (nn.Module, torch.Tensor, type)) and type(v).__module__.startswith('lfd_amd')
            and (hasattr(v, '__slots__') or hasattr(v, '__dict__')))


def _fields(v):
    if hasattr(v, '__slots__'):
        return [(k, getattr(v, k, '<unset>')) for k in v.__slots__]
    return sorted((k, x) for k, x in vars(v).items() if not k.startswith('_'))


def _key_order(kv):
    return (type(kv[0]).__name__, kv[0])


class _Writer(object):
    def __init__(self, model):
        self.names = {}
        for n, mod in model.named_modules():
            self.names.setdefault(id(mod), n or '<model>')
        self.lines = []

    def flat(self, v):
        if isinstance(v, torch.Tensor):
            t = v.detach().contiguous()
            raw = t.reshape(-1).view(torch.uint8).numpy().tobytes() if t.numel() else b''
            return 'T%s:%s:%s' % (list(t.shape), str(t.dtype).replace('torch.', ''), hashlib.sha256(raw).hexdigest()[:12])
        if isinstance(v, nn.Module):
            return 'M:' + self.names.get(id(v), '?' + type(v).__name__)
        if isinstance(v, (list, tuple)):
            return '(' + ','.join(self.flat(x) for x in v) + ')'
        if isinstance(v, dict):
            return '{' + ','.join('%s=%s' % (k, self.flat(x)) for k, x in sorted(v.items(), key=_key_order)) + '}'
        if _is_record(v):
            return '<' + ' '.join('%s=%s' % (k, self.flat(x)) for k, x in _fields(v)) + '>'
        if v is None or isinstance(v, (bool, int, float, str)):
            return repr(v)
        return '?' + type(v).__name__

    def emit(self, prefix, v):
        """one line for record `v`; its attributes that are lists of records follow as lines of their own"""
        own, later = [], []
        for k, x in (_fields(v) if _is_record(v) else sorted(v.items())):
            if k in _SKIP or k.startswith('_'):
                continue
            if isinstance(x, (list, tuple)) and x and all(_is_record(e) or isinstance(e, dict) for e in x):
                later.append((k, x))
            else:
                own.append('%s=%s' % (k, self.flat(x)))
        self.lines.append(prefix + ' ' + ' '.join(own))
        for k, xs in later:
            for i, e in enumerate(xs):
                self.emit('%s.%s[%d]' % (prefix, k, i), e)


def lines_of(model, result):
    w = _Writer(model)
    if isinstance(result, str):
        return [result]
    if isinstance(result, tuple):               # train_engine: (units, taps) / (units, outs)
        for part, xs in zip('ab', result):
            if xs and all(_is_record(e) for e in xs):
                for i, e in enumerate(xs):
                    w.emit('%s[%d]' % (part, i), e)
            else:
                w.lines.append('%s %s' % (part, w.flat(xs)))
        return w.lines
    w.emit('plan', result)
    if hasattr(result, 'launch_names'):
        w.lines.append('launches ' + ','.join(result.launch_names()))
    return w.lines


@contextlib.contextmanager
def _environment(env):
    old = {k: os.environ.get(k) for k in _SWITCHES}
    for k in _SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


_models = {}


def model_of(config):
    if config not in _models:
        _models[config] = fill(configurations()[config][0]()).eval()
    return _models[config]


def lines(config, plan):
    if config + '/' + plan in WALK_CHANGES:
        return ['changed by the description: ' + WALK_CHANGES[config + '/' + plan]]
    m = model_of(config)
    with _environment(configurations()[config][1]):
        try:
            result = plans()[plan](m)
        except Exception as e:      # a refusal (or whatever else the builder raises) is part of the record
            result = 'raises %s: %s' % (type(e).__name__, e)
    return lines_of(m, result)


def fingerprint(config, plan):
    return [hashlib.sha256(l.encode()).hexdigest()[:12] for l in lines(config, plan)]


def keys():
    return ['%s/%s' % (c, p) for c in configurations() for p in plans()]


if __name__ == '__main__':
    if '--write' in sys.argv:
        out = {k: fingerprint(*k.split('/')) for k in keys()}
        with open(FIXTURE, 'w') as f:
            json.dump(out, f, separators=(',', ':'), sort_keys=True)
            f.write('\n')
        print('%d plans, %d lines, %d bytes' % (len(out), sum(len(v) for v in out.values()), os.path.getsize(FIXTURE)))
    elif '--lines' in sys.argv:
        want = [a for a in sys.argv[1:] if not a.startswith('--')] or keys()
        for k in want:
            print('== ' + k)
            for l in lines(*k.split('/')):
                print(l)
    else:
        print(__doc__)
