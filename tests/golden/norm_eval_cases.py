"""tests/golden/norm_eval_cases.py -- seeded cases, float64 references and derived error bounds for the eval-mode BatchNorm
kernels of csrc/train_bn_eval.hip (fine-tuning with frozen stages / norm_eval): the statistics rows from the running statistics
and the one-pass backward.  Error model, input distributions and launch geometry are norm_cases.py's (nothing tuned here);
tests/test_finetune_host.py keeps the restatement honest against float64 autograd on the CPU, tests/test_gpu_finetune.py compares
the kernels with it.  CPU tensors only.

An eval-mode norm normalises with CONSTANTS (mean, rstd) = (running_mean, 1 / sqrt(running_var + eps)):
    z = relu?(gamma * xhat + beta (+ res)),  xhat = (y - mean) * rstd
    g = dz * mask,  dy = gamma * rstd * g,  dgamma = sum(g * xhat) * inv_scale,  dbeta = sum(g) * inv_scale
-- norm_cases.bn_backward_ref without the two mean terms, which come from differentiating the batch statistics."""
import functools

import torch

from norm_cases import (EPS, activations, bn_apply_ref, bn_chain, f32_out_bound, gradients, norm_params, rand16, running_stats,
                        split_stats, store_bound, sum_bound, undecided)

# (name, (n, h, w, c), mask mode, accumulate onto non-zero dgamma / dbeta).  Modes as norm_cases.BN_PLAIN_CASES: 'z' = ReLU mask
# from the stored z, 'y' = recomputed from y, 'res' = residual + the g output, 'none' = no ReLU
BWD_CASES = [
    ('c8_one_pixel', (1, 1, 1, 8), 'none', False),
    ('c8_255', (1, 5, 51, 8), 'z', False),
    ('c8_256', (2, 8, 16, 8), 'y', False),
    ('c8_257', (1, 1, 257, 8), 'none', False),
    ('c64_accumulate', (3, 7, 9, 64), 'z', True),
    ('c256_residual', (2, 6, 5, 256), 'res', False),
    ('above_grid_cap', (1, 129, 128, 128), 'z', False),       # 264 192 vectors > 1024 * 256
]
PREV_DGAMMA, PREV_DBETA = 2.0, -1.0                           # what an accumulating case adds onto
# one launch of the statistics kernel: single norms, and a table of several norms of different widths
STATS_TABLES = [('c8', [8]), ('c64', [64]), ('c256', [256]), ('table', [64, 8, 256, 128, 64])]
# undecided recomputed masks (norm_cases.undecided): at most this fraction of all elements over the cases, none in a small case
UNDECIDED_FRACTION, UNDECIDED_FREE_BELOW = 1e-4, 10000


def stats_inputs(name):
    """-> [(running_mean, running_var)] fp32 per norm of the table"""
    i = [t[0] for t in STATS_TABLES].index(name)
    return [running_stats(c, 300 + 10 * i + k) for k, c in enumerate(STATS_TABLES[i][1])]


def eval_stats_ref(running_mean, running_var, eps=EPS):
    """-> (mean, rstd) float64"""
    return running_mean.double(), 1.0 / torch.sqrt(running_var.double() + eps)


@functools.lru_cache(maxsize=None)
def bwd_inputs(name):
    i = [c[0] for c in BWD_CASES].index(name)
    _, shape, mode, accumulate = BWD_CASES[i]
    seed, c = 90 + i, shape[3]
    gamma, beta = norm_params(c, seed)
    rm, rv = running_stats(c, seed)
    return dict(shape=shape, mode=mode, accumulate=accumulate, c=c, y=activations(shape, seed), dz=gradients(shape, seed), gamma=gamma,
                beta=beta, running_mean=rm, running_var=rv, res=rand16(shape, 7000 + seed) if mode == 'res' else None)


def stats_row(running_mean, running_var, eps=EPS):
    """the row as an exact kernel would write it: float32[2 * c] = (mean, fp32(rstd))"""
    mean, rstd = eval_stats_ref(running_mean, running_var, eps)
    return torch.cat([mean, rstd]).float()


def mask_of(d, stats, z=None):
    """-> (mask bool [m, c] or None, undecided bool [m, c]).  'z' / 'res': from the given stored output (the forward's own z);
    'y': [gamma * xhat + beta > 0] in float64, with the elements the kernel's fp32 expression may decide either way"""
    c = d['c']
    flat = lambda t: t.reshape(-1, c)
    none = torch.zeros(flat(d['y']).shape, dtype=torch.bool)
    if d['mode'] == 'none':
        return None, none
    if d['mode'] == 'y':
        _, _, pre, terms = bn_apply_ref(flat(d['y']), stats, d['gamma'], d['beta'], None, True)
        return pre > 0, undecided(pre, terms)
    return flat(z) > 0, none


def forward_ref(d, stats):
    """z float64 [m, c] of the case from `stats` (bn_apply_ref)"""
    c = d['c']
    res = None if d['res'] is None else d['res'].reshape(-1, c)
    return bn_apply_ref(d['y'].reshape(-1, c), stats, d['gamma'], d['beta'], res, d['mode'] != 'none')[0]


def bn_eval_backward_ref(dz, y, mask, stats, gamma, inv_scale):
    """dz, y [m, c]; mask bool [m, c] or None; stats float32[2 * c] (the kernel's own row).  -> dict with the results and the sums
    of magnitudes the bounds need (as norm_cases.bn_backward_ref)"""
    mean, rstd = split_stats(stats)
    g = dz.double() if mask is None else dz.double() * mask
    xh = (y.double() - mean) * rstd
    a = gamma.double() * rstd
    s0, s1 = g.sum(0), (g * xh).sum(0)
    return dict(g=g, xh=xh, a=a, m=y.size(0), s0=s0, s1=s1, abs0=g.abs().sum(0), abs1=(g * xh).abs().sum(0),
                dbeta=s0 * inv_scale, dgamma=s1 * inv_scale, dy=a * g)


def bn_eval_backward_bounds(r, chain, inv_scale, prev_dgamma=None, prev_dbeta=None):
    """-> (dy, dgamma, dbeta) bounds: norm_cases.bn_backward_bounds minus the mean terms.  dy = fp16(a * g) is a stored value
    behind a two-rounding fp32 expression of one operand; the sums: `chain` fp32 additions (+ 3 roundings inside a g * xhat
    term), then fp64, leaving the final pass rounded to fp32 (+= onto the previous value in fp32)."""
    d0, d1 = sum_bound(chain, r['abs0']), sum_bound(chain, r['abs1'], 3)
    dy = store_bound(r['dy'], r['a'].abs() * r['g'].abs())
    return (dy, d1 * inv_scale + f32_out_bound(r['dgamma'], prev_dgamma), d0 * inv_scale + f32_out_bound(r['dbeta'], prev_dbeta))


def chain_of(d):
    m = d['y'].numel() // d['c']
    return bn_chain(m, d['c'])


def undecided_census():
    """-> (per case {name: (undecided, elements)}, total undecided, total elements) of the float64 reference on exact rows"""
    per, tot_u, tot = {}, 0, 0
    for name, _, _, _ in BWD_CASES:
        d = bwd_inputs(name)
        st = stats_row(d['running_mean'], d['running_var'])
        _, und = mask_of(d, st, forward_ref(d, st))
        per[name] = (int(und.sum()), und.numel())
        tot_u += int(und.sum())
        tot += und.numel()
    return per, tot_u, tot
