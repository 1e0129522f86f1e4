"""INT8 calibration rules: the clipping threshold T of an activation tensor from its magnitude histogram, on the host,
in float64.  The histogram is lossless -- h[b] counts the elements whose fp16 pattern & 0x7fff is b (csrc/calib_hist.hip,
ops.abs_histogram_f16) -- so every rule below is evaluated from the values themselves.  The scale of the tensor is T / 127
(engine_i8.act_scale); the int8 kernels saturate at +-127.

Where the reference hands its calibration batches to tensorrt.IInt8EntropyCalibrator2 (lfd/deployment/tensorrt/build_engine.py:22)
this module offers the standard rules of quantisation toolkits; 'entropy' is this project's own definition in the style of the
published descriptions of entropy calibration and does not claim to reproduce TensorRT.

Notation: val(b) the fp16 value of pattern b (increasing in b); N = sum(h); A = val of the largest non-empty bin.  A == 0 gives
T = 0 for every rule.  A non-empty bin at or above 0x7c00 (Inf, NaN) raises ValueError.

Linear bins ('entropy'): nbins bins of width A / nbins; a non-zero magnitude m goes to bin min(nbins - 1, floor(m * nbins / A))
(float64, in that order); zeros are left out.  Candidates ('entropy', 'mse'): i = start_bin, start_bin + stride, ... <= nbins,
and always nbins itself; T(i) = i * A / nbins (float64, in that order), T(nbins) = A.

  'amax'        T = A
  'percentile'  k = ceil(N * percentile / 100) (float64, in that order) clipped to [1, N]; T = the smallest magnitude v with
                #{|x| <= v} >= k, zeros included
  'entropy'     per candidate i: p[b] = h_lin[b] for b < i, the mass of h_lin[i:] added to p[i - 1]; q from h_lin[0:i] without
                that mass: the i bins are split into nlevels groups [floor(g i / nlevels), floor((g + 1) i / nlevels)), each
                group's total is spread evenly over its non-empty bins (q[b] = total / count), empty bins stay 0.  Both are
                normalised by their exact integer sums (P = p / sum(p), Q = q / sum(h_lin[0:i])); KL = sum over P > 0 of
                P * log(P / Q), +inf where Q == 0 < P; the sum is the correctly rounded one (math.fsum), so it does not depend on
                the order.  The smallest KL wins, the smallest i on a tie; every candidate +inf: T = A.
  'mse'         err(T) = sum over b of h[b] * (d * d), d = val(b) - s * min(127, rint(val(b) / s)), s = T / 127, rint half to
                even, correctly rounded sum; on the fine histogram, zeros included (they cost nothing).  The smallest err wins,
                the smallest T on a tie.

Each rule also reports the clipped share #{|x| > T} / N."""
import math

import numpy

BINS = 32768
FIRST_NONFINITE = 0x7c00
ALGORITHMS = ('amax', 'percentile', 'entropy', 'mse')
DEFAULTS = {
    'amax': {},
    'percentile': {'percentile': 99.99},
    'entropy': {'nbins': 2048, 'nlevels': 128, 'start_bin': 128, 'stride': 1},
    'mse': {'nbins': 2048, 'start_bin': 128, 'stride': 8},
}

_VALUES = None


def bin_values():
    """float64 [32768]: val(b); the patterns from 0x7c00 are inf / nan"""
    global _VALUES
    if _VALUES is None:
        _VALUES = numpy.arange(BINS, dtype=numpy.uint16).view(numpy.float16).astype(numpy.float64)
        _VALUES.setflags(write=False)
    return _VALUES


def check_params(algorithm, params=None):
    """(algorithm, {user's keywords}) -> the rule's full parameter dict (defaults filled in, ints and floats normalised);
    ValueError for an unknown rule, an unknown keyword or a value out of range"""
    if algorithm not in ALGORITHMS:
        raise ValueError('unknown calibration algorithm %r (one of %s)' % (algorithm, ', '.join(ALGORITHMS)))
    params = dict(params or {})
    unknown = sorted(set(params) - set(DEFAULTS[algorithm]))
    if unknown:
        raise ValueError('calibration algorithm %r takes no parameter %s (its parameters: %s)'
                         % (algorithm, ', '.join(unknown), ', '.join(sorted(DEFAULTS[algorithm])) or 'none'))
    out = dict(DEFAULTS[algorithm])
    out.update(params)
    for k, v in out.items():
        if isinstance(v, bool) or not isinstance(v, (int, float, numpy.integer, numpy.floating)):
            raise ValueError('calibration parameter %s must be a number, not %r' % (k, v))
        if k == 'percentile':
            out[k] = float(v)
            if not 0.0 < out[k] <= 100.0:
                raise ValueError('percentile must be in (0, 100], not %r' % (v,))
        else:
            if int(v) != v:
                raise ValueError('calibration parameter %s must be an integer, not %r' % (k, v))
            out[k] = int(v)
    if algorithm in ('entropy', 'mse'):
        if out['nbins'] < 2:
            raise ValueError('nbins must be at least 2, not %d' % out['nbins'])
        if not 1 <= out['start_bin'] <= out['nbins']:
            raise ValueError('start_bin must be in [1, nbins = %d], not %d' % (out['nbins'], out['start_bin']))
        if out['stride'] < 1:
            raise ValueError('stride must be at least 1, not %d' % out['stride'])
    if algorithm == 'entropy' and not 1 <= out['nlevels'] <= out['start_bin']:
        raise ValueError('nlevels must be in [1, start_bin = %d], not %d' % (out['start_bin'], out['nlevels']))
    return out


def _counts(hist, name):
    h = numpy.asarray(hist)
    if h.shape != (BINS,) or h.dtype.kind not in 'iu':
        raise ValueError('%s: a magnitude histogram is %d integer counts' % (name, BINS))
    h = h.astype(numpy.int64)
    if int(h.min()) < 0:
        raise ValueError('%s: negative count in the histogram' % name)
    bad = numpy.nonzero(h[FIRST_NONFINITE:])[0]
    if bad.size:
        raise ValueError('calibration tensor %r holds %d non-finite values (Inf or NaN; first pattern 0x%04x): no threshold can be '
                         'chosen for it' % (name, int(h[FIRST_NONFINITE:].sum()), FIRST_NONFINITE + int(bad[0])))
    return h


def amax_of(hist, name='tensor'):
    """A: the value of the largest non-empty bin (0.0 for an empty histogram)"""
    h = _counts(hist, name)
    nz = numpy.nonzero(h)[0]
    return float(bin_values()[nz[-1]]) if nz.size else 0.0


def clipped_share(hist, t):
    """#{|x| > t} / N over the finite bins (0.0 for an empty histogram)"""
    h = numpy.asarray(hist).astype(numpy.int64)[:FIRST_NONFINITE]
    n = int(h.sum())
    return int(h[bin_values()[:FIRST_NONFINITE] > t].sum()) / n if n else 0.0


def candidates(nbins, start_bin, stride):
    c = list(range(start_bin, nbins + 1, stride))
    if c[-1] != nbins:
        c.append(nbins)
    return c


def _candidate_threshold(i, a, nbins):
    return a if i == nbins else i * a / nbins


def linear_histogram(h, a, nbins):
    """int64 [nbins]: the non-zero magnitudes in nbins bins of width a / nbins"""
    nz = numpy.nonzero(h[1:FIRST_NONFINITE])[0] + 1
    idx = numpy.minimum(nbins - 1, numpy.floor(bin_values()[nz] * nbins / a).astype(numpy.int64))
    lin = numpy.zeros(nbins, dtype=numpy.int64)
    numpy.add.at(lin, idx, h[nz])
    return lin


def _percentile(h, a, p):
    n = int(h.sum())
    k = min(max(int(math.ceil(float(n) * p['percentile'] / 100.0)), 1), n)
    b = int(numpy.searchsorted(numpy.cumsum(h), k, side='left'))
    return float(bin_values()[b])


def _entropy(h, a, p):
    nbins, nlevels = p['nbins'], p['nlevels']
    lin = linear_histogram(h, a, nbins)
    cum = numpy.concatenate([[0], numpy.cumsum(lin)])                  # cum[i] = sum(lin[:i])
    nzcum = numpy.concatenate([[0], numpy.cumsum(lin > 0)])
    nzbins = numpy.nonzero(lin)[0]
    total = float(cum[nbins])
    best, best_i = math.inf, None
    g = numpy.arange(nlevels + 1, dtype=numpy.int64)
    for i in candidates(nbins, p['start_bin'], p['stride']):
        if lin[i - 1] == 0 and cum[nbins] > cum[i]:
            continue                                                   # Q[i - 1] == 0 < P[i - 1]: +inf
        bins = nzbins[:nzcum[i]]                                       # the non-empty bins below i
        pb = lin[bins].astype(numpy.float64)
        pb[-1] += float(cum[nbins] - cum[i])                           # (bin i - 1 is non-empty here, or nothing lies above)
        edges = g * i // nlevels
        grp = numpy.searchsorted(edges, bins, side='right') - 1
        tot = (cum[edges[1:]] - cum[edges[:-1]]).astype(numpy.float64)
        cnt = (nzcum[edges[1:]] - nzcum[edges[:-1]]).astype(numpy.float64)
        qb = tot[grp] / cnt[grp]
        big_p = pb / total
        big_q = qb / float(cum[i])
        kl = math.fsum((big_p * numpy.log(big_p / big_q)).tolist())
        if kl < best:
            best, best_i = kl, i
    return a if best_i is None else _candidate_threshold(best_i, a, nbins)


def _mse(h, a, p):
    nbins = p['nbins']
    nz = numpy.nonzero(h[1:FIRST_NONFINITE])[0] + 1
    v = bin_values()[nz]
    cnt = h[nz].astype(numpy.float64)
    best, best_t = math.inf, a
    for i in candidates(nbins, p['start_bin'], p['stride']):
        t = _candidate_threshold(i, a, nbins)
        s = t / 127.0
        d = v - s * numpy.minimum(127.0, numpy.rint(v / s))
        err = math.fsum((cnt * (d * d)).tolist())
        if err < best:
            best, best_t = err, t
    return best_t


_RULES = {'percentile': _percentile, 'entropy': _entropy, 'mse': _mse}


def threshold(hist, algorithm='amax', name='tensor', **params):
    """histogram (32768 integer counts) -> (T, clipped share) under one rule; name: the tensor's, for the error messages"""
    p = check_params(algorithm, params)
    h = _counts(hist, name)
    a = amax_of(h, name)
    if a == 0.0:
        return 0.0, 0.0
    t = a if algorithm == 'amax' else float(_RULES[algorithm](h, a, p))
    return t, clipped_share(h, t)


def thresholds(hists, algorithm='amax', **params):
    """{name: histogram} -> {'amax': {name: A}, 'threshold': {name: T}, 'clipped': {name: share}}"""
    out = dict(amax={}, threshold={}, clipped={})
    for name, h in hists.items():
        out['amax'][name] = amax_of(h, name)
        out['threshold'][name], out['clipped'][name] = threshold(h, algorithm, name, **params)
    return out
