"""numpy restatement of the synchronisation estimators' terms (include/aether_hip.h, aeth_sync_*): float32 arrays with one
operation per statement (numpy rounds every product and every sum, as the definition does), the phasor from
tests/nco_truth.py, the terms widened to float64 exactly as defined, and a reference sum by math.fsum per component."""
import math

import numpy as np

import nco_truth

f32, f64 = np.float32, np.float64
SQUARE, POW1, POW2, POW4, POW8 = 0, 1, 2, 4, 8
KINDS = (SQUARE, POW1, POW2, POW4, POW8)
POWERS = (1, 2, 4, 8)
RECORD_DTYPE = np.dtype([("re", f64), ("im", f64), ("mass", f64), ("n", np.uint64), ("n_nonfinite", np.uint64),
                         ("reserved", np.uint64)])
QUIET = dict(invalid="ignore", over="ignore", under="ignore")        # Inf, NaN and denormals are data here


def parts(x):
    x = np.ascontiguousarray(x, np.complex64)
    return x.real.astype(f32), x.imag.astype(f32)


def sq(re, im):
    with np.errstate(**QUIET):
        a = re * re
        b = im * im
        p = re * im
        out_re = a - b
        out_im = p + p
    assert out_re.dtype == f32 and out_im.dtype == f32
    return out_re, out_im


def pw(re, im, m):
    assert m in POWERS
    while m > 1:
        re, im = sq(re, im)
        m //= 2
    return re, im


def q(re, im):
    with np.errstate(**QUIET):
        a = re.astype(f64) * re.astype(f64)
        b = im.astype(f64) * im.astype(f64)
        return a + b


def line_terms(x, kind, words=None, n0=0):
    """-> (t_re, t_im, weight), float64 arrays, one entry per sample"""
    re, im = parts(x)
    if words is None:
        words = (0, 0, 0)
    c, d = nco_truth.phasor(nco_truth.words_at(words, nco_truth.positions(n0, re.size)))
    c, d = c.astype(f64), d.astype(f64)
    with np.errstate(**QUIET):
        if kind == SQUARE:
            f = q(re, im)
            return f * c, f * d, f
        zr32, zi32 = pw(re, im, kind)
        zr, zi = zr32.astype(f64), zi32.astype(f64)
        a = zr * c                      # products of two widened f32 values are exact: each line below is one rounding
        b = zi * d
        e = zr * d
        g = zi * c
        return a - b, e + g, q(zr32, zi32)


def lag_terms(x, power, lag, hist=None):
    """-> (t_re, t_im, weight, exists): terms i < lag exist only with a history (its `lag` samples stand in front of x)"""
    x = np.ascontiguousarray(x, np.complex64)
    n = x.size
    exists = np.ones(n, bool)
    if hist is None:
        exists[:lag] = False
        front = np.zeros(lag, np.complex64)
    else:
        front = np.ascontiguousarray(hist, np.complex64)
        assert front.size == lag
    prev = np.concatenate([front, x])[:n]
    ar32, ai32 = pw(*parts(x), power)
    br32, bi32 = pw(*parts(prev), power)
    ar, ai, br, bi = (v.astype(f64) for v in (ar32, ai32, br32, bi32))
    with np.errstate(**QUIET):
        a = ar * br
        b = ai * bi
        e = ai * br
        g = ar * bi
        return a + b, e - g, q(ar32, ai32), exists


def nonfinite(t_re, t_im):
    return ~(np.isfinite(t_re) & np.isfinite(t_im))


def fsum(v):
    """math.fsum with IEEE's answer where fsum has none (an Inf or NaN among the terms)"""
    v = np.asarray(v, f64)
    if not np.isfinite(v).all():
        with np.errstate(**QUIET):
            return float(np.sum(v))
    return math.fsum(v.tolist())


def records(t_re, t_im, wt, block, exists=None):
    """the reference records of a call: fsum per component and block -> (structured array, per-block sum of |t| for re and im)"""
    n = t_re.size
    block = block if block else n
    exists = np.ones(n, bool) if exists is None else exists
    nb = -(-n // block)
    out = np.zeros(nb, RECORD_DTYPE)
    mag = np.zeros((nb, 2))
    for b in range(nb):
        s = slice(b * block, min((b + 1) * block, n))
        k = exists[s]
        r, i, w = t_re[s][k], t_im[s][k], wt[s][k]
        out[b] = (fsum(r), fsum(i), fsum(w), r.size, int(nonfinite(r, i).sum()), 0)
        with np.errstate(**QUIET):
            mag[b] = (fsum(np.abs(r)), fsum(np.abs(i)))
    return out, mag


def same_f64_bits(got, want):
    """bit for bit, except that a NaN matches any NaN"""
    g, w = np.ascontiguousarray(got, f64), np.ascontiguousarray(want, f64)
    nan = np.isnan(w)
    return bool(g.shape == w.shape and (np.isnan(g) == nan).all() and (g.view(np.uint64)[~nan] == w.view(np.uint64)[~nan]).all())


def turns(re, im):
    return 0.0 if re == 0.0 and im == 0.0 else math.atan2(im, re) / (2 * math.pi)
