"""numpy restatement of the arbitrary-ratio resampler's definition (include/aether_hip.h, aeth_arb_*): Python integers
for the time word, float32 array operations for the samples (numpy rounds every product and every sum, as the
definition does; re and im are handled separately so that Inf, NaN and -0.0 behave as two real multiplications).  The
sum starts from the p = 0 product and runs left to right."""
import numpy as np

ONE = 1 << 32


def advance(step, phase, n):
    """(count, next phase) of a call over n input samples, in Python integers"""
    end = n * ONE
    count = 0 if phase >= end else -(-(end - phase) // step)
    return count, phase + count * step - end


def words(step, phase, n):
    """the time words t(m) = phase + m * step below n * 2^32, as Python integers"""
    return [phase + m * step for m in range(advance(step, phase, n)[0])]


def split(t, b):
    """(a, r, mu) of the time words: sample index, phase row, and the f32 weight of the next row"""
    a = np.array([w >> 32 for w in t], np.int64)
    f = [w & (ONE - 1) for w in t]
    r = np.array([(v >> (32 - b)) if b else 0 for v in f], np.int64)
    mu24 = np.array([((v << b) & (ONE - 1)) >> 8 for v in f], np.int64)
    mu = mu24.astype(np.float32) * np.float32(2.0 ** -24)
    assert mu.dtype == np.float32 and (mu.astype(np.float64) * 2.0 ** 24 == mu24).all()       # exact
    return a, r, mu


def deltas(h):
    """d[j] = fl32(h[j + 1] - h[j]) with h[T] = +0.0"""
    h = np.asarray(h, np.float32)
    d = np.concatenate([h[1:], np.zeros(1, np.float32)]) - h
    assert d.dtype == np.float32
    return d


def arb(h, b, x, step, phase=0, hist=None):
    h = np.asarray(h, np.float32); x = np.asarray(x, np.complex64)
    L = 1 << b; P = h.size // L
    assert P * L == h.size
    d = deltas(h)
    pre = np.zeros(P - 1, np.complex64) if hist is None else np.asarray(hist, np.complex64)
    assert pre.size == P - 1
    ext = np.concatenate([pre, x])                       # s[i] = ext[i + P - 1]
    a, r, mu = split(words(step, phase, x.size), b)
    out = np.empty(a.size, np.complex64)
    if not a.size:
        return out
    assert a.max() <= x.size - 1
    with np.errstate(invalid="ignore", over="ignore"):   # Inf and NaN are data here
        for part, dst in ((ext.real, out.real), (ext.imag, out.imag)):
            acc = None
            for p in range(P):
                j = p * L + r
                md = mu * d[j]
                c = h[j] + md
                pr = c * part[a - p + P - 1].astype(np.float32)
                assert md.dtype == c.dtype == pr.dtype == np.float32
                acc = pr if acc is None else acc + pr
            dst[...] = acc
    return out


def arb_f64(h, b, x, step, phase=0):
    """an independent formulation in complex128 (zero history): the continuous impulse response is the polygon through
    (j, h[j]), j = 0 .. T, with h[T] = 0, on a time axis of 1 / L input samples; output m is the sum over the inputs i of
    x[i] * hc((t(m) - i) L), with the whole 32-bit fraction of t(m) (the definition keeps 24 bits of the weight)."""
    h = np.asarray(h).astype(np.float64); x = np.asarray(x).astype(np.complex128)
    L = 1 << b; P = h.size // L
    knots = np.arange(h.size + 1, dtype=np.float64)
    hext = np.concatenate([h, np.zeros(1)])
    t = words(step, phase, x.size)
    out = np.zeros(len(t), np.complex128)
    for m, w in enumerate(t):
        a = w >> 32
        u = (w & (ONE - 1)) * L / ONE                    # f L < 2^44: exact in f64
        lo = max(0, a - (P - 1))
        i = np.arange(lo, a + 1)
        out[m] = np.sum(x[i] * np.interp((a - i) * L + u, knots, hext))
    return out


def covers(a, P, i):
    """the outputs (by their sample index a) whose window s[a - P + 1 .. a] covers input sample i"""
    return (a - (P - 1) <= i) & (i <= a)
