"""numpy restatement of the rational resampler's definition (include/aether_hip.h, aeth_resamp_*): float32 array
operations (numpy rounds every product and every sum, as the definition does; re and im are handled separately so that
Inf, NaN and -0.0 behave as two real multiplications).  The sum starts from the p = 0 product and runs left to right."""
import numpy as np


def resamp(h, U, Q, x, hist=None):
    h = np.asarray(h, np.float32); x = np.asarray(x, np.complex64); P = h.size // U
    no = (x.size // Q) * U
    pre = np.zeros(P - 1, np.complex64) if hist is None else np.asarray(hist, np.complex64)
    assert pre.size == P - 1
    ext = np.concatenate([pre, x])                       # s[i] = ext[i + P - 1]
    k = np.arange(no, dtype=np.int64); a = (k * Q) // U; r = (k * Q) % U
    out = np.empty(no, np.complex64)
    with np.errstate(invalid="ignore", over="ignore"):   # Inf and NaN are data here
        for part, dst in ((ext.real, out.real), (ext.imag, out.imag)):
            acc = None
            for p in range(P):
                pr = h[p * U + r] * part[a - p + P - 1].astype(np.float32)
                assert pr.dtype == np.float32
                acc = pr if acc is None else acc + pr
            dst[...] = acc
    return out


def resamp_f64(h, U, Q, x):
    """an independent formulation in complex128: zero stuffing, convolution, picking (zero history)"""
    h = np.asarray(h).astype(np.float64); x = np.asarray(x).astype(np.complex128)
    n = x.size
    v = np.zeros(n * U, np.complex128); v[::U] = x
    w = np.convolve(v, h)[:n * U]
    return w[::Q][:(n // Q) * U]


def covers(U, Q, P, n_out, i):
    """the outputs whose window s[a - P + 1 .. a] covers input sample i"""
    k = np.arange(n_out, dtype=np.int64); a = (k * Q) // U
    return (a - (P - 1) <= i) & (i <= a)
