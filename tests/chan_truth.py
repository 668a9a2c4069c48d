"""numpy restatement of the filter bank's definition (include/aether_hip.h, aeth_chan_*): the fold in float32 array
operations (numpy rounds every product and every sum, as the definition does; re and im are handled separately so that
Inf, NaN and -0.0 behave as two real multiplications), the transform in complex128."""
import numpy as np


def rots(M, D, frames, phase, first_frame):
    if not phase:
        return [0] * frames
    return [(((first_frame + m + 1) % M) * D) % M for m in range(frames)]


def fold(w, M, D, x, hist=None, phase=0, first_frame=0):
    w = np.asarray(w, np.float32)
    x = np.asarray(x, np.complex64)
    L = w.size
    P = L // M
    F = x.size // D
    pre = np.zeros(L - D, np.complex64) if hist is None else np.asarray(hist, np.complex64)
    assert pre.size == L - D
    ext = np.concatenate([pre, x])                                   # s[i] = ext[i + L - D]: frame m is ext[m D .. m D + L)
    fr = ext[np.arange(F)[:, None] * D + np.arange(L)[None, :]]
    out = np.empty((F, M), np.complex64)
    for part, dst in ((fr.real, out.real), (fr.imag, out.imag)):
        prod = (w[None, :] * part.astype(np.float32)).reshape(F, P, M)
        assert prod.dtype == np.float32
        acc = prod[:, 0, :].copy()
        for p in range(1, P):
            acc = acc + prod[:, p, :]
        dst[...] = acc
    for m, rot in enumerate(rots(M, D, F, phase, first_frame)):
        if rot:
            out[m] = np.roll(out[m], rot)                            # u[q] = v[(q - rot) mod M]
    return out.reshape(-1)


def transform(u, M, sign, factor):
    """factor * DFT_M with exponent sign, per frame, complex128"""
    u = np.asarray(u).astype(np.complex128).reshape(-1, M)
    X = np.fft.fft(u, axis=1) if sign < 0 else np.fft.ifft(u, axis=1) * M
    return (X * float(factor)).reshape(-1)


def same_bits(got, want):
    """bitwise equal, NaN payloads and signs excluded (IEEE does not pin them)"""
    g = np.ascontiguousarray(got).view(np.float32)
    e = np.ascontiguousarray(want).view(np.float32)
    if g.shape != e.shape:
        return False
    gn, en = np.isnan(g), np.isnan(e)
    return bool((gn == en).all() and (g.view(np.uint32)[~gn] == e.view(np.uint32)[~en]).all())
