"""numpy restatement of the synthesis bank's definition (include/aether_hip.h, aeth_synth_*): the overlap-add in float32
array operations (numpy rounds every product and every sum, as the definition does; re and im are handled separately so
that Inf, NaN and -0.0 behave as two real multiplications).  Frames are taken in ascending m; an output's first term
assigns, later terms add, and a frame that does not reach an output adds nothing to it."""
import numpy as np


def depth(L, D):
    """K: frames that touch one output sample"""
    return -(-L // D)


def rots(M, D, K, frames, phase, first_frame):
    """rot_m for m = -(K - 1) .. frames - 1 (Python's %: frame numbers below zero wrap to 0 .. M - 1)"""
    if not phase or D == M:
        return [0] * (K - 1 + frames)
    return [(((first_frame + m + 1) % M) * D) % M for m in range(-(K - 1), frames)]


def unfold(g, M, D, v, hist=None, phase=0, first_frame=0):
    g = np.asarray(g, np.float32)
    v = np.asarray(v, np.complex64).reshape(-1, M)
    L = g.size
    K = depth(L, D)
    F = v.shape[0]
    pre = np.zeros(((K - 1), M), np.complex64) if hist is None else np.asarray(hist, np.complex64).reshape(K - 1, M)
    fr = np.concatenate([pre, v])                                    # row h is frame m = h - (K - 1)
    n = F * D
    out = np.zeros(n, np.complex64)
    seen = np.zeros(n, bool)
    j = np.arange(L)
    rs = rots(M, D, K, F, phase, first_frame)
    for h in range(K - 1 + F):
        m = h - (K - 1)
        i = m * D + j
        ok = (i >= 0) & (i < n)
        if not ok.any():
            continue
        ii, jj = i[ok], j[ok]
        row = fr[h][(jj + rs[h]) % M]
        first = ~seen[ii]
        with np.errstate(invalid="ignore", over="ignore"):           # Inf and NaN are data here
            for part, dst in ((row.real, out.real), (row.imag, out.imag)):
                prod = g[jj] * part.astype(np.float32)
                assert prod.dtype == np.float32
                cur = dst[ii]
                dst[ii] = np.where(first, prod, cur + prod)
        seen[ii] = True
    assert seen.all()
    return out


def unfold_f64(g, M, D, v, hist, phase=0, first_frame=0):
    """the definition with exact products summed in f64 / complex128"""
    g = np.asarray(g).astype(np.float64)
    v = np.asarray(v).astype(np.complex128).reshape(-1, M)
    L = g.size
    K = depth(L, D)
    F = v.shape[0]
    pre = np.zeros((K - 1, M), np.complex128) if hist is None else np.asarray(hist).astype(np.complex128).reshape(K - 1, M)
    fr = np.concatenate([pre, v])
    out = np.zeros((K - 1 + F) * D + L, np.complex128)               # out index i + (K - 1) D
    j = np.arange(L)
    for h, rot in enumerate(rots(M, D, K, F, phase, first_frame)):
        out[h * D:h * D + L] += g * fr[h][(j + rot) % M]
    return out[(K - 1) * D:(K - 1) * D + F * D]


def same_bits(got, want):
    """bitwise equal, NaN payloads and signs excluded (IEEE does not pin them)"""
    a = np.ascontiguousarray(got).view(np.float32)
    e = np.ascontiguousarray(want).view(np.float32)
    if a.shape != e.shape:
        return False
    an, en = np.isnan(a), np.isnan(e)
    return bool((an == en).all() and (a.view(np.uint32)[~an] == e.view(np.uint32)[~en]).all())
