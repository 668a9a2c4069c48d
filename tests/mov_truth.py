"""numpy restatement of the moving-window detectors (include/aether_hip.h, aeth_mov_*): the terms, the ORDER of the f64
additions of a window sum, the metric and the search records.  numpy's cumsum is sequential, so the segment scans restate
directly; every other step is one element-wise numpy operation, rounded on its own.

The order (van Herk's scheme over segments of W terms counted from the call's index 0, history in segments -1, -2, ...):
  position k = j mod W of term j inside its segment, cell c = k // 32 (the last cell of a segment holds W mod 32 terms
  when that is not 0), cps = ceil(W / 32) cells per segment;
    a(k)  the cell's terms from its first through k, added in ascending order from -0.0
    d(k)  the cell's terms from its last down to k, added in descending order from -0.0
    T_c   = a(last k of cell c)
    v     = the log-step scan of T_0 .. T_{cps-1}: for s = 1, 2, 4, ... < cps:  v[c] = v[c - s] + v[c] for c >= s, all c at once
    u     = the same scan of the totals in reverse order, T_{cps-1} .. T_0
    h(k)  = a(k) for c == 0, else v[c - 1] + a(k)                    the segment's terms 0 .. k
    g(k)  = d(k) for c == cps - 1, else u[cps - 2 - c] + d(k)        the segment's terms k .. W - 1
  S(i) = h(W - 1) of i's segment when i mod W == W - 1 (the window is that segment), else g(k + 1) of the segment in front
  + h(k) of i's own, k = i mod W."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
LAG, POWER = 0, 1
CELL = 32
PEAK_DTYPE = np.dtype([("index", np.uint64), ("first", np.uint64), ("p_re", f64), ("p_im", f64), ("r", f64), ("r_lag", f64),
                       ("metric", f32), ("n_nan", np.uint32), ("reserved", np.uint64)])


def history(kind, window, lag):
    return window - 1 + (lag if kind == LAG else 0)


def extended(x, hist, H):
    """the samples of indices -H .. n - 1 (zeros where there is no history)"""
    x = np.ascontiguousarray(x, np.complex64)
    h = np.zeros(H, np.complex64) if hist is None else np.ascontiguousarray(hist, np.complex64)
    assert h.size == H
    return np.concatenate([h, x])


def q(z):
    re, im = z.real.astype(f64), z.imag.astype(f64)
    return re * re + im * im


def lag_terms(a, b):
    """c = a * conj(b), one rounding per component"""
    ar, ai, br, bi = (v.astype(f64) for v in (a.real, a.imag, b.real, b.imag))
    with np.errstate(all="ignore"):
        return ar * br + ai * bi, ai * br - ar * bi


def window_sums(t, W, lo):
    """t: the f64 terms of indices lo .. lo + t.size - 1 -> S(i) for i = lo + W - 1 .. lo + t.size - 1, in the order of
    the module's docstring (segments are counted from index 0, so `lo` matters)"""
    t = np.ascontiguousarray(t, f64)
    hi = lo + t.size                                     # one past the last index
    s0, s1 = lo // W, -(-hi // W)                        # segments s0 .. s1 - 1 cover the terms
    cps = -(-W // CELL)
    pad = np.full((s1 - s0) * W, -0.0)                   # terms nobody needs: in front of lo, behind the last one
    pad[lo - s0 * W: hi - s0 * W] = t
    cells = np.full((s1 - s0, cps * CELL), -0.0)         # -0.0 behind a short last cell: the identity in either direction
    cells[:, :W] = pad.reshape(s1 - s0, W)
    cells = cells.reshape(s1 - s0, cps, CELL)
    with np.errstate(all="ignore"):
        a = np.cumsum(cells, axis=2)
        d = np.cumsum(cells[:, :, ::-1], axis=2)[:, :, ::-1]
        T = a[:, :, -1]
        v, u = T.copy(), T[:, ::-1].copy()
        s = 1
        while s < cps:
            v[:, s:] = v[:, :-s] + v[:, s:]
            u[:, s:] = u[:, :-s] + u[:, s:]
            s *= 2
        h, g = a.copy(), d.copy()
        if cps > 1:
            h[:, 1:, :] = v[:, :-1, None] + a[:, 1:, :]
            g[:, :-1, :] = u[:, ::-1][:, 1:, None] + d[:, :-1, :]          # u[cps - 2 - c] for c = 0 .. cps - 2
        h = h.reshape(s1 - s0, cps * CELL)[:, :W].reshape(-1)
        g = g.reshape(s1 - s0, cps * CELL)[:, :W].reshape(-1)
        i = np.arange(lo + W - 1, hi)
        at = i - s0 * W                                  # where index i sits in h and g
        whole = (i % W) == W - 1
        out = h[at].copy()
        part = ~whole
        out[part] = g[at[part] - (W - 1)] + h[at[part]]
    return out


def sums(x, kind, W, L=0, hist=None):
    """-> dict of the f64 window sums of outputs 0 .. n - 1: "r" (and "p_re", "p_im", "r_lag" for the lag kind)"""
    n = len(x)
    H = history(kind, W, L)
    xe = extended(x, hist, H)
    e = q(xe)                                            # indices -H .. n - 1
    R = window_sums(e, W, -H)                            # R(i) for i = -H + W - 1 .. n - 1
    if kind == POWER:
        return {"r": R}
    a, b = xe[L:], xe[:-L]                               # terms j = -(W - 1) .. n - 1: x_j and x_{j - L}
    c_re, c_im = lag_terms(a, b)
    return {"p_re": window_sums(c_re, W, -(W - 1)), "p_im": window_sums(c_im, W, -(W - 1)), "r": R[L:], "r_lag": R[:n]}


def metric(s, kind, W):
    """M in f64 operations rounded one by one, then to f32"""
    with np.errstate(all="ignore"):
        if kind == POWER:
            return (s["r"] / f64(W)).astype(f32)
        num = s["p_re"] * s["p_re"] + s["p_im"] * s["p_im"]
        den = s["r"] * s["r_lag"]
        safe = np.where(den == 0, 1.0, den)
        return np.where(den == 0, 0.0, num / safe).astype(f32)


def planes(x, kind, W, L=0, hist=None):
    """-> (p complex64 or None, r f32, m f32, the f64 sums)"""
    s = sums(x, kind, W, L, hist)
    with np.errstate(all="ignore"):
        p = None
        if kind == LAG:
            p = np.empty(len(x), np.complex64)
            p.real, p.imag = s["p_re"].astype(f32), s["p_im"].astype(f32)
        return p, s["r"].astype(f32), metric(s, kind, W), s


def same_bits(got, want):
    """bit for bit, except that a NaN matches any NaN"""
    g, w = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if g.shape != w.shape or g.dtype != w.dtype:
        return False
    if g.dtype == np.complex64:
        g, w = g.view(f32), w.view(f32)
    u = {4: np.uint32, 8: np.uint64}[g.dtype.itemsize]
    nan = np.isnan(w)
    return bool((np.isnan(g) == nan).all() and (g.view(u)[~nan] == w.view(u)[~nan]).all())


def fsum_windows(t, W):
    """math.fsum of every window of W terms -> (sums, sums of the magnitudes), one entry per complete window"""
    t = [float(v) for v in t]
    n = len(t) - W + 1
    return (np.array([math.fsum(t[i:i + W]) for i in range(n)]), np.array([math.fsum(abs(v) for v in t[i:i + W]) for i in range(n)]))


def records(m, s, kind, n, block, r_min, threshold):
    """the search records a host forms from the metric plane and the f64 sums: candidates, argmax with ties to the lowest
    index, first crossing"""
    block = block if block else n
    nb = -(-n // block)
    out = np.zeros(nb, PEAK_DTYPE)
    with np.errstate(all="ignore"):
        cand = ~np.isnan(m) & (s["r"] >= r_min)
        if kind == LAG:
            cand &= s["r_lag"] >= r_min
    for b in range(nb):
        lo, hi = b * block, min((b + 1) * block, n)
        out[b] = fold_rows(m[lo:hi], cand[lo:hi], {k: v[lo:hi] for k, v in s.items()}, lo, n, threshold)
    return out


def fold_rows(m, cand, s, lo, n, threshold):
    rec = np.zeros((), PEAK_DTYPE)
    rec["n_nan"] = min(int(np.isnan(m).sum()), 2 ** 32 - 1)
    idx = np.flatnonzero(cand)
    if idx.size == 0:
        rec["index"], rec["first"], rec["metric"] = n, n, np.nan
        return rec
    best = idx[np.argmax(m[idx])]                        # argmax returns the first of equals
    rec["index"], rec["metric"] = lo + best, m[best]
    over = idx[m[idx].astype(f64) >= f64(threshold)]
    rec["first"] = lo + over[0] if over.size else n
    rec["p_re"], rec["p_im"] = (s["p_re"][best], s["p_im"][best]) if "p_re" in s else (0.0, 0.0)
    rec["r"], rec["r_lag"] = s["r"][best], (s["r_lag"][best] if "r_lag" in s else 0.0)
    return rec


def fold_records(recs, n):
    """the record over the whole call from the block records"""
    out = np.zeros((), PEAK_DTYPE)
    out["index"], out["first"], out["metric"] = n, n, np.nan
    nan = 0
    for r in recs:
        nan += int(r["n_nan"])
        if r["index"] != n and (out["index"] == n or r["metric"] > out["metric"]):
            keep_first = min(int(out["first"]), int(r["first"]))
            out = r.copy()
            out["first"] = keep_first
        else:
            out["first"] = min(int(out["first"]), int(r["first"]))
    out["n_nan"] = min(nan, 2 ** 32 - 1)
    out["reserved"] = 0
    return out
