"""The numpy restatement of aeth_polar_list_* (include/aether_hip.h): the successive-cancellation list decoder with path
metrics, and the pick among its rows.  `paths` is vectorised over codewords and paths: every level of every path is held,
and at an information leaf all of them are gathered by parent; every leaf is walked, nothing is pruned.  `plain_paths` is
the definition read literally, one path and one leaf at a time, each leaf value recomputed from the channel under the
path's own decisions: slow, for n <= 5, and what `paths` is checked against."""
import numpy as np

import polar_truth as T

CODEWORD, ALL = 1, 2
NONE = 0xFFFFFFFF
LIST_RECORD = np.dtype([("metric", np.uint32, 8)])
BIG = np.int64(1) << 40                                           # the metric of a list position not yet in use


def paths(msk, soft, L, trace=None):
    """-> (u [F][L][N] decisions, pm [F][L] metrics), both in the final list order; a list given as `trace` receives the
    metrics [F][L] behind every leaf, in the list order of that moment"""
    msk = np.asarray(msk, np.uint8)
    N = msk.size
    n = N.bit_length() - 1
    assert (1 << min(int(msk.sum()), 3)) >= L, "the code has fewer words than paths"
    F = soft.size // N
    y = np.asarray(soft, np.int8).reshape(F, 1, N).astype(np.int32)
    V = [np.zeros((F, L, 1 << d), np.int32) for d in range(n)] + [np.repeat(y, L, 1)]       # V[d]: the node of 2^d values above the leaf
    X = [np.zeros((F, L, 1 << d), np.uint8) for d in range(n)]                               # X[d]: a finished left child's bits
    u = np.zeros((F, L, N), np.uint8)
    pm = np.full((F, L), BIG, np.int64)
    pm[:, 0] = 0
    fi = np.arange(F)[:, None]
    for i in range(N):
        s = n if i == 0 else (i & -i).bit_length() - 1
        if s < n:
            src, h = V[s + 1], 1 << s
            a, b = src[:, :, :h], src[:, :, h:]
            V[s] = np.where(X[s] == 0, b + a, b - a)
        for d in range(min(s, n) - 1, -1, -1):
            src, h = V[d + 1], 1 << d
            V[d] = T.f_of(src[:, :, :h], src[:, :, h:])
        lam = V[0][:, :, 0].astype(np.int64)
        act = pm < BIG
        if not msk[i]:
            pm = np.where(act & (lam < 0), pm - lam, pm)
            bit = np.zeros((F, L), np.uint8)
        else:
            hard = lam < 0
            c = np.stack([np.where(hard, pm + np.abs(lam), pm), np.where(hard, pm, pm + np.abs(lam))], 2)     # [F][L][b]
            c = np.where(act[:, :, None], c, BIG).reshape(F, 2 * L)
            order = np.argsort(c * (2 * L) + np.arange(2 * L)[None, :], axis=1)[:, :L]       # by (metric, p, b)
            par, bit = order // 2, (order % 2).astype(np.uint8)
            pm = np.take_along_axis(c, order, 1)
            bit = np.where(pm < BIG, bit, 0).astype(np.uint8)
            V = [v[fi, par] if d < n else v for d, v in enumerate(V)]
            X = [x[fi, par] for x in X]
            u = u[fi, par]
        u[:, :, i] = bit
        x = bit[:, :, None]
        d = 0
        while (i >> d) & 1:
            x = np.concatenate([X[d] ^ x, x], 2)
            d += 1
        if d < n:
            X[d] = x
        if trace is not None:
            trace.append(pm.copy())
    assert (pm < BIG).all()
    order = np.argsort(pm * L + np.arange(L)[None, :], axis=1)                               # the final order: (PM, position)
    return u[fi, order], np.take_along_axis(pm, order, 1)


def leaf_values(y, u, i):
    """the value at leaf i for P paths: y [P][N] channel values, u [P][N] decisions (those below i are read)"""
    def rec(Lv, base, m):
        if m == 1:
            return Lv[:, 0]
        h = m // 2
        a, b = Lv[:, :h], Lv[:, h:]
        if i < base + h:
            return rec(T.f_of(a, b), base, h)
        x1 = T.transform(u[:, base:base + h])
        return rec(np.where(x1 == 0, b + a, b - a), base + h, h)
    return rec(y, 0, y.shape[1])


def plain_paths(msk, soft, L):
    """the definition, literally -> [(u [L][N], pm [L])] per codeword"""
    msk = np.asarray(msk, np.uint8)
    N = msk.size
    F = soft.size // N
    y = np.asarray(soft, np.int8).reshape(F, N).astype(np.int32)
    out = []
    for f in range(F):
        u, pm = np.zeros((1, N), np.uint8), [0]
        for i in range(N):
            A = u.shape[0]
            lam = [int(v) for v in leaf_values(np.repeat(y[f:f + 1], A, 0), u, i)]
            if not msk[i]:
                pm = [m + (-v if v < 0 else 0) for m, v in zip(pm, lam)]
                continue
            cand = sorted((pm[p] + (abs(lam[p]) if b != int(lam[p] < 0) else 0), p, b) for p in range(A) for b in (0, 1))[:min(2 * A, L)]
            nu = np.stack([u[p] for _, p, _ in cand]).copy()
            for r, (_, _, b) in enumerate(cand):
                nu[r, i] = b
            u, pm = nu, [c[0] for c in cand]
        order = sorted(range(len(pm)), key=lambda p: (pm[p], p))
        out.append((u[order], np.array(pm, np.int64)[order]))
    return out


def decode(msk, soft, L, flags=0):
    """-> (bits flat uint8 as aeth_polar_list_decode writes them, records [F] of LIST_RECORD)"""
    msk = np.asarray(msk, np.uint8)
    N = msk.size
    u, pm = paths(msk, soft, L)
    F = u.shape[0]
    rows = T.transform(u.reshape(F * L, N)).reshape(F, L, N) if flags & CODEWORD else u[:, :, np.flatnonzero(msk)]
    if not flags & ALL:
        rows = rows[:, 0]
    rec = np.zeros(F, LIST_RECORD)
    rec["metric"] = NONE
    rec["metric"][:, :L] = pm
    return np.ascontiguousarray(rows).ravel(), rec


def metric_of(soft, word):
    """sum over j of |soft_j| [word_j != (soft_j < 0)]: soft [N], word [..][N]"""
    y = np.asarray(soft, np.int8).astype(np.int64)
    return ((np.asarray(word) != (y < 0)) * np.abs(y)).sum(-1)


def pick(rows, row_bytes, L, diff):
    """-> (out [F][row_bytes], which [F] uint32)"""
    rows = np.asarray(rows, np.uint8).reshape(-1, L, row_bytes)
    ok = np.asarray(diff).reshape(-1, L) == 0
    first = ok.argmax(1)
    which = np.where(ok.any(1), first, NONE).astype(np.uint32)
    return rows[np.arange(rows.shape[0]), np.where(ok.any(1), first, 0)], which
