"""The numpy restatement of aeth_turbo_* (include/aether_hip.h): the recursive systematic constituent code, the encoder with
its two tails, the windowed max-log-MAP pass and the iterations with their record.

`siso_plain` is the header's text with plain loops over windows, steps and states on Python integers, one codeword at a
time.  `siso` does the same steps on [codewords][windows][states] arrays (int64, so that a value that left int32 would
show), the loop running over a window's steps only; tests/test_turbo_truth.py shows the two equal.  `decode` uses `siso`."""
import numpy as np

EARLY = 1
NEG = -(1 << 28)
RECORD = np.dtype([("iterations", np.uint32), ("disagreements", np.uint32)])
NAMED = {"lte": (4, 0o13, 0o15), "ccsds": (5, 0o23, 0o33), "k3": (3, 0o7, 0o5)}
MIN_K, MAX_K = 8, 8192


def parity(v):
    return bin(int(v)).count("1") & 1


def qpp(K, f1, f2):
    """pi[i] = (f1 i + f2 i^2) mod K as Python integers; None when that is no permutation"""
    pi = [(f1 * i + f2 * i * i) % K for i in range(K)]
    return np.array(pi, np.uint32) if len(set(pi)) == K else None


class Code:
    """the transition tables of one constituent code"""

    def __init__(self, k, fb, ff):
        self.k, self.fb, self.ff = k, fb, ff
        self.nu = nu = k - 1
        self.S = S = 1 << nu
        self.nxt = np.zeros((S, 2), np.int64)
        self.z = np.zeros((S, 2), np.int64)
        for s in range(S):
            for u in (0, 1):
                a = u ^ parity(s & fb & (S - 1))
                reg = (a << nu) | s
                self.z[s, u] = parity(reg & ff)
                self.nxt[s, u] = reg >> 1
        self.tail_u = np.array([parity(s & fb & (S - 1)) for s in range(S)], np.int64)
        # the two branches into a state: pred_s[s'][b], pred_u[s'][b]
        self.pred_s = np.zeros((S, 2), np.int64)
        self.pred_u = np.zeros((S, 2), np.int64)
        fill = [0] * S
        for s in range(S):
            for u in (0, 1):
                n = self.nxt[s, u]
                self.pred_s[n, fill[n]], self.pred_u[n, fill[n]] = s, u
                fill[n] += 1
        assert fill == [2] * S


def named(name):
    return Code(*NAMED[name])


def rsc(code, u):
    """[F][K] bits -> (z [F][K], tail x [F][nu], tail z [F][nu]); every row ends in state 0"""
    u = np.asarray(u, np.int64) & 1
    F, K = u.shape
    s = np.zeros(F, np.int64)
    z = np.zeros((F, K), np.uint8)
    for t in range(K):
        z[:, t] = code.z[s, u[:, t]]
        s = code.nxt[s, u[:, t]]
    tx = np.zeros((F, code.nu), np.uint8)
    tz = np.zeros((F, code.nu), np.uint8)
    for j in range(code.nu):
        ut = code.tail_u[s]
        tx[:, j], tz[:, j] = ut, code.z[s, ut]
        s = code.nxt[s, ut]
    assert (s == 0).all()
    return z, tx, tz


def encode(code, pi, bits):
    """F K bytes -> F N coded bits, N = 3 K + 4 nu, planar"""
    pi = np.asarray(pi, np.int64)
    K = pi.size
    u = (np.asarray(bits, np.uint8) & 1).reshape(-1, K)
    F = u.shape[0]
    z1, tx1, tz1 = rsc(code, u)
    z2, tx2, tz2 = rsc(code, u[:, pi])
    tail = np.zeros((F, 4 * code.nu), np.uint8)
    tail[:, 0:2 * code.nu:2], tail[:, 1:2 * code.nu:2] = tx1, tz1
    tail[:, 2 * code.nu::2], tail[:, 2 * code.nu + 1::2] = tx2, tz2
    return np.concatenate([u, z1, z2, tail], axis=1).ravel()


def siso_plain(code, x, p, K, W, A):
    """one codeword, x and p of K + nu Python integers -> D of K integers; the header's text step by step"""
    S, nu = code.S, code.nu
    x, p = [int(v) for v in x], [int(v) for v in p]

    def g(t, s, u):
        return (1 - 2 * u) * x[t] + (1 - 2 * int(code.z[s, u])) * p[t]

    def fwd(alpha, t):
        new = [None] * S
        for s in range(S):
            for u in (0, 1):
                n, v = int(code.nxt[s, u]), alpha[s] + g(t, s, u)
                new[n] = v if new[n] is None else max(new[n], v)
        return new

    def bwd(beta, t):
        return [max(g(t, s, u) + beta[int(code.nxt[s, u])] for u in (0, 1)) for s in range(S)]

    D = [0] * K
    for w0 in range(0, K, W):
        e = min(w0 + W, K)
        if w0 - A <= 0:
            t, alpha = 0, [0] + [NEG] * (S - 1)
        else:
            t, alpha = w0 - A, [0] * S
        while t < w0:
            alpha, t = fwd(alpha, t), t + 1
        store = {}
        while t < e:
            store[t] = alpha
            alpha, t = fwd(alpha, t), t + 1
        if e + A >= K:
            t, beta = K + nu, [0] + [NEG] * (S - 1)
        else:
            t, beta = e + A, [0] * S
        while t > e:
            t -= 1
            beta = bwd(beta, t)
        while t > w0:
            t -= 1
            m = [max(store[t][s] + g(t, s, u) + beta[int(code.nxt[s, u])] for s in range(S)) for u in (0, 1)]
            D[t] = m[0] - m[1]
            beta = bwd(beta, t)
    return D


class Range:
    """the least and greatest intermediate value seen (tests: nothing leaves int32)"""

    def __init__(self):
        self.lo, self.hi = 0, 0

    def see(self, a):
        self.lo, self.hi = min(self.lo, int(a.min())), max(self.hi, int(a.max()))
        return a


def siso(code, x, p, K, W, A, seen=None):
    """[F][K + nu] int64 x and p -> D [F][K]: `siso_plain` for every codeword, all windows in step"""
    S, nu = code.S, code.nu
    F = x.shape[0]
    see = seen.see if seen is not None else (lambda a: a)
    w0 = np.arange(0, K, W, dtype=np.int64)
    nw = w0.size
    e = np.minimum(w0 + W, K)
    sign_u = np.array([1, -1], np.int64)[None, None, None, :]
    sign_z = (1 - 2 * code.z)[None, None, :, :]
    start = np.zeros((F, nw, S), np.int64)
    exact = np.zeros((F, nw, S), np.int64)
    exact[:, :, 1:] = NEG

    def gamma(t):
        """[F][nw][S][2] branch values of step t[w] (t clipped where a window idles)"""
        tc = np.clip(t, 0, K + nu - 1)
        return see(sign_u * x[:, tc][:, :, None, None] + sign_z * p[:, tc][:, :, None, None])

    # forward
    alpha = np.where((w0 - A <= 0)[None, :, None], exact, start)
    store = np.zeros((F, K, S), np.int64)
    for r in range(-A, W):
        t = w0 + r
        on = (t >= 0) & (t < e)
        if not on.any():
            continue
        if r >= 0:
            store[:, t[on], :] = alpha[:, on, :]
        cand = see(alpha[:, :, :, None] + gamma(t))
        new = cand[:, :, code.pred_s, code.pred_u].max(axis=3)
        alpha = np.where(on[None, :, None], new, alpha)
    # backward
    last = e + A >= K
    beta = np.where(last[None, :, None], exact, start)
    D = np.zeros((F, K), np.int64)
    for j in range(A + nu, -W, -1):
        t = e + j - 1 if j > 0 else w0 + (W - 1 + j)
        if j > 0:
            on = np.where(last, t < K + nu, j <= A)
        else:
            on = t < e
        if not on.any():
            continue
        gm = gamma(t)
        out = see(gm + beta[:, :, code.nxt])                               # [F][nw][S][2]: g + beta[s'(s, u)]
        if j <= 0:
            tot = see(store[:, np.clip(t, 0, K - 1), :][:, :, :, None] + out).max(axis=2)
            D[:, t[on]] = (tot[:, :, 0] - tot[:, :, 1])[:, on]
        beta = np.where(on[None, :, None], out.max(axis=3), beta)
    return see(D)


def scale(e):
    return np.sign(e) * np.minimum((3 * np.abs(e)) >> 3, 2047)


def split(code, K, soft):
    """[F][N] int8 -> s [F][K], (p1 | tail z) and (p2 | tail z') [F][K + nu], tail x and x' [F][nu], all int64"""
    nu = code.nu
    v = np.asarray(soft, np.int8).reshape(-1, 3 * K + 4 * nu).astype(np.int64)
    t = v[:, 3 * K:]
    p1 = np.concatenate([v[:, K:2 * K], t[:, 1:2 * nu:2]], axis=1)
    p2 = np.concatenate([v[:, 2 * K:3 * K], t[:, 2 * nu + 1::2]], axis=1)
    return v[:, :K], p1, p2, t[:, 0:2 * nu:2], t[:, 2 * nu::2]


def decode(code, pi, W, A, soft, max_iter, flags=0, seen=None, history=None):
    """-> (F K decisions, flat uint8; records [F]); seen, a Range, is shown every intermediate value; history, a list,
    receives (h2 [F][K], disagreements [F]) of every iteration of a run without EARLY"""
    pi = np.asarray(pi, np.int64)
    K = pi.size
    s, p1, p2, t1, t2 = split(code, K, soft)
    F = s.shape[0]
    see = seen.see if seen is not None else (lambda a: a)
    a1 = np.zeros((F, K), np.int64)
    bits = np.zeros((F, K), np.uint8)
    rec = np.zeros(F, RECORD)
    live = np.arange(F)
    for it in range(1, max_iter + 1):
        if live.size == 0:
            break
        x1 = see(s[live] + a1[live])
        D1 = siso(code, np.concatenate([x1, t1[live]], axis=1), p1[live], K, W, A, seen)
        a2 = scale(see(D1 - 2 * x1))[:, pi]
        x2 = see(s[live][:, pi] + a2)
        D2 = siso(code, np.concatenate([x2, t2[live]], axis=1), p2[live], K, W, A, seen)
        e2 = scale(see(D2 - 2 * x2))
        a1[np.ix_(live, pi)] = e2
        h2 = np.zeros((live.size, K), np.uint8)
        h2[:, pi] = D2 < 0
        dis = ((D1 < 0) != (h2 != 0)).sum(axis=1)
        bits[live] = h2
        rec["iterations"][live], rec["disagreements"][live] = it, dis
        if history is not None:
            assert not flags & EARLY
            history.append((h2.copy(), dis.copy()))
        if flags & EARLY:
            live = live[dis != 0]
    return bits.ravel(), rec


def from_history(history, max_iter, flags=0):
    """what `decode` returns for max_iter <= len(history), with or without EARLY, from one run's history: a codeword's
    iterations do not depend on when its neighbours stop"""
    F = history[0][1].size
    last = np.full(F, max_iter, np.int64)
    if flags & EARLY:
        for it in range(max_iter, 0, -1):
            last[history[it - 1][1] == 0] = it
    bits = np.stack([history[last[f] - 1][0][f] for f in range(F)])
    rec = np.zeros(F, RECORD)
    rec["iterations"] = last
    rec["disagreements"] = [history[last[f] - 1][1][f] for f in range(F)]
    return bits.ravel(), rec


def soft_of_bits(coded, level=127):
    """the noise-free soft values of coded bits: +level for 0, -level for 1"""
    return (level - 2 * level * (np.asarray(coded, np.int16) & 1)).astype(np.int8)


def noisy_soft(rng, coded, sigma, scale_to=16.0):
    """BPSK +-1 through AWGN of deviation sigma, scaled and clamped to int8"""
    y = 1.0 - 2.0 * (np.asarray(coded, np.float64) % 2) + sigma * rng.standard_normal(np.size(coded))
    return np.clip(np.rint(scale_to * y), -128, 127).astype(np.int8)


def test_codes():
    """{name: (code name, pi, W, A)}: the codes of tests/test_gpu_turbo.py"""
    return {
        "k3_8": ("k3", qpp(8, 3, 4), 8, 0),
        "lte40_full": ("lte", qpp(40, 3, 10), 40, 0),
        "lte40_16_8": ("lte", qpp(40, 3, 10), 16, 8),
        "lte40_8_0": ("lte", qpp(40, 3, 10), 8, 0),
        "lte37_rand": ("lte", np.random.default_rng(37).permutation(37).astype(np.uint32), 5, 3),
        "ccsds64": ("ccsds", qpp(64, 7, 16), 16, 16),
        "lte512": ("lte", qpp(512, 31, 64), 32, 16),
        "lte1024": ("lte", qpp(1024, 31, 64), 8, 8),
        "lte6144": ("lte", qpp(6144, 263, 480), 32, 32),
    }


test_codes.__test__ = False
