"""The numpy restatement of aeth_ldpc_* (include/aether_hip.h), written from the definition and not from the kernels: the
dense H of a shift table, P = B^-1 A by its own elimination on byte matrices, the systematic encoder, the layered
normalised min-sum decoder vectorised over the checks of a layer and over codewords, and the same decoder as plain
loops over one codeword (`decode_scalar`) to hold the vectorised one against."""
import numpy as np

EARLY, PAYLOAD = 1, 2
BIG = 32767


def dims(shift, z):
    shift = np.asarray(shift, np.int64)
    rows, cols = shift.shape
    return rows, cols, cols * z, rows * z, (cols - rows) * z


def dense_h(shift, z):
    """H [M][N] as uint8: block (r, c) has the one of its row i at column (i + s) mod z"""
    rows, cols, N, M, K = dims(shift, z)
    H = np.zeros((M, N), np.uint8)
    i = np.arange(z)
    for r in range(rows):
        for c in range(cols):
            s = int(shift[r][c])
            if s >= 0:
                H[r * z + i, c * z + (i + s) % z] = 1
    return H


def generator(shift, z):
    """P [M][K] uint8 with B P = A over GF(2), or None where the parity part B is singular"""
    rows, cols, N, M, K = dims(shift, z)
    H = dense_h(shift, z)
    W = np.concatenate([H[:, K:], H[:, :K]], axis=1)                  # [B | A]
    for j in range(M):
        p = np.flatnonzero(W[j:, j])
        if p.size == 0:
            return None
        p = j + int(p[0])
        if p != j:
            W[[j, p]] = W[[p, j]]
        hit = np.flatnonzero(W[:, j])
        hit = hit[hit != j]
        W[hit] ^= W[j]
    return np.ascontiguousarray(W[:, M:])


def encode(shift, z, bits, P=None):
    """[F K] bytes -> [F N] bytes: the information bits & 1, then P u"""
    rows, cols, N, M, K = dims(shift, z)
    P = generator(shift, z) if P is None else P
    u = (np.asarray(bits, np.uint8) & 1).reshape(-1, K)
    par = np.stack([np.bitwise_xor.reduce(P[:, row.astype(bool)], axis=1) for row in u]) if u.size else np.zeros((0, M), np.uint8)
    return np.concatenate([u, par.astype(np.uint8)], axis=1).ravel()


def layers(shift, z):
    """per row: (global index of its first edge, [d][z] variable indices, columns ascending)"""
    shift = np.asarray(shift, np.int64)
    i = np.arange(z)
    out, e = [], 0
    for r in range(shift.shape[0]):
        cs = np.flatnonzero(shift[r] >= 0)
        out.append((e, np.stack([c * z + (i + shift[r][c]) % z for c in cs])))
        e += cs.size
    return out, e


def unsat(lay, Q):
    """[F] unsatisfied checks of the hard decisions Q < 0"""
    hard = Q < 0
    return sum(np.logical_xor.reduce(hard[:, v], axis=1).sum(axis=1) for _, v in lay)


def decode(shift, z, soft, max_iter=20, flags=EARLY, stats=None):
    """[F N] int8 -> ([F nb] uint8, [F][2] uint32 of {iterations, unsatisfied}); stats["max_q"] receives max |Q|"""
    rows, cols, N, M, K = dims(shift, z)
    lay, E = layers(shift, z)
    Q = np.asarray(soft, np.int8).astype(np.int32).reshape(-1, N)
    F = Q.shape[0]
    R = np.zeros((F, E, z), np.int32)
    iters = np.zeros(F, np.int64)
    bad = unsat(lay, Q)
    live = np.ones(F, bool)
    max_q = int(np.abs(Q).max()) if Q.size else 0
    for it in range(max_iter):
        idx = np.flatnonzero(live)
        if idx.size == 0:
            break
        q, rr = Q[idx], R[idx]
        for e0, v in lay:
            d = v.shape[0]
            T = q[:, v] - rr[:, e0:e0 + d]                             # [f][d][z]
            neg = T < 0
            mag_in = np.abs(T)
            a = np.argmin(mag_in, axis=1)                              # the first of equal minima
            m1 = np.minimum(np.min(mag_in, axis=1), BIG)
            rest = mag_in.copy()
            np.put_along_axis(rest, a[:, None, :], BIG, axis=1)
            m2 = np.minimum(np.min(rest, axis=1), BIG)
            is_a = np.arange(d)[None, :, None] == a[:, None, :]
            mag = np.minimum((3 * np.where(is_a, m2[:, None, :], m1[:, None, :])) >> 2, 127)
            par = np.logical_xor.reduce(neg, axis=1)
            new = np.where(par[:, None, :] ^ neg, -mag, mag)
            rr[:, e0:e0 + d] = new
            q[:, v] = T + new
        Q[idx], R[idx] = q, rr
        max_q = max(max_q, int(np.abs(q).max()))
        iters[idx] = it + 1
        bad[idx] = unsat(lay, q)
        if flags & EARLY:
            live[idx] = bad[idx] != 0
    if stats is not None:
        stats["max_q"] = max_q
    nb = K if flags & PAYLOAD else N
    bits = (Q[:, :nb] < 0).astype(np.uint8)
    return bits.ravel(), np.stack([iters, bad], axis=1).astype(np.uint32)


def decode_scalar(shift, z, soft, max_iter=20, flags=EARLY):
    """one codeword, plain loops over checks and edges"""
    rows, cols, N, M, K = dims(shift, z)
    Q = [int(x) for x in np.asarray(soft, np.int8)]
    assert len(Q) == N
    R = {}

    def edges(r, i):
        return [(c, c * z + (i + int(shift[r][c])) % z) for c in range(cols) if int(shift[r][c]) >= 0]

    def count():
        n = 0
        for r in range(rows):
            for i in range(z):
                par = 0
                for _, v in edges(r, i):
                    par ^= Q[v] < 0
                n += par
        return n

    iters, bad = 0, count()
    for it in range(max_iter):
        for r in range(rows):
            for i in range(z):
                ed = edges(r, i)
                T = [Q[v] - R.get((r, c, i), 0) for c, v in ed]
                m1 = m2 = BIG
                a, par = -1, 0
                for k, t in enumerate(T):
                    par ^= t < 0
                    m = abs(t)
                    if m < m1:
                        m2, m1, a = m1, m, k
                    elif m < m2:
                        m2 = m
                for k, (c, v) in enumerate(ed):
                    mag = min((3 * (m2 if k == a else m1)) >> 2, 127)
                    new = -mag if par ^ (T[k] < 0) else mag
                    R[(r, c, i)] = new
                    Q[v] = T[k] + new
        iters, bad = it + 1, count()
        if flags & EARLY and bad == 0:
            break
    nb = K if flags & PAYLOAD else N
    return np.array([q < 0 for q in Q[:nb]], np.uint8), (iters, bad)


SHAPES = ((2, 4, 1), (3, 6, 5), (4, 8, 27), (4, 24, 64), (12, 24, 81), (6, 12, 96))


def test_codes():
    """{name: (shift, z)}: the staircase codes of SHAPES (col_weight 3, or `rows` where that is less; seed 0) and one whose
    row 0 holds a single block"""
    from aether_primitives_amd.ldpc import staircase
    out = {f"{r}x{c}x{z}": (staircase(r, c, z), z) for r, c, z in SHAPES}
    one = staircase(3, 7, 13, 2, seed=5)
    one[0, :4] = -1                                                    # row 0 keeps its diagonal parity block alone
    out["single-block-row"] = (one, 13)
    return out


test_codes.__test__ = False


def bpsk_soft(rng, coded, sigma):
    """BPSK over AWGN: bit 0 -> +1; soft = rint(8 y / sigma^2) clamped to +-127"""
    y = 1.0 - 2.0 * (np.asarray(coded, np.uint8) & 1) + sigma * rng.standard_normal(np.asarray(coded).size)
    return np.clip(np.rint(8.0 * y / sigma ** 2), -127, 127).astype(np.int8)
