"""CPU: the restatement tests/polar_truth.py against the definition's own algebra -- the transform against the Kronecker
power of F, encode / decode round trips, a second formulation of the decoder that recomputes every leaf's value from the
channel values and the earlier decisions, and the rules of records and flips."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import polar_truth as T                                # noqa: E402

CODES = T.test_codes()


@pytest.mark.parametrize("n", (1, 2, 3, 4, 5, 6))
def test_transform_is_the_kronecker_power(n):
    N = 1 << n
    Fk = np.array([[1]], np.int64)
    for _ in range(n):
        Fk = np.kron(np.array([[1, 0], [1, 1]], np.int64), Fk)
    u = np.random.default_rng(n).integers(0, 2, (40, N), dtype=np.uint8)
    u[0], u[1] = 0, 1
    assert T.transform(u).tobytes() == ((u.astype(np.int64) @ Fk) % 2).astype(np.uint8).tobytes()
    assert T.transform(np.eye(N, dtype=np.uint8)).tobytes() == Fk.astype(np.uint8).tobytes()
    assert T.transform(T.transform(u)).tobytes() == u.tobytes()                  # an involution


def test_the_literal_orders_and_masks():
    assert T.rank(3).tolist() == [7, 6, 5, 3, 4, 2, 1, 0]
    assert T.rank(4).tolist() == [15, 14, 13, 11, 7, 12, 10, 9, 6, 5, 3, 8, 4, 2, 1, 0]
    for n in range(3, 11):
        w = T.weights(n)
        assert len(set(w)) == 1 << n, "a tie among the weights"
        assert sorted(T.rank(n).tolist()) == list(range(1 << n))
        for K in (1, 2, (1 << n) // 2, (1 << n) - 1, 1 << n):
            m = T.mask(n, K)
            assert int(m.sum()) == K and set(np.flatnonzero(m).tolist()) == set(T.rank(n)[:K].tolist())
    assert T.Q == tuple(round(2 ** (r / 4) * 2 ** 32) for r in range(4))


@pytest.mark.parametrize("name", sorted(CODES))
def test_noise_free_round_trip(name):
    n, msk = CODES[name]
    K = int(msk.sum())
    F = 9
    bits = np.random.default_rng(K).integers(0, 256, F * K, dtype=np.uint8)
    coded = T.encode(msk, bits)
    assert coded.size == F << n and coded.max() <= 1
    got, rec = T.decode(msk, T.soft_of_bits(coded))
    assert got.tobytes() == (bits & 1).tobytes()
    back, rec2 = T.decode(msk, T.soft_of_bits(coded), flags=T.CODEWORD)
    assert back.tobytes() == coded.tobytes() and rec.tobytes() == rec2.tobytes()


def leaf_by_leaf(msk, soft, flip):
    """one codeword, straight from the recursion with no partial-sum arrays: the value of every leaf is recomputed from
    the channel values and the decisions made so far"""
    N = msk.size
    u = [0] * N

    def value(base, m, k):
        """input value k of the node that decides u[base .. base + m)"""
        if m == N:
            return int(soft[k])
        pbase = base & ~(2 * m - 1)
        a, b = value(pbase, 2 * m, k), value(pbase, 2 * m, k + m)
        if base == pbase:
            return int(np.sign(a) * np.sign(b)) * min(abs(a), abs(b))
        x1 = int(T.transform(np.array([u[pbase:pbase + m]], np.uint8))[0, k])
        return b - a if x1 else b + a

    leaves = []
    for i in range(N):
        L = value(i, 1, 0)
        if msk[i]:
            u[i] = int(L < 0) ^ int(i == flip)
            leaves.append((abs(L), i))
    return np.array(u, np.uint8), sorted(leaves)[:4]


@pytest.mark.parametrize("n", (3, 4, 5))
def test_the_restatement_equals_the_leaf_by_leaf_formulation(n):
    N = 1 << n
    rng = np.random.default_rng(100 + n)
    for msk in (T.mask(n, N // 2), T.mask(n, N), T.random_mask(n, max(N // 3, 1), n), T.random_mask(n, 1, n + 50)):
        F = 6
        soft = rng.integers(-128, 128, F * N).astype(np.int8)
        soft[:N] = -128
        soft[N:2 * N] = rng.integers(-1, 2, N)
        info = np.flatnonzero(msk)
        flip = np.array([T.NONE, info[0], info[-1], N, int(np.flatnonzero(msk == 0)[0]) if (msk == 0).any() else T.NONE, info[len(info) // 2]], np.uint32)
        bits, rec = T.decode(msk, soft, flip)
        word, rec_w = T.decode(msk, soft, flip, T.CODEWORD)
        assert rec.tobytes() == rec_w.tobytes()
        for c in range(F):
            u, leaves = leaf_by_leaf(msk, soft[c * N:(c + 1) * N], int(flip[c]))
            assert bits.reshape(F, -1)[c].tolist() == u[info].tolist(), (n, c)
            assert word.reshape(F, N)[c].tobytes() == T.transform(u[None, :])[0].tobytes(), (n, c)
            want_i = [i for _, i in leaves] + [T.NONE] * (4 - len(leaves))
            want_a = [a for a, _ in leaves] + [T.NONE] * (4 - len(leaves))
            assert rec["index"][c].tolist() == want_i and rec["abs"][c].tolist() == want_a, (n, c)


@pytest.mark.parametrize("name", sorted(CODES))
def test_records_and_flips(name):
    n, msk = CODES[name]
    N, K = 1 << n, int(msk.sum())
    F = 12
    rng = np.random.default_rng(N + K)
    soft = T.noisy_soft(rng, T.encode(msk, rng.integers(0, 2, F * K, dtype=np.uint8)), 0.9)
    bits, rec = T.decode(msk, soft)
    bits = bits.reshape(F, K)
    info = np.flatnonzero(msk)
    # sorted by (abs, index); slots beyond K empty in both fields
    for c in range(F):
        pairs = list(zip(rec["abs"][c].tolist(), rec["index"][c].tolist()))
        used = pairs[:min(K, 4)]
        assert used == sorted(used) and all(msk[i] for _, i in used) and len({i for _, i in used}) == len(used)
        assert pairs[min(K, 4):] == [(T.NONE, T.NONE)] * (4 - min(K, 4))
    # a flip at index[0] inverts exactly that leaf's rule: the decisions in front of it stay, its own is inverted, and the
    # leaf saw the same value
    flip = rec["index"][:, 0].copy()
    fbits, frec = T.decode(msk, soft, flip)
    fbits = fbits.reshape(F, K)
    for c in range(F):
        r = int(np.searchsorted(info, flip[c]))
        assert fbits[c, :r].tolist() == bits[c, :r].tolist() and fbits[c, r] == bits[c, r] ^ 1
        key = (int(rec["abs"][c][0]), int(flip[c]))                       # the leaf saw the same value as before
        seen = list(zip(frec["abs"][c].tolist(), frec["index"][c].tolist()))
        assert key in seen or key > max(seen)
    # a frozen position, NONE and a value >= N change nothing
    frozen = np.flatnonzero(msk == 0)
    for other in (np.full(F, T.NONE), np.full(F, N), np.full(F, N + 7), np.full(F, frozen[0] if frozen.size else T.NONE)):
        b2, r2 = T.decode(msk, soft, other.astype(np.uint32))
        assert b2.tobytes() == bits.tobytes() and r2.tobytes() == rec.tobytes()
