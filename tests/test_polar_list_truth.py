"""CPU: the restatement tests/polar_list_truth.py of the list decoder against what it can be checked with alone.

  1. `paths` (vectorised, levels gathered by parent) equals `plain_paths` (the definition, one path and one leaf at a
     time) for n <= 5, four kinds of input.
  2. L = 1 equals `polar_truth.decode` for the eight codes of `polar_truth.test_codes()`.
  3. every finished path's metric equals sum |soft_j| [x^_j != (soft_j < 0)] over its re-encoded codeword.
  4. with K = log2 L -- (3, 3) at L = 8, (6, 1) at L = 2 -- the list is every codeword and the metrics equal a brute-force
     enumeration, sorted.
  5. all-zero input: every metric is 0, so (metric, p, b) leaves every decision 0 but the last log2 L, which count the rows.
  6. a wholly frozen subtree adds sum |v_j| [v_j < 0] over the node's own values.
  7. a mask whose last position is frozen: the order behind the last information leaf is not the final one."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import polar_truth as T                                # noqa: E402
import polar_list_truth as LT                          # noqa: E402


def inputs(rng, msk, F):
    N, K = msk.size, int(msk.sum())
    return {"uniform": rng.integers(-128, 128, F * N).astype(np.int8), "ties": rng.integers(-1, 2, F * N).astype(np.int8),
            "zero": np.zeros(F * N, np.int8),
            "noisy": T.noisy_soft(rng, T.encode(msk, rng.integers(0, 2, F * K, dtype=np.uint8)), 0.9, 24.0)}


def frozen_last_mask():
    """a seeded random mask of n = 5 with position 31 frozen"""
    m = T.random_mask(5, 14, 531)
    m[31] = 0
    return m


@pytest.mark.parametrize("n,K,L", ((3, 3, 8), (3, 4, 2), (4, 8, 4), (5, 16, 8), (5, 16, 2), (5, None, 4)))
def test_vectorised_equals_the_definition(n, K, L):
    msk = T.mask(n, K) if K else frozen_last_mask()
    rng = np.random.default_rng(100 * n + L)
    for kind, s in inputs(rng, msk, 5).items():
        want = LT.plain_paths(msk, s, L)
        u, pm = LT.paths(msk, s, L)
        for f in range(5):
            assert (want[f][0] == u[f]).all() and (want[f][1] == pm[f]).all(), (kind, f)


@pytest.mark.parametrize("name", sorted(T.test_codes()))
def test_a_list_of_one_is_successive_cancellation(name):
    n, msk = T.test_codes()[name]
    rng = np.random.default_rng(n)
    for kind, s in inputs(rng, msk, 3).items():
        for flags in (0, T.CODEWORD):
            assert LT.decode(msk, s, 1, flags)[0].tobytes() == T.decode(msk, s, None, flags)[0].tobytes(), (kind, flags)
            assert LT.decode(msk, s, 1, flags | LT.ALL)[0].tobytes() == T.decode(msk, s, None, flags)[0].tobytes(), (kind, flags)


@pytest.mark.parametrize("name,L", (("3x4", 8), ("5x16", 4), ("7x64r", 8), ("9x171", 2), ("10x512", 8)))
def test_the_metric_is_the_codewords_distance(name, L):
    n, msk = T.test_codes()[name]
    N = 1 << n
    rng = np.random.default_rng(n + L)
    for kind, s in inputs(rng, msk, 3).items():
        u, pm = LT.paths(msk, s, L)
        word, rec = LT.decode(msk, s, L, LT.ALL | LT.CODEWORD)
        word = word.reshape(3, L, N)
        assert (word == T.transform(u.reshape(3 * L, N)).reshape(3, L, N)).all()
        for f in range(3):
            assert (LT.metric_of(s[f * N:(f + 1) * N], word[f]) == pm[f]).all(), (kind, f)
        assert (np.diff(pm, axis=1) >= 0).all() and (rec["metric"][:, :L] == pm).all() and (rec["metric"][:, L:] == LT.NONE).all()
        assert pm.max() <= 128 * N


@pytest.mark.parametrize("n,msk,L", ((3, T.mask(3, 3), 8), (6, T.test_codes()["6x1"][1], 2)))
def test_a_list_as_large_as_the_code_holds_every_codeword(n, msk, L):
    N, K = 1 << n, int(msk.sum())
    assert 1 << K == L
    every = np.array([[(w >> (K - 1 - r)) & 1 for r in range(K)] for w in range(L)], np.uint8)
    words = T.encode(msk, every.ravel()).reshape(L, N)
    rng = np.random.default_rng(n)
    for kind, s in inputs(rng, msk, 4).items():
        got, rec = LT.decode(msk, s, L, LT.ALL | LT.CODEWORD)
        got = got.reshape(4, L, N)
        for f in range(4):
            assert len({r.tobytes() for r in got[f]}) == L, (kind, f)
            brute = LT.metric_of(s[f * N:(f + 1) * N], words)
            assert sorted(brute.tolist()) == rec["metric"][f, :L].tolist(), (kind, f)
            assert (LT.metric_of(s[f * N:(f + 1) * N], got[f]) == rec["metric"][f, :L]).all()


@pytest.mark.parametrize("name,L", (("3x4", 4), ("5x16", 8), ("7x64r", 2), ("3x8", 8)))
def test_zero_input_is_ordered_by_position_and_bit(name, L):
    n, msk = T.test_codes()[name]
    K = int(msk.sum())
    bits, rec = LT.decode(msk, np.zeros(2 << n, np.int8), L, LT.ALL)
    bits = bits.reshape(2, L, K)
    lg = L.bit_length() - 1
    assert (rec["metric"][:, :L] == 0).all()
    for r in range(L):
        want = np.zeros(K, np.uint8)
        want[K - lg:] = [(r >> (lg - 1 - c)) & 1 for c in range(lg)]
        assert (bits[:, r] == want).all(), r


def node_values(y, u, base, m):
    """the values of the node (base, m) of one codeword under the decisions u[0..base)"""
    def rec(Lv, b0, mm):
        if mm == m:
            return Lv
        h = mm // 2
        a, b = Lv[:h], Lv[h:]
        if base < b0 + h:
            return rec(T.f_of(a, b), b0, h)
        x1 = T.transform(u[None, b0:b0 + h])[0]
        return rec(np.where(x1 == 0, b + a, b - a), b0 + h, h)
    return rec(y.astype(np.int64), 0, y.size)


@pytest.mark.parametrize("name", ("5x16", "7x64r", "9x171"))
def test_a_frozen_subtree_adds_its_nodes_negative_values(name):
    n, msk = T.test_codes()[name]
    N = 1 << n
    rng = np.random.default_rng(7 * n)
    blocks = [(b, m) for m in (2, 4, 8, 16, 32) for b in range(0, N, m) if not msk[b:b + m].any()]
    assert blocks
    for kind, s in inputs(rng, msk, 2).items():
        trace = []
        u, pm = LT.paths(msk, s, 1, trace)
        for f in range(2):
            for b, m in blocks:
                v = node_values(s[f * N:(f + 1) * N], u[f, 0], b, m)
                before = trace[b - 1][f, 0] if b else 0
                assert trace[b + m - 1][f, 0] - before == int(np.where(v < 0, -v, 0).sum()), (kind, f, b, m)
    # with four paths: a leading frozen block, in front of the first fork
    first = int(np.flatnonzero(msk)[0])
    m = 1 << (first.bit_length() - 1) if first else 0
    if m:
        s = inputs(rng, msk, 2)["uniform"]
        trace = []
        LT.paths(msk, s, 4, trace)
        for f in range(2):
            v = node_values(s[f * N:(f + 1) * N], np.zeros(N, np.uint8), 0, m)
            assert trace[m - 1][f, 0] == int(np.where(v < 0, -v, 0).sum())


def test_trailing_frozen_leaves_need_the_final_sort():
    msk = frozen_last_mask()
    assert msk[31] == 0 and msk.sum() >= 2
    rng = np.random.default_rng(31)
    s = rng.integers(-128, 128, 64 * 32).astype(np.int8)
    trace = []
    u, pm = LT.paths(msk, s, 4, trace)
    assert (np.diff(pm, axis=1) >= 0).all()
    unsorted = (np.diff(trace[-1], axis=1) < 0).any(axis=1)
    assert unsorted.any(), "no codeword of this input whose order the trailing frozen leaves change"
    want = LT.plain_paths(msk, s[:8 * 32], 4)
    for f in range(8):
        assert (want[f][0] == u[f]).all() and (want[f][1] == pm[f]).all()


def test_pick_restated():
    rows = np.arange(3 * 4 * 2, dtype=np.uint8)
    diff = np.array([5, 0, 0, 1, 7, 7, 7, 7, 0, 1, 1, 0], np.uint64)
    out, which = LT.pick(rows, 2, 4, diff)
    assert which.tolist() == [1, LT.NONE, 0] and out.tolist() == [[2, 3], [8, 9], [16, 17]]
