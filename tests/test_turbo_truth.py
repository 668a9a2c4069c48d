"""CPU: the restatement tests/turbo_truth.py against the definition's own consequences -- the full-window pass is the
brute-force max over all terminated paths, a warm-up of K steps is the full window, the vectorised pass is the plain one,
encoders end in state 0, noise-free codewords decode to themselves, the QPP pairs, and the int32 bound."""
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import turbo_truth as T                                # noqa: E402

QPP_PAIRS = ((40, 3, 10), (64, 7, 16), (128, 15, 32), (512, 31, 64), (1024, 31, 64), (6144, 263, 480))


def int8_inputs(rng, n):
    v = rng.integers(-128, 128, n).astype(np.int64)
    v[rng.integers(0, n)] = -128
    v[rng.integers(0, n)] = 127
    return v


def brute(code, x, p, K):
    """D[t] = max over all input sequences of K + nu steps that end in state 0 with u[t] = 0, minus the same with u[t] = 1"""
    best = [[None, None] for _ in range(K)]
    for seq in itertools.product((0, 1), repeat=K + code.nu):
        s, m = 0, 0
        for t, u in enumerate(seq):
            m += (1 - 2 * u) * int(x[t]) + (1 - 2 * int(code.z[s, u])) * int(p[t])
            s = int(code.nxt[s, u])
        if s:
            continue
        for t in range(K):
            b = best[t]
            b[seq[t]] = m if b[seq[t]] is None else max(b[seq[t]], m)
    return [b[0] - b[1] for b in best]


@pytest.mark.parametrize("name", ("k3", "lte", "ccsds"))
def test_full_window_is_the_brute_force_max(name):
    code, K = T.named(name), 8
    rng = np.random.default_rng(code.k)
    for _ in range(3):
        x, p = int8_inputs(rng, K + code.nu), int8_inputs(rng, K + code.nu)
        want = brute(code, x, p, K)
        assert T.siso_plain(code, x, p, K, K, 0) == want
        assert T.siso(code, x[None, :], p[None, :], K, K, 0)[0].tolist() == want


@pytest.mark.parametrize("name", ("k3", "lte", "ccsds"))
def test_warm_up_of_k_steps_is_the_full_window_and_vectorised_is_plain(name):
    code = T.named(name)
    rng = np.random.default_rng(10 + code.k)
    for K in (8, 37, 40):
        x = np.stack([int8_inputs(rng, K + code.nu) for _ in range(3)])
        p = np.stack([int8_inputs(rng, K + code.nu) for _ in range(3)])
        x[:, :K] += rng.integers(-2047, 2048, (3, K))                      # with an a-priori of full size
        full = T.siso(code, x, p, K, K, 0)
        for W in (1, 3, 8, K - 1, K, K + 5):
            assert (T.siso(code, x, p, K, W, K) == full).all(), (K, W)
            assert (T.siso(code, x, p, K, W, K + 3) == full).all(), (K, W)
        for W, A in ((5, 3), (16, 8), (8, 0), (1, 0), (1, 1), (7, 40), (K, 0), (3, 100)):
            got = T.siso(code, x, p, K, W, A)
            for f in range(3):
                assert got[f].tolist() == T.siso_plain(code, x[f], p[f], K, W, A), (K, W, A, f)


@pytest.mark.parametrize("name", ("k3", "lte", "ccsds"))
def test_encoder_ends_in_state_zero_and_clean_codewords_decode_in_one_iteration(name):
    code = T.named(name)
    rng = np.random.default_rng(20 + code.k)
    for K, f1, f2 in ((40, 3, 10), (64, 7, 16)):
        pi = T.qpp(K, f1, f2)
        u = rng.integers(0, 256, 5 * K, dtype=np.uint8)
        coded = T.encode(code, pi, u)                                      # rsc() asserts the final state
        assert coded.size == 5 * (3 * K + 4 * code.nu) and coded.max() <= 1
        assert (coded.reshape(5, -1)[:, :K].ravel() == (u & 1)).all()
        for W, A in ((K, 0), (16, 8), (8, 0)):
            for level in (127, 1):
                bits, rec = T.decode(code, pi, W, A, T.soft_of_bits(coded, level), 1)
                assert bits.tobytes() == (u & 1).tobytes(), (K, W, A, level)
                assert (rec["iterations"] == 1).all() and (rec["disagreements"] == 0).all()


@pytest.mark.parametrize("K,f1,f2", QPP_PAIRS)
def test_qpp_pairs_are_permutations(K, f1, f2):
    pi = T.qpp(K, f1, f2)
    assert pi is not None and sorted(pi.tolist()) == list(range(K))
    i = np.arange(K, dtype=object)
    assert pi.tolist() == [int(v) for v in (f1 * i + f2 * i * i) % K]


def test_qpp_refuses_a_pair_that_is_no_permutation():
    assert T.qpp(40, 2, 10) is None


@pytest.mark.parametrize("name", ("k3", "lte", "ccsds"))
def test_all_zero_input(name):
    code, K = T.named(name), 40
    pi = T.qpp(K, 3, 10)
    N = 3 * K + 4 * code.nu
    bits, rec = T.decode(code, pi, 16, 8, np.zeros(3 * N, np.int8), 8, T.EARLY)
    assert not bits.any() and rec["iterations"].tolist() == [1] * 3 and rec["disagreements"].tolist() == [0] * 3
    bits, rec = T.decode(code, pi, 16, 8, np.zeros(3 * N, np.int8), 8)
    assert not bits.any() and rec["iterations"].tolist() == [8] * 3 and rec["disagreements"].tolist() == [0] * 3


def test_early_stop_is_per_codeword():
    code, K = T.named("lte"), 40
    pi = T.qpp(K, 3, 10)
    rng = np.random.default_rng(7)
    coded = T.encode(code, pi, rng.integers(0, 2, 6 * K, dtype=np.uint8))
    soft = T.noisy_soft(rng, coded, 1.0)
    bits, rec = T.decode(code, pi, 16, 8, soft, 8, T.EARLY)
    assert len(set(rec["iterations"].tolist())) > 1, rec
    for f in range(6):
        one = T.decode(code, pi, 16, 8, soft.reshape(6, -1)[f], int(rec["iterations"][f]))
        assert one[0].tobytes() == bits.reshape(6, -1)[f].tobytes() and one[1][0] == rec[f]


def test_a_history_gives_every_shorter_run():
    code, K = T.named("lte"), 40
    pi = T.qpp(K, 3, 10)
    rng = np.random.default_rng(8)
    soft = T.noisy_soft(rng, T.encode(code, pi, rng.integers(0, 2, 9 * K, dtype=np.uint8)), 1.0)
    history = []
    T.decode(code, pi, 16, 8, soft, 8, 0, None, history)
    for max_iter in (1, 2, 5, 8):
        for flags in (0, T.EARLY):
            want = T.decode(code, pi, 16, 8, soft, max_iter, flags)
            got = T.from_history(history, max_iter, flags)
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (max_iter, flags)


@pytest.mark.parametrize("name,W,A,iters", (("lte", 32, 32, 64), ("ccsds", 64, 64, 64), ("ccsds", 8192, 0, 4)))
def test_nothing_leaves_int32_at_the_largest_frame(name, W, A, iters):
    """all -128 at K = 8192: through 64 iterations with windows, and through 4 with the full window, whose paths are the
    longest (a full-window iteration costs a second here).  The restatement computes in int64 and records the range."""
    code, K = T.named(name), 8192
    pi = T.qpp(K, 31, 64)
    assert pi is not None
    soft = np.full(3 * K + 4 * code.nu, -128, np.int8)
    seen = T.Range()
    bits, rec = T.decode(code, pi, W, A, soft, iters, 0, seen)
    assert rec["iterations"][0] == iters
    assert -(1 << 31) <= seen.lo and seen.hi < (1 << 31), (seen.lo, seen.hi)
    print(name, W, A, "range", seen.lo, seen.hi)
