"""CPU: the numpy restatement the convolutional-code tests compare with (tests/cc_truth.py) against independent plain
loops: the encoder against a shift register, the K = 7 impulse response, the decoder with one block and no warm-up or
traceback against a textbook Viterbi, chunked calls against one call, and noise-free hard decisions decoding exactly."""
import numpy as np
import pytest

import cc_truth
from cc_truth import SMALL_SHAPES


def shift_register(k, polys, bits, hist=None):
    reg = 0
    for b in ([0] * (k - 1) if hist is None else list(hist)):
        reg = (reg >> 1) | ((int(b) & 1) << (k - 1))
    out = []
    for b in bits:
        reg = (reg >> 1) | ((int(b) & 1) << (k - 1))              # the current bit at the MSB
        out += [bin(reg & p).count("1") & 1 for p in polys]
    return np.array(out, np.uint8)


def textbook_viterbi(k, polys, soft):
    """one window over the whole call, all metrics 0 at the start, forward formulation, plain loops"""
    n, S = len(polys), 1 << (k - 1)
    N = len(soft) // n
    m = [0] * S
    prev = []
    for t in range(N):
        v = [int(x) for x in soft[n * t:n * t + n]]
        new, back = [None] * S, [0] * S
        for s in range(S):                                         # ascending: of two equal candidates the smaller predecessor stays
            for u in (0, 1):
                reg = (u << (k - 1)) | s
                cand = m[s] + sum((1 - 2 * (bin(reg & p).count("1") & 1)) * v[q] for q, p in enumerate(polys))
                ns = (u << (k - 2)) | (s >> 1)
                if new[ns] is None or cand > new[ns]:
                    new[ns], back[ns] = cand, s
        m = new
        prev.append(back)
    s = max(range(S), key=lambda x: (m[x], -x))
    out = np.zeros(N, np.uint8)
    for t in range(N - 1, -1, -1):
        out[t] = s >> (k - 2)
        s = prev[t][s]
    return out


@pytest.mark.parametrize("k,polys", [(s[0], s[1]) for s in SMALL_SHAPES])
def test_encoder_equals_a_shift_register(k, polys):
    rng = np.random.default_rng(k)
    bits = rng.integers(0, 256, 301).astype(np.uint8)              # bytes are taken & 1
    hist = rng.integers(0, 2, k - 1).astype(np.uint8)
    assert (cc_truth.encode(k, polys, bits) == shift_register(k, polys, bits)).all()
    assert (cc_truth.encode(k, polys, bits, hist) == shift_register(k, polys, bits, hist)).all()
    whole = cc_truth.encode(k, polys, bits, hist)                  # chunks concatenate
    cut = 77
    two = np.concatenate([cc_truth.encode(k, polys, bits[:cut], hist), cc_truth.encode(k, polys, bits[cut:], bits[cut - (k - 1):cut])])
    assert (two == whole).all()


def test_k7_impulse_response():
    c = cc_truth.encode(7, (0o171, 0o133), [1, 0, 0, 0, 0, 0, 0]).reshape(7, 2)
    assert "".join(map(str, c[:, 0])) == "1111001" and "".join(map(str, c[:, 1])) == "1011011"


@pytest.mark.parametrize("k,polys", [(s[0], s[1]) for s in SMALL_SHAPES])
@pytest.mark.parametrize("kind", ("ties", "uniform"))
def test_one_block_decoder_equals_textbook_viterbi(k, polys, kind):
    rng = np.random.default_rng(100 + k)
    N, n = 150, len(polys)
    soft = (rng.integers(-1, 2, N * n) if kind == "ties" else rng.integers(-128, 128, N * n)).astype(np.int8)
    assert (cc_truth.decode(k, polys, N, 0, 0, soft) == textbook_viterbi(k, polys, soft)).all()


@pytest.mark.parametrize("k,polys,D,A,T", SMALL_SHAPES)
def test_chunked_equals_one_call(k, polys, D, A, T):
    rng = np.random.default_rng(7)
    n, N = len(polys), 5 * D + 3
    soft = rng.integers(-128, 128, N * n).astype(np.int8)
    hist = rng.integers(-128, 128, (A + T) * n).astype(np.int8)
    whole = cc_truth.decode(k, polys, D, A, T, soft, hist)
    for cut in (D, 3 * D):                                         # the first call's N is a multiple of D
        ext = np.concatenate([hist, soft])
        h2 = ext[cut * n:(cut + A + T) * n]                        # the last A + T steps before step `cut`
        two = np.concatenate([cc_truth.decode(k, polys, D, A, T, soft[:cut * n], hist), cc_truth.decode(k, polys, D, A, T, soft[cut * n:], h2)])
        assert (two == whole).all(), cut


@pytest.mark.parametrize("k,polys,D,A,T", SMALL_SHAPES)
def test_noise_free_hard_decisions_decode_exactly(k, polys, D, A, T):
    rng = np.random.default_rng(11)
    bits = rng.integers(0, 2, 5 * D + 3).astype(np.uint8)
    soft = (1 - 2 * cc_truth.encode(k, polys, bits).astype(np.int8)).astype(np.int8)
    assert (cc_truth.decode_stream(k, polys, D, A, T, soft) == bits).all()


def test_soft_demodulator_restatement_on_known_points():
    qpsk = np.array([1 + 1j, -1 + 1j, 1 - 1j, -1 - 1j], np.complex64)
    sym = np.array([1 + 1j, -1 - 1j, 0.25 - 0.5j, complex(np.nan, 0), complex(np.inf, 1), 100 + 100j], np.complex64)
    got = cc_truth.demod_soft(qpsk, sym, 8.0).reshape(-1, 2)
    # d2 differences are 4 re and 4 im: L = 32 re, 32 im; a NaN or infinite distance leaves Inf - Inf = NaN -> 0
    assert got.tolist() == [[32, 32], [-32, -32], [8, -16], [0, 0], [0, 0], [127, 127]]
