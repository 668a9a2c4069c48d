"""CPU: the host algebra of aeth_ldpc_generator against the restatement tests/ldpc_truth.py, and the restatement against
itself: H [u | P u] = 0, a singular parity part, noise-free codewords in one iteration, the vectorised decoder against
plain loops, and the noisy channel the definition was prototyped on."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from aether_primitives_amd import _lib, ldpc          # noqa: E402
import ldpc_truth as T                                # noqa: E402

CODES = T.test_codes()


@pytest.fixture(scope="module")
def generators():
    return {name: T.generator(*code) for name, code in CODES.items()}


@pytest.mark.parametrize("name", sorted(CODES))
def test_generator_equals_the_restatement_and_encodes_into_the_null_space(generators, name):
    shift, z = CODES[name]
    P = generators[name]
    rows, cols, N, M, K = T.dims(shift, z)
    assert P is not None and P.shape == (M, K)
    got = ldpc.generator(shift, z)
    assert got.shape == (M, K) and got.tobytes() == P.tobytes()
    rng = np.random.default_rng(z)
    u = rng.integers(0, 256, 5 * K, dtype=np.uint8)
    cw = T.encode(shift, z, u, P).reshape(5, N)
    assert cw[:, :K].tobytes() == (u & 1).tobytes()
    assert not ((cw.astype(np.int64) @ T.dense_h(shift, z).T.astype(np.int64)) & 1).any()


def test_a_singular_parity_part_is_refused():
    shift = ldpc.staircase(3, 6, 5)
    shift[2, 3:] = shift[1, 3:]                                        # two equal block rows in the parity part
    assert T.generator(shift, 5) is None
    with pytest.raises(_lib.AetherError) as e:
        ldpc.generator(shift, 5)
    assert e.value.code == _lib.E_ARG and "parity part singular" in str(e.value)
    shift = ldpc.staircase(2, 4, 4)
    shift[0, 3] = 0                                                    # [[I, I], [I, I]]
    assert T.generator(shift, 4) is None
    with pytest.raises(_lib.AetherError, match="parity part singular"):
        ldpc.generator(shift, 4)


@pytest.mark.parametrize("name", sorted(CODES))
def test_noise_free_codewords_decode_in_one_iteration(generators, name):
    shift, z = CODES[name]
    rows, cols, N, M, K = T.dims(shift, z)
    rng = np.random.default_rng(1)
    cw = T.encode(shift, z, rng.integers(0, 2, 3 * K, dtype=np.uint8), generators[name])
    for amp in (1, 20, 127):
        soft = (amp * (1 - 2 * cw.astype(np.int32))).astype(np.int8)
        bits, rec = T.decode(shift, z, soft, 20, T.EARLY)
        assert bits.tobytes() == cw.tobytes() and rec.tolist() == [[1, 0]] * 3, (name, amp)
    bits, rec = T.decode(shift, z, np.zeros(N, np.int8), 20, T.EARLY)
    assert not bits.any() and rec.tolist() == [[1, 0]]
    bits, rec = T.decode(shift, z, soft, 0, T.EARLY | T.PAYLOAD)
    assert bits.tobytes() == cw.reshape(3, N)[:, :K].tobytes() and rec.tolist() == [[0, 0]] * 3


@pytest.mark.parametrize("kind", ("ties", "uniform", "noisy"))
def test_vectorised_decoder_equals_plain_loops(generators, kind):
    shift, z = CODES["3x6x5"]
    rows, cols, N, M, K = T.dims(shift, z)
    rng = np.random.default_rng(3)
    F = 6
    if kind == "ties":
        soft = rng.integers(-1, 2, F * N).astype(np.int8)
    elif kind == "uniform":
        soft = rng.integers(-128, 128, F * N).astype(np.int8)
    else:
        soft = T.bpsk_soft(rng, T.encode(shift, z, rng.integers(0, 2, F * K, dtype=np.uint8), generators["3x6x5"]), 0.8)
    for max_iter, flags in ((0, 0), (1, 0), (7, T.EARLY), (7, 0), (50, T.EARLY | T.PAYLOAD)):
        bits, rec = T.decode(shift, z, soft, max_iter, flags)
        nb = K if flags & T.PAYLOAD else N
        for f in range(F):
            b, r = T.decode_scalar(shift, z, soft[f * N:(f + 1) * N], max_iter, flags)
            assert bits[f * nb:(f + 1) * nb].tobytes() == b.tobytes() and tuple(rec[f]) == r, (kind, max_iter, flags, f)


def test_the_prototype_channel(generators):
    """staircase(12, 24, 81), BPSK at sigma = 0.6, soft = rint(8 y / sigma^2) clamped: about 4.8 % raw errors, 20 of 20
    codewords within 5 iterations, max |Q| far below 2^15"""
    shift, z = CODES["12x24x81"]
    rows, cols, N, M, K = T.dims(shift, z)
    rng = np.random.default_rng(20)
    cw = T.encode(shift, z, rng.integers(0, 2, 20 * K, dtype=np.uint8), generators["12x24x81"])
    soft = T.bpsk_soft(rng, cw, 0.6)
    raw = np.mean((soft < 0) != cw)
    assert 0.03 < raw < 0.07, raw
    stats = {}
    bits, rec = T.decode(shift, z, soft, 20, T.EARLY, stats)
    print("raw error rate", raw, "iterations", rec[:, 0].tolist(), "max |Q|", stats["max_q"])
    assert bits.tobytes() == cw.tobytes() and not rec[:, 1].any() and rec[:, 0].max() <= 5
    assert stats["max_q"] <= 128 + 127 * rows
