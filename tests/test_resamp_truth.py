"""CPU: the numpy restatement of the resampler (tests/resamp_truth.py) against an independent formulation in complex128
(zero stuffing, np.convolve, picking every Q-th sample) under the bound of aeth_fft_exec (-120 dB, tests/test_gpu_fft.py),
and its chunks concatenating bit for bit when the previous P - 1 samples are passed as history."""
import numpy as np
import pytest

import resamp_truth
from helpers import bits_equal, rand_c64

TOL_DB = -120.0                                   # tests/test_gpu_fft.py:20

# (U, Q, P, B): B periods of Q input samples
SHAPES = [(1, 1, 1, 100), (1, 1, 5, 300), (2, 1, 4, 300), (1, 2, 4, 300), (3, 2, 8, 200), (2, 3, 3, 200), (147, 160, 4, 9),
          (160, 147, 16, 9), (7, 5, 64, 300), (1, 64, 2, 100), (64, 1, 1, 100), (4096, 4095, 2, 1), (5, 4096, 3, 2)]
IDS = [f"U{u}-Q{q}-P{p}-B{b}" for u, q, p, b in SHAPES]


def taps_of(U, P):
    return np.random.default_rng(1000 * U + P).standard_normal(U * P).astype(np.float32)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_restatement_against_complex128(shape):
    U, Q, P, B = shape
    h, x = taps_of(U, P), rand_c64(U + 3 * Q + P, B * Q)
    got = resamp_truth.resamp(h, U, Q, x)
    assert got.dtype == np.complex64 and got.size == B * U
    want = resamp_truth.resamp_f64(h, U, Q, x)
    db = 20 * np.log10(np.linalg.norm(got.astype(np.complex128) - want) / np.linalg.norm(want))
    print(f"{IDS[SHAPES.index(shape)]}: {db:.1f} dB")
    assert db <= TOL_DB, db


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_chunks_with_history_concatenate_bit_for_bit(shape):
    U, Q, P, B = shape
    h, x = taps_of(U, P), rand_c64(U + 3 * Q + P + 1, B * Q)
    whole = resamp_truth.resamp(h, U, Q, x)
    splits = range(1, B) if B <= 20 else sorted({1, 2, B // 3, B // 2, B - 1})
    for b in splits:
        cut = b * Q
        if cut < P - 1:
            hist = np.concatenate([np.zeros(P - 1 - cut, np.complex64), x[:cut]])
        else:
            hist = x[cut - (P - 1):cut]
        parts = np.concatenate([resamp_truth.resamp(h, U, Q, x[:cut]), resamp_truth.resamp(h, U, Q, x[cut:], hist)])
        assert bits_equal(parts, whole), (shape, b)
    if B == 1:                                     # one period: an explicit history of zeros is the NULL history
        assert bits_equal(resamp_truth.resamp(h, U, Q, x, np.zeros(P - 1, np.complex64)), whole)


def test_minus_zero_and_the_first_product():
    """the sum starts from the p = 0 product: -0.0 survives a single positive tap"""
    out = resamp_truth.resamp(np.array([1.0], np.float32), 1, 1, np.array([complex(-0.0, -0.0)] * 3, np.complex64))
    assert out.view(np.uint32).tolist() == [0x80000000] * 6
