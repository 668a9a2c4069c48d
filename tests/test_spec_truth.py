"""CPU: the numpy restatement of the averaged spectra (tests/spec_truth.py) against math.fsum, the order as part of the
contract, rows that concatenate, and the arithmetic of examples/psd.py."""
import math

import numpy as np
import pytest

import spec_truth
from aether_primitives_amd import chan

LEN = 16


@pytest.mark.parametrize("F", (1, 2, 7, 64, 1000))
@pytest.mark.parametrize("C", (1, 3, 8, 64))
def test_sums_are_within_the_sequential_bound_of_fsum(F, C):
    x = spec_truth.burst_then_noise(F * 131 + C, F, LEN)
    q = spec_truth.level_q(x).reshape(F, LEN)
    for B in (0, 1, C, C + 3, 2 * C):
        s, m = spec_truth.frame_sums(x, LEN, B, C)
        rows = spec_truth.rows_of(F, B)
        assert s.shape == m.shape == (len(rows), LEN)
        for r, (r0, r1) in enumerate(rows):
            for k in range(LEN):
                col = q[r0:r1, k].tolist()
                exact = math.fsum(col)
                # r1 - r0 - 1 additions of non-negative terms, each within 2^-53 of its result
                assert abs(s[r, k] - exact) <= (r1 - r0) * 2.0 ** -52 * exact, (F, C, B, r, k)
                assert m[r, k] == max(col)


def test_the_order_is_part_of_the_contract():
    """(b0 + b9) + b10 against b0 + (b9 + b10): frames 9 and 10 share a chunk of 8 that frame 0 is not in"""
    x = spec_truth.burst_then_noise(7, 1000, LEN)
    a, ma = spec_truth.frame_sums(x, LEN, 0, 64)
    b, mb = spec_truth.frame_sums(x, LEN, 0, 8)
    assert (a.view(np.uint64) != b.view(np.uint64)).any()
    assert np.allclose(a, b, rtol=1e-12, atol=0)
    assert (ma == mb).all()                                       # the max has no order


@pytest.mark.parametrize("B,C,cut", ((8, 3, 16), (5, 8, 35), (64, 64, 64), (1, 4, 7)))
def test_rows_concatenate_at_a_multiple_of_the_block(B, C, cut):
    F = 100
    x = spec_truth.burst_then_noise(B + C, F, LEN)
    s, m = spec_truth.frame_sums(x, LEN, B, C)
    s0, m0 = spec_truth.frame_sums(x[:cut * LEN], LEN, B, C)
    s1, m1 = spec_truth.frame_sums(x[cut * LEN:], LEN, B, C)
    assert spec_truth.same_plane(np.concatenate([s0, s1]), s) and spec_truth.same_plane(np.concatenate([m0, m1]), m)


def test_nan_and_inf():
    x = np.zeros((5, 3), np.complex64)
    x[:, 0] = np.nan
    x[2, 1] = np.inf
    x[1, 2], x[3, 2] = np.nan, 2.0
    s, m = spec_truth.frame_sums(x.reshape(-1), 3, 0, 2)
    assert np.isnan(s[0, 0]) and m[0, 0] == -np.inf              # a column of NaNs
    assert s[0, 1] == np.inf and m[0, 1] == np.inf
    assert np.isnan(s[0, 2]) and m[0, 2] == 4.0                   # the max skips the NaN


def test_the_example_arithmetic():
    """examples/psd.py: a tone of amplitude 0.05 on a bin under the periodic Hann window of 1024 shows a^2 (M / 2)^2 = 655
    over a noise level of 3 M / 8 = 384 per bin"""
    M, a = 1024, 0.05
    w = chan.prototype("hann", M, 1).astype(np.float64)
    assert abs(w.sum() - M / 2) < 1e-3 and abs((w ** 2).sum() - 3 * M / 8) < 1e-3
    n = np.arange(M)
    X = np.fft.fft(w * a * np.exp(2j * np.pi * 200 * n / M))
    assert abs(abs(X[200]) ** 2 - 655.36) < 0.01
    assert 384 * math.log(1024) > 2 * 655.36                      # one frame: the largest noise bin hides the tone
    assert 655.36 > 20 * 384 / math.sqrt(2048)                    # 2048 frames: far above the spread of the mean
