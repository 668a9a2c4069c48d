"""CPU: the numpy restatement of the arbitrary-ratio resampler (tests/arb_truth.py) against an independent formulation
in complex128 (the polygon through the taps as a continuous impulse response, np.interp, the whole fraction) under the
bound of aeth_fft_exec and of the rational resampler (-120 dB, tests/test_gpu_fft.py); its chunks concatenating bit for
bit with carried phase and history; and its equality with the rational resampler's restatement where the step is
Q * 2^32 / L exactly."""
import numpy as np
import pytest

import arb_truth
import resamp_truth
from helpers import bits_equal, rand_c64

TOL_DB = -120.0                                   # tests/test_gpu_fft.py:20

# (b, P, step as a ratio, input samples)
SHAPES = [(5, 8, 0.731, 900), (6, 16, 0.91876, 900), (8, 16, 1.37, 900), (4, 4, 3.3, 900), (6, 16, 0.25001, 400),
          (0, 1, 1.0, 100), (12, 2, 2.0 ** -12, 5), (4, 3, 4096.0, 3 * 4096 + 5), (3, 64, 0.7, 300)]
IDS = [f"b{b}-P{p}-step{s:g}" for b, p, s, _ in SHAPES]
PHASES = (0, (1 << 32) - 1, 3 * (1 << 32) + 12345)


def word(ratio):
    return int(float(ratio) * 4294967296.0)


def taps_of(b, P):
    return np.random.default_rng(1000 * b + P).standard_normal(P << b).astype(np.float32)


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_restatement_against_complex128(shape):
    b, P, ratio, n = shape
    h, x = taps_of(b, P), rand_c64(7 * b + P, n)
    # a single tap at fraction 1 - 2^-32 makes outputs of h[0] * 2^-32 throughout: the 24 bits the weight keeps are an error
    # of 2^-24 |d| in absolute terms, which no bound relative to such an output can hold
    for phase in (PHASES if h.size > 1 else (PHASES[0], PHASES[2])):
        got = arb_truth.arb(h, b, x, word(ratio), phase)
        assert got.dtype == np.complex64 and got.size == arb_truth.advance(word(ratio), phase, n)[0] > 0
        want = arb_truth.arb_f64(h, b, x, word(ratio), phase)
        db = 20 * np.log10(np.linalg.norm(got.astype(np.complex128) - want) / np.linalg.norm(want))
        print(f"{IDS[SHAPES.index(shape)]} phase {phase}: {db:.1f} dB")
        assert db <= TOL_DB, (phase, db)


def history_at(x, cut, P):
    if cut < P - 1:
        return np.concatenate([np.zeros(P - 1 - cut, np.complex64), x[:cut]])
    return x[cut - (P - 1):cut]


CUTS = (0, 1, 7, 300, 301, 977, 1500)


@pytest.mark.parametrize("shape", SHAPES[:5] + [(4, 4, 64.3, 0), (0, 1, 1.0, 0)], ids=IDS[:5] + ["b4-P4-step64.3", "b0-P1-step1"])
@pytest.mark.parametrize("phase", PHASES[:2])
def test_chunks_with_carried_phase_concatenate_bit_for_bit(shape, phase):
    b, P, ratio, _ = shape
    n, step = 2000, word(ratio)
    h, x = taps_of(b, P), rand_c64(11 * b + P, n)
    whole = arb_truth.arb(h, b, x, step, phase)
    parts, ph, empty = [], phase, 0
    edges = CUTS + (n,)
    for lo, hi in zip((0,) + CUTS, edges):
        part = arb_truth.arb(h, b, x[lo:hi], step, ph, history_at(x, lo, P))
        count, ph = arb_truth.advance(step, ph, hi - lo)
        assert part.size == count
        empty += count == 0
        parts.append(part)
    assert empty >= 1                                               # the cut at 0 is a call over no samples
    assert bits_equal(np.concatenate(parts), whole), shape
    assert ph == arb_truth.advance(step, phase, n)[1]               # the phase after the chunks is the phase after the stream


def test_exact_rational_step_is_the_rational_resampler():
    b, Q, P = 3, 5, 8
    h, x = taps_of(b, P), rand_c64(3, 1000)
    step = Q * (1 << 32) // 8
    assert step * 8 == Q << 32
    got = arb_truth.arb(h, b, x, step)
    assert got.size == 1600
    assert bits_equal(got, resamp_truth.resamp(h, 8, Q, x))
    hist = rand_c64(4, P - 1)
    assert bits_equal(arb_truth.arb(h, b, x, step, 0, hist), resamp_truth.resamp(h, 8, Q, x, hist))


def test_the_largest_weight_reaches_the_zero_behind_the_last_tap():
    """phase 2^32 - 1: r = L - 1 and mu = 1 - 2^-24; with one tap per phase the tap is h[L - 1] (1 - mu) up to rounding"""
    b = 2
    h = np.array([1.0, 2.0, 3.0, 4.0], np.float32)
    out = arb_truth.arb(h, b, np.ones(1, np.complex64), 1 << 32, (1 << 32) - 1)
    mu = np.float32(1.0 - 2.0 ** -24)
    assert out.size == 1 and out.real[0] == np.float32(4.0) + mu * np.float32(-4.0)


def test_minus_zero_and_the_first_product():
    """the sum starts from the p = 0 product: -0.0 survives a single positive tap"""
    out = arb_truth.arb(np.array([1.0], np.float32), 0, np.array([complex(-0.0, -0.0)] * 3, np.complex64), 1 << 32)
    assert out.view(np.uint32).tolist() == [0x80000000] * 6
