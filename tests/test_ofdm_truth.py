"""CPU: the numpy restatement of the OFDM calls (tests/ofdm_truth.py) against closed forms, so that the GPU tests compare
the kernels with something that is itself checked.  The signs are the library's (`Fft::fwd` = +j): ofdm_truth.py says what
that does to the textbook equations."""
import numpy as np
import pytest

import aether_primitives_amd  # noqa: F401  (the package the restatement describes: without its Ofdm there is nothing to check)
from aether_primitives_amd.ofdm import EQ_KINDS

import ofdm_truth as ot

N, G = 64, 16
BINS = np.array(list(range(N - 26, N)) + list(range(1, 27)))          # -26 .. -1, 1 .. 26
K = len(BINS)


def carriers(seed, n_sym, k=K):
    r = np.random.default_rng(seed)
    return r.standard_normal((n_sym, k)) + 1j * r.standard_normal((n_sym, k))


def through(taps, x):
    """the channel: y[n] = sum_t taps[t] x[n - t], zeros in front"""
    return np.convolve(x, taps)[:len(x)]


def test_kinds_agree_with_the_package():
    assert (ot.ZF, ot.MMSE, ot.MATCHED) == (EQ_KINDS["zf"], EQ_KINDS["mmse"], EQ_KINDS["matched"])


@pytest.mark.parametrize("n_fft,cp,bins", [(N, G, BINS), (N, 0, np.arange(N)), (12, 5, np.array([3, 0, 11])), (256, 256, np.array([7]))])
def test_demod_of_mod_returns_the_carriers(n_fft, cp, bins):
    X = carriers(1, 5, len(bins))
    t = ot.mod_truth(X, n_fft, cp, bins, 5, scale=1.0 / n_fft)
    assert t.shape == (5 * (n_fft + cp),)
    got = ot.demod_truth(t[cp:], n_fft, cp, bins, 5)
    assert np.max(np.abs(got - X)) < 1e-12


def test_prefix_is_the_tail_of_the_symbol_and_unoccupied_bins_are_zero():
    X = carriers(2, 3)
    t = ot.mod_truth(X, N, G, BINS, 3).reshape(3, N + G)
    assert np.array_equal(t[:, :G], t[:, N:])
    full = ot.fwd(t[:, G:]) / N
    off = np.setdiff1d(np.arange(N), BINS)
    assert np.max(np.abs(full[:, off])) < 1e-12


@pytest.mark.parametrize("a", [0, 4, G])
def test_channel_inside_the_prefix_is_one_tap_per_carrier(a):
    ntaps = G + 1 - a
    r = np.random.default_rng(3)
    taps = (r.standard_normal(ntaps) + 1j * r.standard_normal(ntaps)) / ntaps
    X = carriers(4, 6)
    rx = through(taps, ot.mod_truth(X, N, G, BINS, 6, scale=1.0 / N))
    got = ot.demod_truth(rx[G - a:], N, G, BINS, 6)
    want = X * (ot.channel_response(taps, N) * ot.advance_ramp(N, a))[BINS][None, :]
    # symbol 0 has zeros, not a previous symbol, in front: the equation holds for it all the same (its prefix is its own)
    assert np.max(np.abs(got - want)) < 1e-12
    # ... and one tap more reaches into the previous symbol: the test sees the prefix
    long = np.concatenate([taps, [0.5]])
    rx = through(long, ot.mod_truth(X, N, G, BINS, 6, scale=1.0 / N))
    got = ot.demod_truth(rx[G - a:], N, G, BINS, 6)
    want = X * (ot.channel_response(long, N) * ot.advance_ramp(N, a))[BINS][None, :]
    assert np.max(np.abs(got[1:] - want[1:])) > 1e-6


@pytest.mark.parametrize("x_sym", [1, 4])
def test_estimate_of_a_noise_free_channel(x_sym):
    r = np.random.default_rng(5)
    H = (r.standard_normal(K) + 1j * r.standard_normal(K)).astype(np.complex64)
    X = carriers(6, x_sym).astype(np.complex64)
    X[:, 7] = 0                                              # a carrier without training
    Y = (np.broadcast_to(X, (4, K)) * H[None, :]).astype(np.complex64)
    eps = np.finfo(np.float32).eps
    h, w, csi = ot.estimate_truth(Y, X, 4, x_sym, K, 0.0, ot.ZF)
    assert h.dtype == np.complex64 and w.dtype == np.complex64 and csi.dtype == np.float32
    live = np.arange(K) != 7
    # Y is H X rounded to f32 (two roundings per component) and H is rounded once more
    assert np.max(np.abs(h[live] - H[live]) / np.abs(H[live])) < 4 * eps
    assert np.max(np.abs(w[live].astype(np.complex128) * H[live] - 1)) < 8 * eps
    assert np.allclose(csi[live], np.abs(H[live]) ** 2, rtol=8 * eps)
    assert h[7] == 0 and w[7] == 0 and csi[7] == 0
    hm, wm, _ = ot.estimate_truth(Y, X, 4, x_sym, K, 0.0, ot.MATCHED)
    assert np.array_equal(hm.view(np.uint32), h.view(np.uint32))
    assert np.array_equal(wm.view(np.uint32), np.conj(hm).view(np.uint32))
    assert hm[7] == 0 and wm[7] == 0
    _, wn, _ = ot.estimate_truth(Y, X, 4, x_sym, K, 0.1, ot.MMSE)
    want = np.conj(H[live].astype(np.complex128)) / (np.abs(H[live].astype(np.complex128)) ** 2 + np.float64(np.float32(0.1)))
    assert np.max(np.abs(wn[live] - want) / np.abs(want)) < 8 * eps
    assert wn[7] == 0                                        # conj(0) / 0.1


def test_estimate_with_zero_noise_variance_and_no_training_gives_zero_not_nan():
    X = np.zeros((1, 3), np.complex64)
    Y = np.ones((2, 3), np.complex64)
    for kind in (ot.ZF, ot.MMSE, ot.MATCHED):
        h, w, csi = ot.estimate_truth(Y, X, 2, 1, 3, 0.0, kind)
        assert not np.isnan(h).any() and not np.isnan(w).any() and (csi == 0).all()
        assert (h == 0).all() and (w == 0).all()
