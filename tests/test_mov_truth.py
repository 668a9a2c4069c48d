"""CPU: the numpy restatement of the moving-window detectors (tests/mov_truth.py) against math.fsum of every window's own
terms, and against closed forms.

Bounds.  A window sum is W terms added in SOME order from -0.0: at most W additions, each within 2^-53 relative of a
partial sum that never exceeds sum|t_j| over the window, and fsum's own rounding of the reference on top: taken twice,
W * 2^-52 * sum_window|t_j|.  A running sum that is differenced misses this by fifteen orders of magnitude behind the burst
of the input below (first third at 3e9, the rest at 1e-3); the fsum reference meets it trivially.
The metric M = |P|^2 / (R R'): |P| <= sqrt(R R') and sum|c_j| <= sqrt(R R') (Cauchy-Schwarz), so the relative error of each
window sum above moves M by at most a few W * 2^-52, and the rounding to f32 by 2^-24 relative: 2^-23 * M + 8 * W * 2^-52."""
import numpy as np
import pytest

import mov_truth as mt

EPS = 2.0 ** -52
SHAPES = ((1, 1, 50), (2, 1, 65), (16, 16, 400), (63, 5, 300), (64, 64, 700), (65, 1, 500), (144, 2048, 3000), (1000, 16, 4200),
          (4096, 64, 9000))


def burst_input(n, seed):
    """the first third scaled by 3e9, the rest by 1e-3"""
    r = np.random.default_rng(seed)
    x = r.standard_normal(n) + 1j * r.standard_normal(n)
    x[: n // 3] *= 3e9
    x[n // 3:] *= 1e-3
    return x.astype(np.complex64)


def abs_windows(t, W):
    return np.lib.stride_tricks.sliding_window_view(np.abs(t), W).sum(axis=1)


def fsum_sums(x, W, L, hist):
    """the four window sums by fsum, and the sums of the magnitudes of their terms"""
    n = len(x)
    H = mt.history(mt.LAG, W, L)
    xe = mt.extended(x, hist, H)
    e = mt.q(xe)
    c_re, c_im = mt.lag_terms(xe[L:], xe[:-L])
    R, _ = mt.fsum_windows(e, W)                         # R(i), i = -L .. n - 1
    out = {"p_re": mt.fsum_windows(c_re, W)[0], "p_im": mt.fsum_windows(c_im, W)[0], "r": R[L:], "r_lag": R[:n]}
    RA = abs_windows(e, W)
    mag = {"p_re": abs_windows(c_re, W), "p_im": abs_windows(c_im, W), "r": RA[L:], "r_lag": RA[:n]}
    return out, mag


@pytest.mark.parametrize("W,L,n", SHAPES)
def test_every_window_sum_is_its_own_terms_and_the_metric_follows(W, L, n):
    x = burst_input(n, 1000 + W)
    hist = burst_input(mt.history(mt.LAG, W, L), 7)[::-1].copy() if W % 2 else None
    got = mt.sums(x, mt.LAG, W, L, hist)
    want, mag = fsum_sums(x, W, L, hist)
    worst = 0.0
    for name in ("p_re", "p_im", "r", "r_lag"):
        err, bound = np.abs(got[name] - want[name]), W * EPS * mag[name]
        assert got[name].shape == (n,) and (err <= bound).all(), (name, float((err / np.maximum(bound, 1e-300)).max()))
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0)
    m = mt.metric(got, mt.LAG, W).astype(np.float64)
    den = want["r"] * want["r_lag"]
    m_ref = np.where(den == 0, 0.0, (want["p_re"] ** 2 + want["p_im"] ** 2) / np.where(den == 0, 1.0, den))
    err, bound = np.abs(m - m_ref), 2.0 ** -23 * m_ref + 8 * W * EPS
    assert (err <= bound).all(), float((err / bound).max())
    print(f"W={W} L={L} n={n}: sums within {worst:.3f} of the bound, metric within {float((err / bound).max()):.3f}")
    # the power kind: the same R, the mean over W
    p = mt.sums(x, mt.POWER, W, 0, None if hist is None else hist[L:])
    assert mt.same_bits(p["r"], got["r"])
    assert mt.same_bits(mt.metric(p, mt.POWER, W), (got["r"] / np.float64(W)).astype(np.float32))


def test_a_differenced_running_sum_would_miss_the_bound():
    """the scheme the order rules out, on the same input: behind the burst it keeps the burst's rounding error"""
    W, n = 64, 700
    e = mt.q(burst_input(n, 1064))
    cs = np.concatenate([[0.0], np.cumsum(e)])
    run = cs[W:] - cs[:-W]
    want, mag = mt.fsum_windows(e, W)
    assert (np.abs(run - want) > 1e6 * W * EPS * mag).any()
    got = mt.window_sums(e, W, 0)
    assert (np.abs(got - want) <= W * EPS * mag).all()


@pytest.mark.parametrize("W", (1, 2, 31, 32, 33, 64, 100, 1000, 4096))
def test_a_constant_gives_w_times_its_power(W):
    n = 2 * W + 37
    x = np.full(n, 3 - 2j, np.complex64)                 # q = 13: every partial sum is an integer below 2^53
    for kind, L in ((mt.POWER, 0), (mt.LAG, 5)):
        s = mt.sums(x, kind, W, L)
        i = np.arange(n)
        assert (s["r"] == 13.0 * np.minimum(i + 1, W)).all(), (W, kind)     # zero initial state: the window fills up
        if kind == mt.LAG:
            full = i >= W - 1 + L
            assert (s["p_re"][full] == 13.0 * W).all() and (s["p_im"] == 0).all()
            assert (mt.metric(s, kind, W)[full] == 1.0).all()
        else:
            assert (mt.metric(s, kind, W)[W - 1:] == np.float32(13.0)).all()


@pytest.mark.parametrize("W", (1, 16, 63, 144, 1000))
def test_a_repeated_half_gives_exactly_one(W):
    """L = W: x[j] == x[j - L] makes c_j = e_j term by term, and R(i - L) the same additions one segment back"""
    r = np.random.default_rng(W)
    half = (r.standard_normal(W) + 1j * r.standard_normal(W)).astype(np.complex64)
    x = np.concatenate([half, half, half])
    s = mt.sums(x, mt.LAG, W, W)
    m = mt.metric(s, mt.LAG, W)
    full = np.arange(x.size) >= 2 * W - 1
    assert mt.same_bits(s["p_re"][full], s["r"][full]) and (s["p_im"][full] == 0).all()
    assert (m[full] == 1.0).all() and (m <= 1.0).all()


def test_a_window_of_one_hands_out_each_term_with_the_sign_of_its_zero():
    v = np.array([0.0, -0.0, 1e-40, -1e-42, 1.0, 3e9, np.inf, -np.inf, np.nan], np.float32)
    x = np.empty(v.size ** 2, np.complex64)
    x.real, x.imag = np.repeat(v, v.size), np.tile(v, v.size)
    hist = np.array([-0.0 - 1j], np.complex64)
    xe = mt.extended(x, hist, 1)
    c_re, c_im = mt.lag_terms(xe[1:], xe[:-1])
    s = mt.sums(x, mt.LAG, 1, 1, hist)
    assert mt.same_bits(s["p_re"], c_re) and mt.same_bits(s["p_im"], c_im) and mt.same_bits(s["r"], mt.q(x))
    assert mt.same_bits(s["r_lag"], mt.q(xe[:-1]))
    assert np.signbit(c_im).any() and (c_im == 0).any()                    # there are zeros of both signs among them
    finite = np.isfinite(c_re) & np.isfinite(c_im) & (s["r"] * s["r_lag"] != 0) & np.isfinite(s["r"] * s["r_lag"])
    m = mt.metric(s, mt.LAG, 1)
    ok = finite & (s["r"] > 1e-30) & (s["r_lag"] > 1e-30) & (s["r"] < 1e30)
    assert np.allclose(m[ok], 1.0, rtol=2.0 ** -22)                        # |a conj b|^2 == |a|^2 |b|^2 up to rounding


@pytest.mark.parametrize("kind,W,L", ((mt.LAG, 16, 64), (mt.LAG, 144, 2048), (mt.LAG, 1, 3), (mt.POWER, 1000, 0), (mt.POWER, 33, 0)))
def test_a_cut_at_the_grid_continues_bit_for_bit(kind, W, L):
    n = 5 * W + 1234
    x = burst_input(n, 50 + W)
    H = mt.history(kind, W, L)
    whole = mt.planes(x, kind, W, L)
    for cut in sorted({W, 2 * W, (n - 1) // W * W}):     # the first one is shorter than the history of the lag kinds: zeros fill in
        hist = np.concatenate([np.zeros(max(H - cut, 0), np.complex64), x[max(cut - H, 0):cut]])
        a, b = mt.planes(x[:cut], kind, W, L), mt.planes(x[cut:], kind, W, L, hist)
        for j in range(3):
            if whole[j] is not None:
                assert mt.same_bits(np.concatenate([a[j], b[j]]), whole[j]), (cut, j)


def test_records_restate_the_candidate_rule():
    m = np.array([0.5, np.nan, 0.9, 0.9, 0.2, 0.95, 0.1], np.float32)
    s = {"p_re": np.arange(7.0), "p_im": -np.arange(7.0), "r": np.array([1, 1, 1, 1, 1, 0.01, 1.0]), "r_lag": np.ones(7)}
    rec = mt.records(m, s, mt.LAG, 7, 0, 0.5, 0.6)
    assert rec.size == 1 and rec[0]["index"] == 2 and rec[0]["first"] == 2 and rec[0]["n_nan"] == 1 and rec[0]["p_re"] == 2.0
    rec = mt.records(m, s, mt.LAG, 7, 2, 0.5, 0.6)
    assert list(rec["index"]) == [0, 2, 4, 6] and list(rec["first"]) == [7, 2, 7, 7]
    best = mt.fold_records(rec, 7)
    assert best["index"] == 2 and best["first"] == 2 and best["n_nan"] == 1
    none = mt.records(m, s, mt.LAG, 7, 0, 2.0, 0.0)
    assert none[0]["index"] == 7 and none[0]["first"] == 7 and np.isnan(none[0]["metric"]) and none[0]["r"] == 0.0
