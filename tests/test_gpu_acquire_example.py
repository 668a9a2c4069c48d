"""examples/acquire.py end to end: timing, carrier frequency and carrier phase estimated on the device, no bit error.

  * zero bit errors, the 16 edge symbols on each side excluded;
  * each device estimate equals the estimate from the f64 restatement (tests/sync_truth.py, math.fsum) of the SAME device
    bytes: the sums within the record bound of tests/test_gpu_sync.py (n * 2^-52 * sum|t_i| per component), hence the
    angles within that bound divided by |S| and by 2 pi (plus 2^-52 turns for the two atan2 roundings), and the words
    derived from them within that angle scaled like the word, plus one unit of the word's last place (truncation);
  * planted against estimated timing and frequency agree within twice the worst error of a numpy restatement of the whole
    chain -- exact root-raised-cosine pulses, the timing offset in the pulse's argument, matched filter by np.convolve,
    the square-law line, an FFT-domain fractional shift to the symbol instants, the lag-1 sum of the fourth power -- run
    on the CPU over seeds 0 .. 19 at Es/N0 = 20 dB, 1024 symbols: worst timing error 0.012858 samples, worst frequency
    error 1.1362e-4 cycles per sample, no bit error in any seed.  The bounds below are twice those figures and were
    fixed before the example first ran on a device."""
import importlib.util
import math
import os

import numpy as np
import pytest

import sync_truth as st
from aether_primitives_amd import nco, sync

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 2.0 ** -52
WORST_TIMING, WORST_FREQ = 0.012858, 1.1362e-4            # the restatement's worst errors over 20 seeds (see above)


def angle_bound(rec, mag, j=0):
    """turns between the angle of a device record and the angle of its reference sum"""
    s = math.hypot(rec["re"][j], rec["im"][j])
    return float(rec["n"][j]) * EPS * (mag[j, 0] + mag[j, 1]) / s / (2 * math.pi) + EPS


def within_record_bound(dev, want, mag):
    nb = want["n"].astype(np.float64)
    assert (np.asarray(dev["n"]) == want["n"]).all()
    for j, name in enumerate(("re", "im")):
        assert (np.abs(np.asarray(dev[name]) - want[name]) <= nb * EPS * mag[:, j]).all(), name


def as_array(r):
    return np.array([(r.re, r.im, r.mass, r.n, r.n_nonfinite, 0)], st.RECORD_DTYPE)


def test_acquire_example_estimates_what_was_planted_and_decodes_every_bit(ctx):
    spec = importlib.util.spec_from_file_location("example_acquire", os.path.join(ROOT, "examples", "acquire.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    r = ex.main(keep=True)
    try:
        y, s, coarse = r["y"].to_host(), r["s"].to_host(), r["coarse"].to_host()
    finally:
        for k in ("y", "s", "coarse"):
            del r[k]
        r.pop("ctx").close()
    assert r["errors"] == 0

    # timing: the square-law line of the matched filter's output
    want, mag = st.records(*st.line_terms(y, st.SQUARE, (0, nco.word(-1.0 / ex.SPS), 0), 0), 0)
    within_record_bound(as_array(r["t_line"]), want, mag)
    turns = st.turns(want["re"][0], want["im"][0])
    b = angle_bound(want, mag)
    assert abs(sync.turns(r["t_line"]) - turns) <= b
    f = -turns - math.floor(-turns)
    assert abs(r["t_phase"] / 2.0 ** 32 - f * ex.SPS) <= b * ex.SPS + 2.0 ** -32
    print(f"timing {r['timing']:.5f} samples, restated from the device bytes {f * ex.SPS:.5f}, angle bound {b:.2e} turns")

    # carrier frequency: the lag-1 sum of the fourth power of the symbols
    t_re, t_im, wt, exists = st.lag_terms(s, 4, 1, None)
    want, mag = st.records(t_re, t_im, wt, 0, exists)
    within_record_bound(as_array(r["f_lag"]), want, mag)
    turns = st.turns(want["re"][0], want["im"][0])
    b = angle_bound(want, mag)
    assert abs(sync.turns(r["f_lag"]) - turns) <= b
    assert abs(ex.signed(r["f_step"]) - (-turns / 4)) <= b / 4 + 2.0 ** -52
    print(f"carrier {r['freq_lag']:.4e} cycles per sample, restated {turns / 4 / ex.SPS:.4e}, angle bound {b:.2e} turns")

    # carrier phase: the block sums of the fourth power
    want, mag = st.records(*st.line_terms(coarse, st.POW4), ex.BLOCK)
    assert want.size == 16 == r["blocks"].size
    within_record_bound(r["blocks"], want, mag)
    for j in range(want.size):
        assert abs(sync.turns(r["blocks"][j]) - st.turns(want["re"][j], want["im"][j])) <= angle_bound(want, mag, j), j

    # planted against estimated
    print(f"timing error {r['timing'] - ex.TIMING:+.5f} samples (bound {2 * WORST_TIMING}), frequency error of the lag sum "
          f"{r['freq_lag'] - ex.FREQ:+.3e}, after the phase fit {r['freq'] - ex.FREQ:+.3e} cycles per sample (bound {2 * WORST_FREQ})")
    assert abs(r["timing"] - ex.TIMING) <= 2 * WORST_TIMING
    assert abs(r["freq_lag"] - ex.FREQ) <= 2 * WORST_FREQ
