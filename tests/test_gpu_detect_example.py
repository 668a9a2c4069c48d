"""examples/detect.py end to end: a coded OFDM burst at a start the receiver is not told, behind noise, found by the
moving-window metric, its carrier offset taken from the lag sum at the peak, decoded on the device.

  * no decoded bit error;
  * the start found lies inside the part of the cyclic prefix the channel has left clean: at most G - (taps - 1) samples in
    front of the planted first sample of the repeated symbol, and not behind it;
  * start and carrier offset within twice the worst error of the restatement.

The figures come from `restate` below: a numpy restatement of the SAME chain -- the same constants (imported from the
example), the encoder, QPSK and Viterbi decoder of tests/test_gpu_ofdm_example.py, tests/ofdm_truth.py for the symbols,
np.convolve for the channel and for the window sums, the metric, the gate, the peak, the crossing at 0.9 of the peak, the
prefix sums, the f64 estimate -- run on the CPU (`python tests/test_gpu_detect_example.py`) over seeds 0 .. 19 at the
example's noise level.  The restatement's figures:
    decoded bit errors      0 in every seed
    start - target          the target is the middle of the clean prefix, planted - (G - (taps - 1)) / 2 = planted - 7 (the
                            metric climbs through 0.9 of its peak four to five samples in front of the plateau, which
                            the channel's taps round off; AHEAD = 11 puts the window there); worst |error| 1 sample
    coarse offset error     worst 2.9608e-4 cycles per sample (the repeated halves alone: 32 terms)
    offset error            worst 4.6544e-5 cycles per sample (with the prefixes)
They were fixed before the example first ran on a device.  `test_restatement_*` re-runs three of the seeds on the CPU so
that the figures cannot drift away from the code."""
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if __name__ == "__main__":
    sys.path[:0] = [ROOT, HERE]

import ofdm_truth as ot                               # noqa: E402
from test_gpu_ofdm_example import encode, viterbi     # noqa: E402  (the restated encoder and decoder)

WORST_START, WORST_COARSE, WORST_FREQ = 1, 2.9608e-4, 4.6544e-5      # the restatement over seeds 0 .. 19 (see above)


def example():
    spec = importlib.util.spec_from_file_location("example_detect", os.path.join(ROOT, "examples", "detect.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    return ex


def expected_start(ex):
    """the middle of the part of the prefix the channel has left clean"""
    return ex.START + ex.G - (ex.G - (ex.TAPS.size - 1)) // 2


def window_metric(x, W, L, r_min):
    """P, R, R(i - L), M and the candidates of the lag kind with zero initial state, in plain f64"""
    n = x.size
    xl = np.concatenate([np.zeros(L, complex), x[:n - L]]) if L < n else np.zeros(n, complex)
    box = np.ones(W)
    P = np.convolve(x * np.conj(xl), box)[:n]
    R = np.convolve(np.abs(x) ** 2, box)[:n]
    Rl = np.concatenate([np.zeros(L), R[:n - L]]) if L < n else np.zeros(n)
    den = R * Rl
    M = np.where(den > 0, np.abs(P) ** 2 / np.where(den > 0, den, 1.0), 0.0).astype(np.float32)
    return P, M, (R >= r_min) & (Rl >= r_min)


def restate(ex, seed):
    """the example's chain in numpy -> (decoded errors, start, coarse offset, offset)"""
    N, G, K, L, n_sym = ex.N, ex.G, ex.K, ex.N + ex.G, 1 + ex.N_TRAIN + ex.N_DATA
    r = np.random.default_rng(seed)
    bits = r.integers(0, 2, ex.NBITS, dtype=np.uint8)
    bits[-ex.TAIL:] = 0
    coded = encode(bits, ex.POLYS)
    table = np.array([1 + 1j, -1 + 1j, 1 - 1j, -1 - 1j])
    data = table[(coded[1::2].astype(int) << 1) + coded[0::2]]
    train = ex.training_symbol().astype(np.complex128)
    car = np.concatenate([ex.repeated_symbol().astype(np.complex128), np.tile(train, ex.N_TRAIN), data])
    tx = ot.mod_truth(car, N, G, ex.BINS, n_sym, 1 / np.sqrt(N))
    capture = np.zeros(ex.START + tx.size + ex.REST, complex)
    capture[ex.START:ex.START + tx.size] = tx
    rx = np.convolve(capture, ex.TAPS.astype(np.complex128))[: capture.size]
    rx = rx * np.exp(2j * np.pi * (ex.FREQ * np.arange(rx.size) + ex.PHASE))
    rx = rx + ex.NOISE_POWER * (r.standard_normal(rx.size) + 1j * r.standard_normal(rx.size))
    # the burst and its coarse offset
    P, M, cand = window_metric(rx, ex.HALF, ex.HALF, ex.R_MIN)
    idx = np.flatnonzero(cand)
    peak = idx[np.argmax(M[idx])]
    first = idx[M[idx].astype(np.float64) >= ex.EDGE * float(M[peak])][0]
    start = int(first) - (N - 1) + ex.AHEAD
    f_coarse = np.angle(P[peak]) / (2 * np.pi * ex.HALF)
    coarse = rx[start:] * np.exp(-2j * np.pi * f_coarse * np.arange(rx.size - start))
    # the prefixes, one block per symbol
    frames = coarse[: n_sym * L]
    Pc, Mc, _ = window_metric(frames, G, N, 0.0)
    at = np.arange(n_sym) * L + Mc.reshape(n_sym, L).argmax(axis=1)
    f_fine = np.angle(Pc[at].sum()) / (2 * np.pi * N)
    fixed = coarse * np.exp(-2j * np.pi * f_fine * np.arange(coarse.size))
    window = fixed[L:]
    y_train = ot.demod_truth(window, N, G, ex.BINS, ex.N_TRAIN, None, 1 / np.sqrt(N))
    h, eq, _ = ot.estimate_truth(y_train.astype(np.complex64), train.astype(np.complex64), ex.N_TRAIN, 1, K, 0.0, ot.MATCHED)
    z = ot.demod_truth(window[ex.N_TRAIN * L:], N, G, ex.BINS, ex.N_DATA, eq, 1 / np.sqrt(N)).reshape(-1)
    soft = np.empty(2 * z.size)
    soft[0::2], soft[1::2] = 4 * z.real * ex.SOFT_SCALE, 4 * z.imag * ex.SOFT_SCALE
    soft = np.clip(np.rint(soft), -127, 127)
    decoded = viterbi(soft, ex.POLYS)
    return int((decoded != bits).sum()), start, float(f_coarse), float(f_coarse + f_fine)


def test_restatement_decodes_without_error_inside_the_recorded_figures():
    ex = example()
    for seed in (0, 7, 19):
        errors, start, f_coarse, f = restate(ex, seed)
        assert errors == 0, seed
        assert abs(start - expected_start(ex)) <= WORST_START, (seed, start)
        assert abs(f_coarse - ex.FREQ) <= WORST_COARSE and abs(f - ex.FREQ) <= WORST_FREQ, (seed, f_coarse, f)


@pytest.mark.gpu
def test_detect_example_finds_the_burst_and_decodes_every_bit(ctx):
    ex = example()
    r = ex.main(keep=True)
    r.pop("ctx").close()
    lo, hi = r["planted_start"] - (ex.G - (ex.TAPS.size - 1)), r["planted_start"]
    print(f"start {r['start']} (clean prefix {lo} .. {hi}, expected {expected_start(ex)} +- {2 * WORST_START}), coarse offset error "
          f"{r['freq_coarse'] - ex.FREQ:+.3e} (bound {2 * WORST_COARSE:.3e}), offset error {r['freq'] - ex.FREQ:+.3e} (bound {2 * WORST_FREQ:.3e})")
    assert r["route"] == "fused"
    assert r["errors"] == 0
    assert lo <= r["start"] <= hi
    assert abs(r["start"] - expected_start(ex)) <= 2 * WORST_START
    assert abs(r["freq_coarse"] - ex.FREQ) <= 2 * WORST_COARSE
    assert abs(r["freq"] - ex.FREQ) <= 2 * WORST_FREQ


if __name__ == "__main__":
    ex_ = example()
    res = [restate(ex_, s) for s in range(20)]
    print("decoded errors", [e for e, _, _, _ in res])
    print("start - target", [s - expected_start(ex_) for _, s, _, _ in res], "planted", ex_.START + ex_.G, "expected", expected_start(ex_))
    print(f"coarse worst {max(abs(c - ex_.FREQ) for _, _, c, _ in res):.4e}  total worst {max(abs(f - ex_.FREQ) for _, _, _, f in res):.4e}")
