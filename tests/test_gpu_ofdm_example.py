"""examples/ofdm.py end to end: a coded OFDM burst through multipath, a carrier offset and noise, decoded on the device.

  * no decoded bit error;
  * the raw (uncoded) bit error rate inside a band;
  * the channel estimate as close to the planted channel as the restatement says it can be.

The band and the bound come from `restate` below: a numpy restatement of the SAME chain -- the same constants (imported
from the example), convolutional encoder, QPSK, tests/ofdm_truth.py for the symbols, np.convolve for the channel, the
prefix-against-tail lag sum, the f64 estimate, CSI-weighted soft values rounded and clamped like aeth_demod_soft, and a
full-traceback Viterbi decoder -- run on the CPU (`python tests/test_gpu_ofdm_example.py`) over seeds 0 .. 19 at the
example's noise level, NOISE_POWER = 0.16 (a complex noise sample of variance 2 * 0.16^2 on received samples of power 1.9:
15.7 dB).  Of the levels 0.05, 0.07, 0.09, 0.12, 0.16, 0.2, 0.25, 0.3, 0.4 the restatement decodes every seed without error up
to 0.25 and loses seeds from 0.3 on; 0.16 leaves 5 dB to that, and its raw error counts (10 to 26 of 1248) are large enough
for a band to mean something.  The restatement's figures at 0.16:
    decoded bit errors   0 in every seed
    raw error rate       min 0.00801, max 0.02083    -> band [0.00401, 0.03125] (widened by half of each)
    estimate error       worst 0.1104 of the norm    -> bound 0.2208 (twice, the margin of test_gpu_acquire_example.py)
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

RAW_MIN, RAW_MAX, WORST_ESTIMATE = 0.00801, 0.02083, 0.1104      # the restatement over seeds 0 .. 19 (see above)


def example():
    spec = importlib.util.spec_from_file_location("example_ofdm", os.path.join(ROOT, "examples", "ofdm.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    return ex


def encode(bits, polys, k=7):
    """c[n t + j] = parity(reg_t & poly[j]), reg_t = sum_i u[t - i] 2^(k - 1 - i), zero history"""
    reg, out = 0, []
    for u in bits:
        reg = (reg >> 1) | (int(u) << (k - 1))
        out += [bin(reg & p).count("1") & 1 for p in polys]
    return np.array(out, np.uint8)


def viterbi(soft, polys, k=7):
    """maximum-metric path from the zero state, full traceback from the best final state; soft > 0 means bit 0"""
    S, n = 1 << (k - 1), len(polys)
    steps = len(soft) // n
    j = np.arange(S)
    u = j >> (k - 2)
    p0 = (2 * j) % S
    sign = np.empty((2, S, n))
    for d in (0, 1):
        reg = (u << (k - 1)) + p0 + d
        for q, p in enumerate(polys):
            par = np.array([bin(int(r) & p).count("1") & 1 for r in reg])
            sign[d, :, q] = 1 - 2 * par
    metric = np.full(S, -1e18)
    metric[0] = 0.0
    choice = np.empty((steps, S), np.uint8)
    v = np.asarray(soft, np.float64).reshape(steps, n)
    for t in range(steps):
        c0 = metric[p0] + sign[0] @ v[t]
        c1 = metric[p0 + 1] + sign[1] @ v[t]
        choice[t] = c1 > c0
        metric = np.where(choice[t], c1, c0)
    s, out = int(np.argmax(metric)), np.empty(steps, np.uint8)
    for t in range(steps - 1, -1, -1):
        out[t] = s >> (k - 2)
        s = (2 * s) % S + int(choice[t, s])
    return out


def restate(ex, seed, noise_power=None):
    """the example's chain in numpy -> (decoded errors, raw error rate, estimate error)"""
    power = ex.NOISE_POWER if noise_power is None else noise_power
    N, G, K, L, n_sym = ex.N, ex.G, ex.K, ex.N + ex.G, ex.N_TRAIN + ex.N_DATA
    r = np.random.default_rng(seed)
    bits = r.integers(0, 2, ex.NBITS, dtype=np.uint8)
    bits[-ex.TAIL:] = 0
    coded = encode(bits, ex.POLYS)
    table = np.array([1 + 1j, -1 + 1j, 1 - 1j, -1 - 1j])
    data = table[(coded[1::2].astype(int) << 1) + coded[0::2]]
    train = ex.training_symbol().astype(np.complex128)
    car = np.concatenate([np.tile(train, ex.N_TRAIN), data])
    tx = ot.mod_truth(car, N, G, ex.BINS, n_sym, 1 / np.sqrt(N))
    rx = np.convolve(tx, ex.TAPS.astype(np.complex128))[: tx.size]
    rx = rx * np.exp(2j * np.pi * (ex.FREQ * np.arange(rx.size) + ex.PHASE))
    rx = rx + power * (r.standard_normal(rx.size) + 1j * r.standard_normal(rx.size))
    # carrier offset: the tails against their prefixes
    i = (np.arange(n_sym)[:, None] * L + N + np.arange(G)[None, :]).reshape(-1)
    lag_sum = np.sum(rx[i] * np.conj(rx[i - N]))
    f = np.angle(lag_sum) / (2 * np.pi * N)
    fixed = rx * np.exp(-2j * np.pi * f * np.arange(rx.size))
    window = fixed[G - ex.ADVANCE:]
    y_train = ot.demod_truth(window, N, G, ex.BINS, ex.N_TRAIN, None, 1 / np.sqrt(N))
    h, eq, _ = ot.estimate_truth(y_train.astype(np.complex64), train.astype(np.complex64), ex.N_TRAIN, 1, K, 0.0, ot.MATCHED)
    z = ot.demod_truth(window[ex.N_TRAIN * L:], N, G, ex.BINS, ex.N_DATA, eq, 1 / np.sqrt(N)).reshape(-1)
    soft = np.empty(2 * z.size)
    soft[0::2], soft[1::2] = 4 * z.real * ex.SOFT_SCALE, 4 * z.imag * ex.SOFT_SCALE      # (d2 with the bit 1 - with the bit 0) * scale
    soft = np.clip(np.rint(soft), -127, 127)
    hard = np.empty(2 * z.size, np.uint8)
    hard[0::2], hard[1::2] = z.real < 0, z.imag < 0
    decoded = viterbi(soft, ex.POLYS)
    return int((decoded != bits).sum()), float((hard != coded).mean()), ex.estimate_error(h, ex.planted_channel())


def test_restatement_decodes_without_error_inside_the_recorded_figures():
    ex = example()
    for seed in (0, 7, 19):
        errors, raw, est = restate(ex, seed)
        assert errors == 0, seed
        assert RAW_MIN <= raw <= RAW_MAX and est <= WORST_ESTIMATE, (seed, raw, est)


def test_restated_pieces_are_the_librarys_definitions():
    """the encoder's convention on the K = 7 impulse response, and the decoder on a noise-free stream"""
    ex = example()
    assert encode([1, 0, 0, 0, 0, 0, 0], ex.POLYS).tolist() == [1, 1, 1, 0, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1]     # 0o171, 0o133 MSB first
    bits = np.random.default_rng(1).integers(0, 2, 200, dtype=np.uint8)
    bits[-8:] = 0
    c = encode(bits, ex.POLYS)
    assert np.array_equal(viterbi(100.0 * (1 - 2.0 * c), ex.POLYS), bits)


@pytest.mark.gpu
def test_ofdm_example_decodes_every_bit_and_estimates_the_planted_channel(ctx):
    ex = example()
    r = ex.main(keep=True)
    r.pop("ctx").close()
    print(f"raw error rate {r['raw_rate']:.5f} (band {0.5 * RAW_MIN:.5f} .. {1.5 * RAW_MAX:.5f}), estimate error "
          f"{r['estimate_error']:.4f} (bound {2 * WORST_ESTIMATE:.4f}), carrier offset {r['freq']:.3e} (planted {ex.FREQ:.3e})")
    assert r["route"] == "fused"
    assert r["errors"] == 0
    assert 0.5 * RAW_MIN <= r["raw_rate"] <= 1.5 * RAW_MAX
    assert r["estimate_error"] <= 2 * WORST_ESTIMATE


if __name__ == "__main__":
    ex_ = example()
    for p in (0.05, 0.07, 0.09, 0.12, 0.16, 0.2, 0.25, 0.3, 0.4):
        res = [restate(ex_, s, p) for s in range(20)]
        print(f"noise power {p}: decoded errors {[e for e, _, _ in res]}, raw min {min(r for _, r, _ in res):.5f} "
              f"max {max(r for _, r, _ in res):.5f}, estimate worst {max(e for _, _, e in res):.4f}")
