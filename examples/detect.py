#!/usr/bin/env python3
"""The coded OFDM link of examples/ofdm.py with the burst at a start the receiver is not told: only records, the
52-entry channel estimate and bits are downloaded.

Transmit: as in ofdm.py (random bits, `ConvCode` K = 7 rate 1/2, QPSK, `Ofdm.mod` at N = 64, G = 16, two known training
symbols), behind one more symbol on the EVEN carriers only: its two halves of N / 2 samples are identical (Schmidl and
Cox).  The burst sits in a capture that begins with START samples of nothing.

Channel: three taps through `Fir`, a carrier offset of 30 % of the carrier spacing and a phase planted with `Nco`, AWGN
over the whole capture: the receiver sees noise, not zeros, in front of the burst.

Receive:
  1. `mov.search` with L = W = N / 2 over the capture: the metric |P|^2 / (R(i) R(i - L)) is near 1 while window and partner
     lie in the repeated stretch (the prefix continues it: a plateau of G + 1 samples less the channel's length) and near
     1 / W in noise.  The record's P at the peak gives, through `mov.freq_step`, the `Nco` step that removes the offset;
  2. `mov.search` again with the threshold at 0.9 of the peak: `first` is where the metric climbs onto the plateau (the
     peak itself wanders over the plateau with the noise).  The first window sample is taken AHEAD samples behind the
     crossing: inside the part of the prefix the channel has left clean;
  3. the cyclic prefixes (L = N, W = G, one block per symbol from the detected start: one record each) add up to the fine
     carrier offset, as the lag sum of ofdm.py does;
  4. the rest as in ofdm.py: `Ofdm.demod` of the training symbols, `Ofdm.estimate` ("matched"), `Ofdm.demod` of the
     payload, `demod_soft`, the Viterbi decoder."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import aether_primitives_amd as ap
from aether_primitives_amd import modulation, mov, noise

N, G = 64, 16
HALF = N // 2
BINS = np.array(list(range(N - 26, N)) + list(range(1, 27)))       # -26 .. -1, 1 .. 26
K = BINS.size
N_TRAIN, N_DATA = 2, 12
NBITS, TAIL = N_DATA * K, 8
POLYS = (0o171, 0o133)
TAPS = np.array([0.85, 0.45 - 0.35j, -0.2 + 0.3j], np.complex64)
FREQ, PHASE = 0.3 / N, 0.17                                         # cycles per sample (30 % of the spacing), cycles
NOISE_POWER = 0.16                                                  # Awgn's `power`: a complex sample of variance 2 power^2
SOFT_SCALE = 6.0
TRAIN_SEED, SC_SEED = 64, 65
START, REST = 3217, 600                                             # samples in front of the burst and behind it
R_MIN = 0.25 * HALF                                                 # window power: noise alone gives 0.05 W, the burst 1.9 W
EDGE = 0.9                                                          # the crossing is taken at this fraction of the peak
AHEAD = 11                                                          # first window sample, counted from the crossing's window start: the
                                                                    # middle of the clean prefix (tests/test_gpu_detect_example.py measures it)


def training_symbol():
    idx = np.random.default_rng(TRAIN_SEED).integers(0, 4, K)
    return modulation.GENERIC_QPSK_TABLE[idx]


def repeated_symbol():
    """QPSK on the even carriers, nothing on the odd ones, at the power of a full symbol: two identical halves"""
    idx = np.random.default_rng(SC_SEED).integers(0, 4, K)
    return (modulation.GENERIC_QPSK_TABLE[idx] * np.where(BINS % 2 == 0, np.sqrt(2.0), 0.0)).astype(np.complex64)


def planted_channel(advance):
    """what the carriers see: the taps' response at each bin and the ramp of a window `advance` samples early"""
    h = np.zeros(N, np.complex128)
    h[:TAPS.size] = TAPS
    hf = np.fft.ifft(h) * N
    return (hf * np.exp(2j * np.pi * np.arange(N) * advance / N))[BINS]


def estimate_error(h, planted):
    h, planted = np.asarray(h, np.complex128), np.asarray(planted, np.complex128)
    c = np.vdot(planted, h) / np.vdot(planted, planted)
    return float(np.linalg.norm(h - c * planted) / np.linalg.norm(c * planted))


def signed(word):
    """a 64-bit word as a signed fraction of a turn"""
    return ((int(word) + (1 << 63)) % (1 << 64) - (1 << 63)) / 2.0 ** 64


def main(seed=815, keep=False):
    ctx = ap.Context(0)
    L, n_sym = N + G, 1 + N_TRAIN + N_DATA
    ofdm = ap.Ofdm(ctx, N, G, BINS, max_symbols=n_sym)
    code = ap.ConvCode(ctx, 7, POLYS)
    m = modulation.qpsk(ctx)
    train = training_symbol()

    # ---- transmit ------------------------------------------------------------------------------------------------------
    bits = np.random.default_rng(seed).integers(0, 2, NBITS, dtype=np.uint8)
    bits[-TAIL:] = 0
    coded = code.encode(ap.DeviceBits(ctx, NBITS, bits))
    carriers = ctx.empty(n_sym * K)
    ctx.upload(carriers.ptr, np.concatenate([repeated_symbol(), np.tile(train, N_TRAIN)]))
    m.modulate(coded, out=carriers.slice((1 + N_TRAIN) * K, n_sym * K))
    tx = ofdm.mod(carriers, n_sym, scale=ap.Scale.SN)
    capture = ctx.empty(START + tx.n + REST).vec_zero()
    capture.slice(START, START + tx.n).vec_clone(tx)

    # ---- channel -------------------------------------------------------------------------------------------------------
    rx = ap.Fir(ctx, TAPS).filter(capture)
    ap.Nco(ctx, FREQ, PHASE).mix(rx, out=rx)
    noise.new(ctx, NOISE_POWER, seed).apply(rx)

    # ---- receive -------------------------------------------------------------------------------------------------------
    _, peak = mov.search(ctx, rx, mov.LAG, HALF, HALF, R_MIN, 0.0)
    _, edge = mov.search(ctx, rx, mov.LAG, HALF, HALF, R_MIN, EDGE * peak.metric)
    start = int(edge.first) - (N - 1) + AHEAD                       # the first window sample of the repeated symbol
    coarse_step = mov.freq_step(peak, HALF)
    coarse = ap.Nco.from_words(ctx, step=coarse_step).mix(rx.slice(start, rx.n))
    # the prefixes against their tails, one block per symbol: block s ends behind symbol s's last sample
    frames = coarse.slice(0, n_sym * L)
    recs, _ = mov.search(ctx, frames, mov.LAG, G, N, 0.0, 0.0, block=L)
    fine_step = mov.freq_step(complex(recs["p_re"].sum(), recs["p_im"].sum()), N)
    fixed = ap.Nco.from_words(ctx, step=fine_step).mix(coarse)
    window = fixed.slice(L, fixed.n)                                 # the first training symbol's window
    y_train = ofdm.demod(window, N_TRAIN, scale=ap.Scale.SN)
    h, eq, csi = ofdm.estimate(y_train, train, kind="matched")
    z = ofdm.demod(window.slice(N_TRAIN * L, window.n), N_DATA, eq=eq, scale=ap.Scale.SN)
    soft = m.demod_soft(z, SOFT_SCALE)
    decoded = code.decode_stream(soft).to_host()
    hard = m.demod_naive(z, compat=False).to_host()

    raw_errors = int((hard != coded.to_host()).sum())
    errors = int((decoded != bits).sum())
    planted_start = START + G                                        # the repeated symbol's first sample behind its prefix
    h_host = h.to_host()
    err = estimate_error(h_host, planted_channel(planted_start - start))
    freq_coarse = -signed(coarse_step)
    freq = freq_coarse - signed(fine_step)
    print(f"burst found at {start} (planted {planted_start}: the window begins {planted_start - start} samples into the prefix of {G}), "
          f"metric {peak.metric:.3f} at {peak.index}, crossing at {edge.first}; carrier offset {freq_coarse:.4e} from the repeated "
          f"halves, {freq:.4e} with the prefixes (planted {FREQ:.4e} cycles per sample); channel estimate off by {err:.4f} of its "
          f"norm, raw bit errors {raw_errors} of {2 * NBITS}, decoded bit errors {errors} of {NBITS}")
    out = {"errors": errors, "raw_errors": raw_errors, "raw_rate": raw_errors / (2.0 * NBITS), "estimate_error": err, "start": start,
           "planted_start": planted_start, "index": int(peak.index), "first": int(edge.first), "metric": float(peak.metric),
           "freq_coarse": freq_coarse, "freq": freq, "route": ofdm.route}
    if keep:
        out.update(ctx=ctx)                                          # the caller closes the context
        return out
    del tx, capture, rx, coarse, frames, fixed, window, y_train, h, eq, csi, z, soft, carriers, coded
    ofdm.close(); code.close()
    ctx.close()
    return out


if __name__ == "__main__":
    main()
