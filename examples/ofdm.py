#!/usr/bin/env python3
"""A coded OFDM link that stays on the device: only bits, a handful of 48-byte records and the 52-entry channel estimate
are downloaded.

Transmit: random bits (the last eight zero, a tail) -> `ConvCode` K = 7, rate 1/2 -> QPSK (the generic table) -> `Ofdm.mod`
at N = 64, G = 16 on the 52 carriers -26 .. -1, 1 .. 26, behind two copies of a known training symbol.

Channel: three taps through `Fir`, a carrier offset of 3 % of the carrier spacing and a phase planted with `Nco`, AWGN.

Receive:
  1. `sync.lag` at lag 64 in blocks of 16 samples: the cyclic prefix correlates with the tail of its symbol, so the blocks
     that hold the tails (the framing is known: the example plants it) sum to |.| exp(2 pi i 64 f).  The records are added
     on the host and `sync.freq_step` turns the sum into the `Nco` step that removes the offset;
  2. the window is taken four samples into the prefix (pointer arithmetic; the ramp that leaves is part of the channel);
  3. `Ofdm.demod` of the two training symbols, `Ofdm.estimate` with "matched": eq = conj(H);
  4. `Ofdm.demod` of the payload with eq: |H|^2 X + noise, i.e. CSI-weighted symbols;
  5. `demod_soft` and the Viterbi decoder (`ConvCode.decode_stream`).
What is left of the offset turns every later symbol a little further; no pilot tracks it (not built), so
the burst is short."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import aether_primitives_amd as ap
from aether_primitives_amd import modulation, noise, sync

N, G, ADVANCE = 64, 16, 4
BINS = np.array(list(range(N - 26, N)) + list(range(1, 27)))       # -26 .. -1, 1 .. 26
K = BINS.size
N_TRAIN, N_DATA = 2, 12
NBITS, TAIL = N_DATA * K, 8                                         # one info bit per carrier: rate 1/2, two bits per symbol
POLYS = (0o171, 0o133)
TAPS = np.array([0.85, 0.45 - 0.35j, -0.2 + 0.3j], np.complex64)
FREQ, PHASE = 0.03 / N, 0.17                                        # cycles per sample (3 % of the spacing), cycles
NOISE_POWER = 0.16                                                  # Awgn's `power`: a complex sample of variance 2 power^2
SOFT_SCALE = 6.0
TRAIN_SEED = 64


def training_symbol():
    """the known symbol: QPSK from a fixed seed"""
    idx = np.random.default_rng(TRAIN_SEED).integers(0, 4, K)
    return modulation.GENERIC_QPSK_TABLE[idx]


def planted_channel():
    """what the carriers see: the taps' response at each bin (transform with demod's sign) and the ramp of the advanced window"""
    h = np.zeros(N, np.complex128)
    h[:TAPS.size] = TAPS
    hf = np.fft.ifft(h) * N                                         # sum_t h[t] exp(+2 pi i b t / N)
    return (hf * np.exp(2j * np.pi * np.arange(N) * ADVANCE / N))[BINS]


def estimate_error(h, planted):
    """|h - c planted| / |planted| with the common complex factor c that fits best (the carrier's phase is not known)"""
    h, planted = np.asarray(h, np.complex128), np.asarray(planted, np.complex128)
    c = np.vdot(planted, h) / np.vdot(planted, planted)
    return float(np.linalg.norm(h - c * planted) / np.linalg.norm(c * planted))


def tail_blocks(n_sym):
    """indices of the 16-sample blocks whose lag-64 partners are the prefixes: block 4 of the 5 in every symbol"""
    return np.arange(n_sym) * ((N + G) // 16) + N // 16


def main(seed=815, keep=False):
    ctx = ap.Context(0)
    L, n_sym = N + G, N_TRAIN + N_DATA
    ofdm = ap.Ofdm(ctx, N, G, BINS, max_symbols=n_sym)
    code = ap.ConvCode(ctx, 7, POLYS)
    m = modulation.qpsk(ctx)
    train = training_symbol()

    # ---- transmit ------------------------------------------------------------------------------------------------------
    bits = np.random.default_rng(seed).integers(0, 2, NBITS, dtype=np.uint8)
    bits[-TAIL:] = 0
    coded = code.encode(ap.DeviceBits(ctx, NBITS, bits))
    carriers = ctx.empty(n_sym * K)
    ctx.upload(carriers.ptr, np.tile(train, N_TRAIN))
    m.modulate(coded, out=carriers.slice(N_TRAIN * K, n_sym * K))
    tx = ofdm.mod(carriers, n_sym, scale=ap.Scale.SN)

    # ---- channel -------------------------------------------------------------------------------------------------------
    rx = ap.Fir(ctx, TAPS).filter(tx)
    ap.Nco(ctx, FREQ, PHASE).mix(rx, out=rx)
    noise.new(ctx, NOISE_POWER, seed).apply(rx)

    # ---- receive -------------------------------------------------------------------------------------------------------
    recs, _ = sync.lag(ctx, rx, 1, N, block=16)
    pick = recs[tail_blocks(n_sym)]
    lag_sum = complex(pick["re"].sum(), pick["im"].sum())
    f_step = sync.freq_step(lag_sum, 1, N)
    fixed = ap.Nco.from_words(ctx, step=f_step).mix(rx)
    window = fixed.slice(G - ADVANCE, fixed.n)
    y_train = ofdm.demod(window, N_TRAIN, scale=ap.Scale.SN)
    h, eq, csi = ofdm.estimate(y_train, train, kind="matched")
    z = ofdm.demod(window.slice(N_TRAIN * L, window.n), N_DATA, eq=eq, scale=ap.Scale.SN)
    soft = m.demod_soft(z, SOFT_SCALE)
    decoded = code.decode_stream(soft).to_host()
    hard = m.demod_naive(z, compat=False).to_host()

    raw_errors = int((hard != coded.to_host()).sum())
    errors = int((decoded != bits).sum())
    h_host = h.to_host()
    err = estimate_error(h_host, planted_channel())
    freq = -((int(f_step) + (1 << 63)) % (1 << 64) - (1 << 63)) / 2.0 ** 64
    print(f"{NBITS} bits, K = 7 rate 1/2, QPSK on {K} of {N} carriers, prefix {G}, {N_DATA} symbols behind {N_TRAIN} training symbols "
          f"({ofdm.route}): carrier offset {freq:.3e} cycles per sample (planted {FREQ:.3e}), channel estimate off by {err:.4f} "
          f"of its norm, raw bit errors {raw_errors} of {2 * NBITS}, decoded bit errors {errors} of {NBITS}")
    out = {"errors": errors, "raw_errors": raw_errors, "raw_rate": raw_errors / (2.0 * NBITS), "estimate_error": err, "freq": freq,
           "h": h_host, "csi": csi.to_host(), "route": ofdm.route}
    if keep:
        out.update(ctx=ctx)                                          # the caller closes the context
        return out
    del tx, rx, fixed, window, y_train, h, eq, csi, z, soft, carriers, coded
    ofdm.close(); code.close()
    ctx.close()
    return out


if __name__ == "__main__":
    main()
