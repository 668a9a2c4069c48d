#!/usr/bin/env python3
"""The 802.11a 36 Mbit/s mode end to end on the device: 16-QAM, rate 3/4, interleaved over the 192 coded bits of an OFDM
symbol.  Only bits leave the device.

Transmit, 144 data bits per OFDM symbol:
  1. `Sequence.scramble` with x^7 + x^4 + 1;
  2. `ConvCode` K = 7 (0o133, 0o171), rate 1/2: 288 coded bits per symbol;
  3. ONE `Remap`: the puncturer [1, 1, 1, 0, 0, 1] (rate 3/4, 192 bits) followed by the interleaver `bicm16(192, 4)`,
     composed on the host into a single 288 -> 192 table;
  4. a Gray 16-QAM table through `modulation.table` (b0 b1 choose I, b2 b3 choose Q; 00, 01, 11, 10 -> -3, -1, 1, 3);
  5. `Ofdm.mod` at N = 64, G = 16 on the 48 data carriers (-26 .. 26 without 0, +-7 and +-21: pilots are not built).
Then AWGN.  Receive: `Ofdm.demod`, `demod_soft`, ONE `Remap` -- the inverse of the transmit table, which deinterleaves and
puts an erasure (fill 0) where a bit was punctured --, `ConvCode.decode_stream`, and the scrambler again.

Beside the decoded bit errors it prints the raw hard-decision errors of the 192 bits per symbol that went over the air,
and the errors of the same chain without noise.  POWER is the noise deviation per component against carriers of unit mean
energy: Es/N0 = 1 / (2 POWER^2), about 13.8 dB, i.e. Eb/N0 about 9 dB at three data bits per carrier."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import aether_primitives_amd as ap
from aether_primitives_amd import modulation, noise

N, G = 64, 16
BINS = np.array([b % N for b in range(-26, 27) if b not in (0, -21, -7, 7, 21)])   # the 48 data carriers
N_DBPS, N_CBPS, N_BPSC = 144, 192, 4
POLYS = (0o133, 0o171)
KEEP = (1, 1, 1, 0, 0, 1)
SCRAMBLER, SCRAMBLER_INIT = (4, 7), 0b1011101                       # s[n] = s[n - 4] ^ s[n - 7]
POWER, SOFT_SCALE = 0.144, 32.0                                     # L = 32 (d1^2 - d0^2): +-13 next to a decision line
LEVELS = np.array([-3.0, -1.0, 3.0, 1.0])                           # by 2 b0 + b1: 00 -> -3, 01 -> -1, 10 -> 3, 11 -> 1


def qam16_table():
    """index = b0 + 2 b1 + 4 b2 + 8 b3 with b0 the first bit in time; Gray in both axes, unit mean energy"""
    idx = np.arange(16)
    return ((LEVELS[((idx & 1) << 1) | ((idx >> 1) & 1)] + 1j * LEVELS[(((idx >> 2) & 1) << 1) | ((idx >> 3) & 1)]) / np.sqrt(10.0)).astype(np.complex64)


def chain(ctx, parts, bits, awgn):
    """-> (decoded bits, hard decisions of the bits on the air, the bits on the air), all on the host"""
    scr, code, tx_map, rx_map, m, ofdm = parts
    n_sym = bits.size // N_DBPS
    scrambled = scr.scramble(SCRAMBLER_INIT, ap.DeviceBits(ctx, bits.size, bits))
    coded = code.encode(scrambled)
    air = tx_map.exec(coded)                                         # puncture and interleave: one pass
    x = ofdm.mod(m.modulate(air), n_sym, scale=ap.Scale.SN)
    if awgn is not None:
        awgn.apply(x)
    z = ofdm.demod(x.slice(G, x.n), n_sym, scale=ap.Scale.SN)
    soft = rx_map.exec(m.demod_soft(z, SOFT_SCALE), fill=0)          # deinterleave and depuncture to erasures: one pass
    decoded = scr.scramble(SCRAMBLER_INIT, code.decode_stream(soft))
    return decoded.to_host(), m.demod_naive(z, compat=False).to_host(), air.to_host()


def main(n_sym=20, power=POWER, seed=815):
    ctx = ap.Context(0)
    tx_map = ap.Remap.puncture(ctx, KEEP).then(ap.Remap.bicm16(ctx, N_CBPS, N_BPSC))
    parts = (ap.Sequence(ctx, SCRAMBLER), ap.ConvCode(ctx, 7, POLYS), tx_map, tx_map.inverse(), modulation.table(ctx, qam16_table()),
             ap.Ofdm(ctx, N, G, BINS, max_symbols=n_sym))
    bits = np.random.default_rng(seed).integers(0, 2, N_DBPS * n_sym, dtype=np.uint8)
    clean, _, _ = chain(ctx, parts, bits, None)
    decoded, hard, air = chain(ctx, parts, bits, noise.new(ctx, power, seed))
    raw, errors, quiet = int((hard != air).sum()), int((decoded != bits).sum()), int((clean != bits).sum())
    print(f"{bits.size} bits in {n_sym} OFDM symbols, K = 7 rate 3/4, 16-QAM, one {tx_map.r_in} -> {tx_map.r_out} map each way "
          f"+ AWGN(power {power}): raw errors {raw} of {air.size} bits on the air ({100.0 * raw / air.size:.2f} %), "
          f"decoded errors {errors}, noise-free errors {quiet}")
    return errors


if __name__ == "__main__":
    main()
