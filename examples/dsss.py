#!/usr/bin/env python3
"""Direct-sequence spread spectrum end to end on the device ("Such sequences are common building blocks for scrambling,
synchronisation or modulation (Direct-Sequence Spread-Spectrum) systems", src/sequence.rs:24-25): 64 data bits -> BPSK ->
every symbol spread by the 127 chips of the order-7 m-sequence -> AWGN -> the streaming correlator with the same chips as
its template -> one sample per symbol -> the sign of its real part.

The m-sequence is never built on the host: `spread` generates it inside the pass that writes the chips, and `chips`
makes the correlator's template.  Its period equals the spreading factor, so every symbol meets the same 127 chips."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import aether_primitives_amd as ap
from aether_primitives_amd import modulation, noise

M7, M7_INIT, SF = (6, 7), 0x7f, 127          # seq[n] = seq[n-6] ^ seq[n-7] from seven ones: x^7 + x^6 + 1, period 127


def main(nbits=64, power=1.0, seed=815, fft_len=2048):
    ctx = ap.Context(0)
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 2, nbits, dtype=np.uint8)
    m7 = ap.Sequence(ctx, M7)
    sym = modulation.bpsk(ctx).modulate(data)                    # 0 -> 1+1j, 1 -> -1-1j (modulation.rs:77)
    tx = m7.spread(M7_INIT, sym, SF)                             # nbits * 127 chips
    noise.new(ctx, power, seed).apply(tx)                        # amplitude proportional to `power` (noise.rs:41-42,58): deviation 1 per component
    template = m7.chips(M7_INIT, SF, zero=1 + 0j, one=-1 + 0j)   # real +-1 chips: 0 -> +1, 1 -> -1
    corr = ap.Corr(ctx, template.to_host(), fft_len)
    c = corr.correlate(tx).to_host()
    # symbol k occupies chips 127 k .. 127 k + 126; the matched filter is full at its last chip
    peaks = c[SF - 1::SF]
    got = (peaks.real < 0).astype(np.uint8)
    errors = int((got != data).sum())
    print(f"{nbits} bits x {SF} chips, noise power {power}: |peak| {np.abs(peaks.real).min():.1f} .. {np.abs(peaks.real).max():.1f} "
          f"(clean: {SF}), {errors} bit errors")
    chips = template.to_host()
    ctx.close()
    return data, got, peaks, chips


if __name__ == "__main__":
    main()
