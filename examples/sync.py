#!/usr/bin/env python3
"""Frame synchronisation with the streaming correlator (the reference's open item "Add Correlation by Freq. Domain
Convolution", README.md:95): a BPSK-mapped m-sequence is planted at known offsets in noise made by the library
(noise::new(power, seed) + apply, src/noise.rs), and `Corr.search` finds every occurrence in ONE pass over the stream.

What crosses PCIe on the way back: one 16-byte record per overlap-save block (hop samples) and the best record of the
stream; the correlation itself is never written anywhere.  A record holds the strongest sample of its block, so two
occurrences closer than a block apart can share a record; preambles are rarer than that."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import aether_primitives_amd as ap
from aether_primitives_amd import noise


def m_sequence(order=7, taps=(7, 6)):
    """maximal-length sequence of 2^order - 1 chips from the Fibonacci LFSR x^7 + x^6 + 1, mapped 0 -> +1, 1 -> -1"""
    state = [1] * order
    out = []
    for _ in range((1 << order) - 1):
        out.append(state[-1])
        fb = 0
        for t in taps:
            fb ^= state[t - 1]
        state = [fb] + state[:-1]
    return (1.0 - 2.0 * np.array(out)).astype(np.complex64)


def main(n=1 << 20, offsets=(1000, 300000, 777777, 1040000), power=0.5, fft_len=2048):
    ctx = ap.Context(0)
    pre = m_sequence()
    m = pre.size
    x = np.zeros(n, np.complex64)
    for p in offsets:
        x[p:p + m] += pre
    d = ctx.vec(x)
    noise.new(ctx, power, 815).apply(d)
    corr = ap.Corr(ctx, pre, fft_len)
    best, rec = corr.search(d, blocks=True)
    # an occurrence correlates to m = 127; noise alone stays near sqrt(m * power) = 8 per sample
    thr = 0.6 * m
    hits = [int(r["index"]) - (m - 1) for r in rec if r["norm"] > thr]
    print(f"{n} samples, {rec.size} blocks of {corr.hop}: threshold {thr:.1f}, strongest |c| = {best.norm:.1f} at lag {best.lag}")
    print("hits:", " ".join(str(h) for h in hits))
    ctx.close()
    return hits, best, rec


if __name__ == "__main__":
    main()
