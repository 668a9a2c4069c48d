#!/usr/bin/env python3
"""`spectrum` and `waterfall` of the reference's plotting helpers (src/util/plot.rs:102-130 and :36-68) computed on the
device: noise plus a tone -> chunks of fft_len -> vec_rfft(Scale::SN) -> vec_mirror -> DB::from(c.norm()).db() per bin,
all of it ONE call (`HipFft.levels`); then `stats()` of the first frame's spectrum for the peak bin.

What crosses PCIe: frames x fft_len floats for the waterfall (what a plot would draw), and nothing but the 64-byte
record for the peak.  Prints the numbers instead of plotting."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import aether_primitives_amd as ap
from aether_primitives_amd import Scale, noise


def main(fft_len=2048, frames=500, tone_bin=300):
    ctx = ap.Context(0)
    # a tone in bin `tone_bin` of every frame (the reference's fwd carries the +j exponent), buried in noise
    t = np.arange(fft_len * frames) % fft_len
    x = ctx.vec((4.0 * np.exp(-2j * np.pi * tone_bin * t / fft_len)).astype(np.complex64))
    noise.new(ctx, 1.0, 815).apply(x)                                # noise::new(1.0, 815)
    fft = ap.HipFft(ctx, fft_len, max_batch=frames)
    # waterfall: every frame's levels in dB, mirrored (plot.rs:59-66 with use_db); the spectrum itself is never stored
    levels = fft.levels(x, Scale.SN, mirror=True, kind=ap.LEVEL_DB)
    water = levels.to_host().reshape(frames, fft_len)
    # spectrum of one frame (plot.rs:109-130) and its peak, found on the device
    spec = ctx.empty(fft_len)
    fft.rfft_mirror(x.slice(0, fft_len), Scale.SN, out=spec)
    st = spec.stats()
    peak_bin = (st.max_index + fft_len // 2) % fft_len               # undo vec_mirror
    print(f"{frames} x {fft_len}: waterfall median level {np.median(water):.2f} (10 log10 |c|, the reference's dB), "
          f"peak of frame 0 in bin {peak_bin} at |c| = {st.max_norm:.1f}, mean power per bin {st.power:.2f}")
    return water, st, peak_bin


if __name__ == "__main__":
    main()
