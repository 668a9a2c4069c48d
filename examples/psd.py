#!/usr/bin/env python3
"""Welch's averaged periodogram on the device: a tone 30 dB under the noise of a single frame, found in one row of 1024
numbers (`Channelizer.sums`, aeth_chan_exec_sums).

2^20 samples of device AWGN of power 1 (deviation 1 / sqrt 2 per component) plus a tone of amplitude 0.05 at 200 / 1024
cycles per sample go through a Channelizer with the periodic Hann window, M = 1024, hop 512, zeros in front.  By the
window's sums a frame shows the tone at a^2 (M / 2)^2 = 655 over a noise level of 3 M / 8 = 384 per bin; the largest of
1024 noise bins in one frame is about 384 ln 1024 = 2660, so a single frame does not show it.  The mean over 2048 frames
has a noise spread near 12 around 384: there bin 200 stands 4 dB over the floor, unmistakable.

Nothing but the traces that are printed from leaves the device: 1024 floats each.  (Seed 815: the single frame's largest
bin is not 200.)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import aether_primitives_amd as ap
from aether_primitives_amd import chan, nco, noise

M, HOP, TONE_BIN, AMP = 1024, 512, 200, 0.05


def main(n=1 << 20, seed=815):
    ctx = ap.Context(0)
    x = nco.Nco(ctx, freq=TONE_BIN / M).tone(n, AMP)
    noise.new(ctx, np.sqrt(0.5), seed).apply(x)
    bank = ap.Channelizer(ctx, chan.prototype("hann", M, 1), M, hop=HOP)
    frames = bank.frames(n)

    # the averaged row: sum / frames, as power in dB
    # (with the -j exponent a tone exp(+2 pi i k t / M) lands in bin k)
    total, _ = bank.sums(x, sign=ap.SIGN_REF_BWD, want=("sum",))
    mean_db = ctx.sum_levels(total, frames, ap.LEVEL_POWER_DB).to_host()
    # one frame alone (the second: the first holds the zeros in front of the capture)
    one, _ = bank.sums(x.slice(HOP, 2 * HOP), hist=x.slice(0, M - HOP), sign=ap.SIGN_REF_BWD, want=("sum",))
    one_db = ctx.sum_levels(one, 1, ap.LEVEL_POWER_DB).to_host()

    peak, single = int(np.argmax(mean_db)), int(np.argmax(one_db))
    floor_db = float(np.median(mean_db))
    over = float(mean_db[TONE_BIN] - floor_db)
    print(f"{frames} frames of {M} bins, route {'fused' if bank.sums_fused else 'general'}, chunks of {bank.sums_chunk} frames")
    print(f"largest bin of the averaged spectrum: {peak}")
    print(f"largest bin of one frame alone: {single}")
    print(f"noise floor {floor_db:.2f} dB (3 M / 8 is {10 * np.log10(3 * M / 8):.2f} dB), tone {over:.2f} dB over it")
    del bank, x, total, one
    ctx.close()
    return peak, single, floor_db, over


if __name__ == "__main__":
    main()
