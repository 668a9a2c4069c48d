#!/usr/bin/env python3
"""Take a stream apart, excise an interferer in the frequency domain and put the stream back together.

The reference's `waterfall` (src/util/plot.rs:46-68) only takes a stream apart.  Here a QPSK burst sits under a tone 20 dB
above it.  `Channelizer` makes Hann-windowed frames of 256 points at a hop of 64; `Synthesizer` with the dual window
(`synth.dual_window`) inverts that exactly: part 1 prints the error of the round trip.  Part 2 zeroes the tone's bin and
two bins either side of it in every frame on the device before the synthesis, and prints the tone's level in the stream
before and after (the power of its bin in a long transform, read with `levels`)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import aether_primitives_amd as ap
from aether_primitives_amd import chan, synth

M, D = 256, 64
TONE_BIN, HALF_WIDTH, TONE_AMP = 37, 2, 10.0
N_LONG = 1 << 15                              # the long transform that reads the tone's level


def _db(ratio):
    return 10 * np.log10(max(ratio, 1e-300))


def _tone_level(ctx, stream, start):
    """power (dB) of the tone's bin in an N_LONG-point transform of stream[start : start + N_LONG]"""
    f = ap.HipFft(ctx, N_LONG)
    spec = f.exec(stream.slice(start, start + N_LONG), ctx.empty(N_LONG), ap.SIGN_REF_BWD, ap.Scale.N)
    k = TONE_BIN * N_LONG // M
    return float(spec.levels(ap.LEVEL_POWER_DB).to_host()[k])


def main(n=1 << 16, seed=815):
    ctx = ap.Context(0)
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    qpsk = ((2 * rng.integers(0, 2, n) - 1) + 1j * (2 * rng.integers(0, 2, n) - 1)) / np.sqrt(2)
    qpsk[:n // 8] = 0
    qpsk[7 * n // 8:] = 0                                             # a burst: the middle three quarters
    x = (qpsk + TONE_AMP * np.exp(2j * np.pi * TONE_BIN * t / M)).astype(np.complex64)
    stream = ctx.vec(x)

    w = chan.prototype("hann", M, 1)
    bank = ap.Channelizer(ctx, w, M, D)
    back = ap.Synthesizer(ctx, synth.dual_window(w, D), M, D)
    delay = back.ntaps - back.hop                                     # the reconstruction comes out this much later
    # with the -j exponent a tone exp(+2 pi i k t / M) lands in bin k
    spec = bank.exec(stream, sign=ap.SIGN_REF_BWD)

    # 1: analysis, then synthesis, returns the stream
    out = back.exec(spec, sign=ap.SIGN_REF_FWD, s=ap.Scale.N)
    ref = stream.slice(0, n - delay)
    err = ctx.empty(n - delay).vec_clone(out.slice(delay, n)).vec_sub(ref)
    evm = _db(err.stats().power / ref.stats().power)
    print(f"round trip of {n} samples through {spec.n // M} frames: EVM {evm:.1f} dB, delay {delay} samples")

    # 2: the same with the tone's bins zeroed in every frame
    mask = np.ones(M, np.complex64)
    mask[TONE_BIN - HALF_WIDTH:TONE_BIN + HALF_WIDTH + 1] = 0
    spec.vec_mul_frames(ctx.vec(mask), M)
    clean = back.exec(spec, sign=ap.SIGN_REF_FWD, s=ap.Scale.N)
    before = _tone_level(ctx, stream, M)                              # past the frames that hold the zero history
    after = _tone_level(ctx, clean, M + delay)
    print(f"tone level before {before:.1f} dB, after {after:.1f} dB: {before - after:.1f} dB down")
    del bank, back, spec, out, err, ref, clean, stream
    ctx.close()
    return evm, before, after


if __name__ == "__main__":
    main()
