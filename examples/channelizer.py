#!/usr/bin/env python3
"""A polyphase channelizer and a windowed, overlapped spectrogram of the same capture, both through `Channelizer`.

The reference's `waterfall` (src/util/plot.rs:46-68) frames a capture with chunks_mut(fft_len): disjoint rectangular
frames.  Part 1 splits the capture -- two complex tones at the centres of channels 3 and 11 of 16, plus AWGN -- into 16
critically sampled channels with a Hamming-windowed sinc prototype of 8 taps per channel; the two tone channels stand
out by the prototype's stop-band rejection.  Part 2 makes a spectrogram of 1000-point frames, where the tones fall half
way between two bins: with a Hann window and 50 % overlap (`levels`) the leakage three bins off the tone is set by the
noise floor, with the reference's rectangular framing (`HipFft.levels`) by the sinc sidelobes."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import aether_primitives_amd as ap
from aether_primitives_amd import chan, noise

M, P, TONES = 16, 8, (3, 11)
FRAME = 1000                                  # spectrogram frame: 1000 * 3 / 16 = 187.5, between two bins


def _mean_db(levels, frame):
    """power level of every bin, averaged over the frames (the first holds the zero history)"""
    return levels.to_host().reshape(-1, frame)[1:].mean(axis=0)


def _leak(db, tone_bin):
    """level three bins off the tone's stronger bin, relative to it"""
    lo = int(np.floor(tone_bin))
    peak = lo if db[lo] >= db[lo + 1] else lo + 1
    return max(db[peak - 3], db[peak + 3]) - db[peak]


def main(n=1 << 16, power=0.1, seed=815):
    ctx = ap.Context(0)
    t = np.arange(n)
    x = sum(np.exp(2j * np.pi * k * t / M) for k in TONES).astype(np.complex64)
    capture = ctx.vec(x)
    noise.new(ctx, power, seed).apply(capture)                     # deviation `power` per component (noise.rs:41-42,58)

    # 1: 16 channels, critically sampled; with the -j exponent a tone exp(+2 pi i k t / M) lands in channel k
    bank = ap.Channelizer(ctx, chan.prototype("sinc_hamming", M, P), M)
    y = bank.exec(capture, sign=ap.SIGN_REF_BWD).to_host().reshape(-1, M)[P:]      # past the filter's transient
    chan_db = 10 * np.log10((np.abs(y.astype(np.complex128)) ** 2).mean(axis=0))
    for k, v in enumerate(chan_db):
        print(f"channel {k:2d}: {v:7.2f} dB{'  <- tone' if k in TONES else ''}")
    others = max(v for k, v in enumerate(chan_db) if k not in TONES)
    margin = min(chan_db[k] for k in TONES) - others
    print(f"tone channels exceed every other channel by {margin:.1f} dB")

    # 2: the same capture as a spectrogram; Hann, 50 % overlap against rectangular, disjoint frames
    hann = ap.Channelizer(ctx, chan.prototype("hann", FRAME, 1), FRAME, hop=FRAME // 2)
    usable = n - n % FRAME
    spec = capture.slice(0, usable)
    db_hann = _mean_db(hann.levels(spec, sign=ap.SIGN_REF_BWD, kind=ap.LEVEL_POWER_DB), FRAME)
    db_rect = _mean_db(ap.HipFft(ctx, FRAME).levels(spec, kind=ap.LEVEL_POWER_DB, sign=ap.SIGN_REF_BWD), FRAME)
    tone_bin = TONES[0] * FRAME / M
    leak_hann, leak_rect = _leak(db_hann, tone_bin), _leak(db_rect, tone_bin)
    print(f"leakage three bins off the tone: hann {leak_hann:.1f} dB, rectangular {leak_rect:.1f} dB")
    del bank, hann, capture, spec
    ctx.close()
    return chan_db, margin, leak_hann, leak_rect


if __name__ == "__main__":
    main()
