#!/usr/bin/env python3
"""Take a 48 kHz stream to a 44.1 kHz clock that runs 20 parts per million fast, with the arbitrary-ratio resampler.

The reference's rate changes are linear interpolation and sample picking (src/sampling.rs:7-62), and the rational
resampler (examples/resample.py) needs up / down as small integers: 48000 / (44100 * 1.00002) is no such fraction.  Here
the signal of examples/resample.py, a tone at 15 kHz plus a QPSK burst, goes through `ArbResampler` with 256 phases of 16
taps from `resamp.prototype` and the step word of that ratio, in chunks of uneven length (one of a single sample); every
chunk but the first passes the previous chunk's last `history` samples, and the object carries the phase, so the pieces
are the bits of one call.

The last 0.1 s of the stream holds the tone alone.  A transform of that stretch (4800 points before, 4410 after) under a
four-term Blackman-Harris window (side lobes below -92 dB: after the conversion the tone no longer sits on a bin centre)
is read with `stats()`: the peak bin gives the tone's frequency before and after, and the strongest bin outside the
window's main lobe around the tone is the strongest spur: what the filter left of the images, and what the linear
interpolation between phases adds."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import aether_primitives_amd as ap
from aether_primitives_amd import resamp

FS_IN, FS_NOMINAL, PPM = 48000, 44100, 20
FS_OUT = FS_NOMINAL * (1 + PPM * 1e-6)         # 44100.882 Hz
LOG2_PHASES, TAPS_PER_PHASE = 8, 16
TONE_HZ, TONE_AMP = 15000, 10.0
BIN_HZ = 10
CHUNKS = (4801, 9973, 1, 14407, 7000)          # input samples; the rest of the stream is the last chunk
MAIN_LOBE = 4                                  # bins on each side of a peak that a four-term Blackman-Harris window fills


def _window(n):
    k = np.arange(n)
    a = (0.35875, 0.48829, 0.14128, 0.01168)
    w = a[0] - a[1] * np.cos(2 * np.pi * k / n) + a[2] * np.cos(4 * np.pi * k / n) - a[3] * np.cos(6 * np.pi * k / n)
    return (w / a[0]).astype(np.complex64)     # a tone on a bin centre keeps its amplitude


def _peak(ctx, stretch, fs, around=None):
    """(frequency in Hz, amplitude, bin) of the strongest bin of the windowed `stretch`; `around`: a bin whose main lobe is masked"""
    n = stretch.n
    seen = ctx.empty(n).vec_clone(stretch).vec_mul(_window(n))
    spec = ap.HipFft(ctx, n).exec(seen, ctx.empty(n), ap.SIGN_REF_BWD, ap.Scale.N)
    if around is not None:
        mask = np.ones(n, np.complex64)
        mask[(around + np.arange(-MAIN_LOBE, MAIN_LOBE + 1)) % n] = 0
        spec.vec_mul(mask)
    st = spec.stats()
    k = st.max_index if st.max_index < n // 2 else st.max_index - n
    return k * fs / n, float(st.max_norm), st.max_index


def main(seconds=1, seed=815):
    ctx = ap.Context(0)
    n = seconds * FS_IN
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    qpsk = ((2 * rng.integers(0, 2, n) - 1) + 1j * (2 * rng.integers(0, 2, n) - 1)) / np.sqrt(2)
    qpsk[:n // 8] = 0
    qpsk[n // 2:] = 0                                                 # a burst: the tone is alone in the second half
    x = (qpsk + TONE_AMP * np.exp(2j * np.pi * TONE_HZ * t / FS_IN)).astype(np.complex64)
    stream = ctx.vec(x)

    step = ap.step_word(FS_IN / FS_OUT)                               # input samples per output sample, Q32.32
    L = 1 << LOG2_PHASES
    rs = ap.ArbResampler(ctx, resamp.prototype(L, -(-L * step >> 32), TAPS_PER_PHASE), LOG2_PHASES)
    total, _ = rs.advance(step, 0, n)
    out = ctx.empty(total)
    pos, made, lengths = 0, 0, []
    for length in CHUNKS + (n - sum(CHUNKS),):
        hist = stream.slice(pos - rs.history, pos) if pos else None  # the first chunk starts from silence
        count, _ = rs.advance(step, rs.phase, length)
        rs.exec(stream.slice(pos, pos + length), step, hist=hist, out=out.slice(made, made + count))
        pos, made = pos + length, made + count
        lengths.append(count)
    whole = rs.exec(stream, step, 0)                                  # the chunks are the bits of one call
    same = made == total and bool((out.to_host().view(np.uint32) == whole.to_host().view(np.uint32)).all())

    n_in, n_out = FS_IN // BIN_HZ, FS_NOMINAL // BIN_HZ
    f_in, a_in, _ = _peak(ctx, stream.slice(n - n_in, n), FS_IN)
    f_out, a_out, k_out = _peak(ctx, out.slice(out.n - n_out, out.n), FS_OUT)
    f_spur, a_spur, _ = _peak(ctx, out.slice(out.n - n_out, out.n), FS_OUT, around=k_out)
    spur_db = 20 * np.log10(max(a_spur, 1e-300) / a_out)
    print(f"{n} samples at {FS_IN} Hz -> {out.n} samples at {FS_OUT:.3f} Hz (step {step} / 2^32) in chunks making {lengths} "
          f"(route {rs.route(step)}, tile {rs.tile(step)}); chunks equal one call: {same}")
    print(f"tone before {f_in:.1f} Hz (amplitude {a_in:.4f}), after {f_out:.1f} Hz in bin {k_out} (amplitude {a_out:.4f})")
    print(f"strongest spur {spur_db:.1f} dB at {f_spur:.1f} Hz")
    del rs, out, whole, stream
    ctx.close()
    return f_in, f_out, k_out, spur_db, f_spur, same


if __name__ == "__main__":
    main()
