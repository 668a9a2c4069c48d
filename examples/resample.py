#!/usr/bin/env python3
"""Take a 48 kHz stream to 44.1 kHz with the polyphase rational resampler.

The reference's rate changes are linear interpolation and sample picking (src/sampling.rs:7-62).  Here a tone at 15 kHz
plus a QPSK burst, sampled at 48 kHz, goes through `Resampler` with up = 147, down = 160 and 16 taps per phase from
`resamp.prototype`, in five chunks; every chunk but the first passes the previous chunk's last `history` samples, so
the pieces are the bits of one call.

The last 0.1 s of the stream holds the tone alone.  A transform of that stretch (4800 points before, 4410 after: 10 Hz per
bin both times, the tone and all its images at bin centres) is read with `stats()`: the peak bin gives the tone's
frequency before and after, and the strongest bin left once the tone's own is masked is the strongest image of the zero
stuffing that the filter let through."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import aether_primitives_amd as ap
from aether_primitives_amd import resamp

FS_IN, UP, DOWN, TAPS_PER_PHASE = 48000, 147, 160, 16
FS_OUT = FS_IN * UP // DOWN                    # 44100
TONE_HZ, TONE_AMP = 15000, 10.0
BIN_HZ = 10
CHUNKS = 5


def _peak(ctx, stretch, fs, skip=None):
    """(frequency in Hz, amplitude) of the strongest bin of `stretch`, a whole number of BIN_HZ periods; `skip`: a bin to mask"""
    n = stretch.n
    spec = ap.HipFft(ctx, n).exec(stretch, ctx.empty(n), ap.SIGN_REF_BWD, ap.Scale.N)
    if skip is not None:
        mask = np.ones(n, np.complex64)
        mask[skip] = 0
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

    rs = ap.Resampler(ctx, resamp.prototype(UP, DOWN, TAPS_PER_PHASE), UP, DOWN)
    out = ctx.empty(rs.out_count(n))
    step = n // CHUNKS // DOWN * DOWN                                 # whole periods per chunk
    pos = 0
    while pos < n:
        end = n if n - pos < 2 * step else pos + step
        hist = stream.slice(pos - rs.history, pos) if pos else None  # the first chunk starts from silence
        rs.exec(stream.slice(pos, end), hist, out.slice(rs.out_count(pos), rs.out_count(end)))
        pos = end
    whole = rs.exec(stream)                                           # the chunks are the bits of one call
    same = bool((out.to_host().view(np.uint32) == whole.to_host().view(np.uint32)).all())

    n_in, n_out = FS_IN // BIN_HZ, FS_OUT // BIN_HZ
    f_in, a_in, _ = _peak(ctx, stream.slice(n - n_in, n), FS_IN)
    f_out, a_out, k_out = _peak(ctx, out.slice(out.n - n_out, out.n), FS_OUT)
    f_img, a_img, _ = _peak(ctx, out.slice(out.n - n_out, out.n), FS_OUT, skip=k_out)
    image_db = 20 * np.log10(max(a_img, 1e-300) / a_out)
    print(f"{n} samples at {FS_IN} Hz -> {out.n} samples at {FS_OUT} Hz in {CHUNKS} chunks (route {rs.route}, tile {rs.tile}); "
          f"chunks equal one call: {same}")
    print(f"tone before {f_in:.1f} Hz (amplitude {a_in:.4f}), after {f_out:.1f} Hz (amplitude {a_out:.4f})")
    print(f"strongest image {image_db:.1f} dB at {f_img:.1f} Hz")
    del rs, out, whole, stream
    ctx.close()
    return f_in, f_out, image_db, f_img, same


if __name__ == "__main__":
    main()
