#!/usr/bin/env python3
"""Bring a channel at an offset to baseband with the oscillator, then decimate it.

The reference has no frequency shift.  Here a QPSK burst sits at +0.2 cycles per sample beside a tone at -0.1.
`Nco(freq=-0.2)` mixes the stream down in chunks of uneven length (the position carries over, so the pieces are the bits
of one call), and `Resampler(1, 4, 16)` keeps every fourth sample behind its 16-tap low-pass.  The burst comes out
centred on zero; the tone moves to -0.3 cycles per sample, into the filter's stop band, and what is left of it lands at
-0.2 cycles per output sample.

The last stretch of the stream holds the tone alone.  A transform of that stretch before the mixer (4096 points) and
behind the resampler (1024 points) is read with `stats()`: the peak bin gives the tone's frequency before and after.
The burst holds each symbol for 32 samples; the output samples whose 16 taps lie inside one symbol are compared with
that symbol (EVM).  The same composite signal planted WITHOUT the offset, through the same resampler and no mixer, gives
the EVM that the filter and the tone's leakage leave on their own: the shifter must not add to it."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import aether_primitives_amd as ap
from aether_primitives_amd import resamp

OFFSET, TONE, TONE_AMP = 0.2, -0.1, 4.0          # cycles per sample
DOWN, TAPS = 4, 16
N, SYMBOL, BURST_AT, SYMBOLS = 32768, 32, 4096, 256
N_BEFORE, N_AFTER = 4096, 1024                   # transform lengths: the same stretch before and after
CHUNKS = (1000, 1, 4099, 2, 12345)               # samples per mixer call; the rest goes in one more


def wrap(f):
    """a frequency in cycles per sample -> [-0.5, 0.5)"""
    return (f + 0.5) % 1.0 - 0.5


def _peak(ctx, stretch):
    """(frequency in cycles per sample, amplitude) of the strongest bin of `stretch`"""
    n = stretch.n
    st = ap.HipFft(ctx, n).exec(stretch, ctx.empty(n), ap.SIGN_REF_BWD, ap.Scale.N).stats()
    k = st.max_index if st.max_index < n // 2 else st.max_index - n
    return k / n, float(st.max_norm)


def _evm_db(out, symbols):
    """the output samples whose taps lie inside one symbol, against that symbol"""
    per = SYMBOL // DOWN                                               # output samples per symbol
    first = -(-(TAPS - 1) // DOWN)                                     # the first output of a symbol that reads no older one
    k = BURST_AT // DOWN + per * np.arange(SYMBOLS)[:, None] + np.arange(first, per)[None, :]
    want = np.repeat(symbols[:, None], per - first, axis=1)
    return ap.evm_db(out[k].reshape(-1), want.reshape(-1))


def main(seed=815):
    ctx = ap.Context(0)
    rng = np.random.default_rng(seed)
    t = np.arange(N)
    symbols = ((2 * rng.integers(0, 2, SYMBOLS) - 1) + 1j * (2 * rng.integers(0, 2, SYMBOLS) - 1)) / np.sqrt(2)
    burst = np.zeros(N, np.complex128)
    burst[BURST_AT:BURST_AT + SYMBOLS * SYMBOL] = np.repeat(symbols, SYMBOL)
    # what an ideal receiver sees at baseband; the stream carries it OFFSET higher
    base = burst + TONE_AMP * np.exp(2j * np.pi * (TONE - OFFSET) * t)
    stream = ctx.vec((base * np.exp(2j * np.pi * OFFSET * t)).astype(np.complex64))

    osc = ap.Nco(ctx, freq=-OFFSET)
    tuned = ctx.empty(N)
    pos = 0
    for c in CHUNKS + (N - sum(CHUNKS),):
        osc.mix(stream.slice(pos, pos + c), tuned.slice(pos, pos + c))
        pos += c
    whole = ap.Nco(ctx, freq=-OFFSET).mix(stream)                      # the chunks are the bits of one call
    same = bool((tuned.to_host().view(np.uint32) == whole.to_host().view(np.uint32)).all())

    rs = ap.Resampler(ctx, resamp.prototype(1, DOWN, TAPS), 1, DOWN)
    out = rs.exec(tuned)
    plain = rs.exec(ctx.vec(base.astype(np.complex64)))                 # no offset, no mixer

    f_in, a_in = _peak(ctx, stream.slice(N - N_BEFORE, N))
    f_out, a_out = _peak(ctx, out.slice(out.n - N_AFTER, out.n))
    evm, evm_plain = _evm_db(out.to_host(), symbols), _evm_db(plain.to_host(), symbols)
    print(f"{N} samples mixed by {-OFFSET} cycles per sample in {len(CHUNKS) + 1} chunks; chunks equal one call: {same}")
    print(f"tone before {f_in:+.5f} cycles per sample (amplitude {a_in:.4f}), after {f_out:+.5f} cycles per output sample "
          f"(amplitude {a_out:.5f}); the shift puts it at {wrap((TONE - OFFSET) * DOWN):+.5f}")
    print(f"burst EVM {evm:.2f} dB; without the offset and without the mixer {evm_plain:.2f} dB")
    del rs, out, plain, tuned, whole, stream, osc
    ctx.close()
    return f_in, f_out, evm, evm_plain, same


if __name__ == "__main__":
    main()
