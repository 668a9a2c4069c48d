#!/usr/bin/env python3
"""Acquire a QPSK burst whose symbol timing, carrier frequency and carrier phase are unknown, without one sample leaving
the device: only bits and 48-byte records are downloaded.

Transmit side: 2048 random bits -> QPSK (the generic table) -> root-raised-cosine pulse (beta 0.35, +-8 symbols, 4 samples
per symbol; taps computed in numpy, applied by `Resampler(4, 1)`) -> a timing offset of 1.3 samples planted with
`ArbResampler` at step 1.0 -> a carrier of 2.3e-3 cycles per sample and 0.11 turns planted with `Nco` -> AWGN at
Es/N0 = 20 dB.

Receive side, the classical feed-forward chain (aether_primitives_amd.sync):
  1. matched filter (`Fir` with the same pulse);
  2. `sync.line(SQUARE)` with the oscillator at -1/4 cycle per sample: the spectral line of |y|^2 at the symbol rate
     (Oerder and Meyr).  The square law does not see the carrier, so timing goes first;
  3. `sync.timing_phase` -> the Q32.32 instant of the first symbol; `ArbResampler` at step 4.0 from there (plus its own
     group delay) leaves one sample per symbol;
  4. `sync.lag(power 4, lag 1)` on the symbols: the angle of sum s[k]^4 conj(s[k-1]^4) is 4 times the carrier's advance
     per symbol (on all four samples per symbol the estimate is too noisy).  `sync.freq_step` is the `Nco` step that
     removes it;
  5. `sync.line(POW4, block = 64)`: 16 block sums of s^4.  The generic table gives s^4 = -4, so a block's carrier phase is
     turns(-S) / 4.  The 16 phases are unwrapped and fitted by a straight line on the host, and a second `Nco` removes the
     fitted phase and the rest of the frequency;
  6. `demod_naive`; the four-fold ambiguity of the fourth power is resolved by the best of the four rotations."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import aether_primitives_amd as ap
from aether_primitives_amd import modulation, noise, nco, resamp, sync

NBITS, SPS, BETA, SPAN = 2048, 4, 0.35, 8
TIMING, FREQ, PHASE, ESN0_DB = 1.3, 2.3e-3, 0.11, 20.0
LOG2_PHASES, TAPS_PER_PHASE = 8, 16
BLOCK = 64                                     # symbols per carrier-phase estimate
EDGE = 16                                      # symbols at either end that are not counted
PAD = 2 * SPAN + 2 * TAPS_PER_PHASE            # zero symbols behind the burst: every filter runs empty


def rrc(t, beta):
    """the root-raised-cosine pulse at the times t (in symbols), f64"""
    t = np.asarray(t, np.float64)
    out = np.empty_like(t)
    for k, x in enumerate(t):
        if abs(x) < 1e-9:
            out[k] = 1 - beta + 4 * beta / np.pi
        elif abs(abs(x) - 1 / (4 * beta)) < 1e-9:
            out[k] = beta / np.sqrt(2) * ((1 + 2 / np.pi) * np.sin(np.pi / (4 * beta)) + (1 - 2 / np.pi) * np.cos(np.pi / (4 * beta)))
        else:
            out[k] = (np.sin(np.pi * x * (1 - beta)) + 4 * beta * x * np.cos(np.pi * x * (1 + beta))) / (np.pi * x * (1 - (4 * beta * x) ** 2))
    return out


def pulse():
    """2 * SPAN * SPS + 1 taps of unit energy, centred"""
    g = rrc(np.arange(-SPAN * SPS, SPAN * SPS + 1) / SPS, BETA)
    return (g / np.sqrt((g * g).sum())).astype(np.float32)


def signed(word):
    """a 64-bit word as a fraction of a turn in [-0.5, 0.5)"""
    return ((int(word) + (1 << 63)) % (1 << 64) - (1 << 63)) / 2.0 ** 64


def main(seed=815, keep=False):
    ctx = ap.Context(0)
    nsym = NBITS // 2
    g = pulse()
    L = 1 << LOG2_PHASES
    interp = resamp.prototype(L, 1, TAPS_PER_PHASE)                   # the interpolator of both ArbResamplers
    arb_delay_q32 = (L * TAPS_PER_PHASE - 1) << (32 - LOG2_PHASES - 1)  # its group delay (T - 1) / (2 L) samples, Q32.32: exact

    # ---- transmit --------------------------------------------------------------------------------------------------
    bits = np.random.default_rng(seed).integers(0, 2, NBITS, dtype=np.uint8)
    m = modulation.qpsk(ctx)
    symbols = ctx.empty(nsym + PAD).vec_zero()
    m.modulate(modulation.DeviceBits(ctx, NBITS, bits), out=symbols.slice(0, nsym))
    shaped = ap.Resampler(ctx, np.concatenate([g, np.zeros(-g.size % SPS, np.float32)]), SPS, 1).exec(symbols)
    # a delay of 4 + TIMING samples: the interpolator delays by its group delay less the phase it starts from
    plant = ap.ArbResampler(ctx, interp, LOG2_PHASES)
    start = arb_delay_q32 - ap.step_word(4 + TIMING)
    rx = plant.exec(shaped, 1 << 32, start)
    ap.Nco(ctx, FREQ, PHASE).mix(rx, out=rx)
    noise.new(ctx, np.sqrt(2.0 / 10 ** (ESN0_DB / 10) / 2), seed).apply(rx)       # Es = 2, N0 = 2 power^2
    # symbol k now peaks behind the matched filter at sample 4 k + delay
    delay = (g.size - 1) + 4 + TIMING                                             # 68 + 1.3: two pulses, the planted delay

    # ---- receive ---------------------------------------------------------------------------------------------------
    y = ap.Fir(ctx, g.astype(np.complex64)).filter(rx)
    _, t_line = sync.line(ctx, y, sync.SQUARE, words=(0, nco.word(-1.0 / SPS), 0))
    t_phase = sync.timing_phase(t_line, SPS)                                      # Q32.32, in [0, SPS)
    timing = t_phase / 2.0 ** 32
    picker = ap.ArbResampler(ctx, interp, LOG2_PHASES)
    per_symbol = picker.exec(y, SPS << 32, t_phase + arb_delay_q32)               # sample j is y(timing + 4 j)
    first = int(round((delay - timing) / SPS))                                    # where the burst begins: the framing is known
    s = per_symbol.slice(first, first + nsym)

    _, f_lag = sync.lag(ctx, s, 4, 1)
    f_step = sync.freq_step(f_lag, 4, 1)
    coarse = ap.Nco.from_words(ctx, step=f_step).mix(s)

    blocks, _ = sync.line(ctx, coarse, sync.POW4, block=BLOCK)
    turns4 = np.array([sync.turns(complex(-r["re"], -r["im"])) for r in blocks])  # 4 x the carrier phase of each block
    turns4 = np.unwrap(turns4, period=1.0)
    centres = (np.arange(blocks.size) + 0.5) * BLOCK - 0.5
    slope, intercept = np.polyfit(centres, turns4 / 4, 1)                         # turns per symbol, turns
    fine = ap.Nco(ctx, -slope, -intercept).mix(coarse)

    errors, rotation = None, 0
    keep_from, keep_to = 2 * EDGE, NBITS - 2 * EDGE
    for k in range(4):
        got = m.demod_naive(ap.Nco(ctx, 0.0, k / 4).mix(fine), compat=False).to_host()
        e = int((got != bits)[keep_from:keep_to].sum())
        if errors is None or e < errors:
            errors, rotation = e, k
    freq = -(signed(f_step) - slope) / SPS                                        # cycles per sample
    print(f"{NBITS} bits, QPSK, {SPS} samples per symbol, Es/N0 {ESN0_DB} dB: timing {timing:.4f} samples (planted {TIMING}, "
          f"line strength {abs(complex(t_line.re, t_line.im)) / t_line.mass:.3f}), carrier {freq:.3e} cycles per sample "
          f"(planted {FREQ}; the lag sum alone {-signed(f_step) / SPS:.3e}), phase {intercept:+.4f} turns at the first symbol, "
          f"rotation {rotation} / 4, bit errors {errors} of {keep_to - keep_from}")
    out = {"errors": errors, "timing": timing, "freq_lag": -signed(f_step) / SPS, "freq": freq, "t_line": t_line, "t_phase": t_phase,
           "f_lag": f_lag, "f_step": f_step, "blocks": blocks}
    if keep:
        out.update(ctx=ctx, y=y, s=s, coarse=coarse)                              # the caller closes the context
        return out
    del plant, picker, y, s, coarse, fine, rx, shaped, symbols, per_symbol
    ctx.close()
    return out


if __name__ == "__main__":
    main()
