#!/usr/bin/env python3
"""Forward error correction on the device: 2^16 random bits -> K = 7 rate 1/2 convolutional code (0o171, 0o133) -> QPSK
with AWGN in one pass -> soft demodulation -> Viterbi decoder, the bits never leaving the device in between.

Beside the decoded bit errors it counts the raw hard-decision errors of the coded bits, i.e. what the channel did, and
runs the same chain without noise.  The noise power 0.63 is the per-component noise deviation against symbols of
+-1 per component (the library's Awgn scales twice, as the reference does): the raw error share is Q(1 / 0.63), about
5.6 %, which is 4 dB Eb/N0 at rate 1/2."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import aether_primitives_amd as ap
from aether_primitives_amd import modulation, noise

K, POLYS = 7, (0o171, 0o133)
POWER, SOFT_SCALE = 0.63, 8.0                  # L = 4 * component * scale: +-32 at the noise-free points


def chain(ctx, code, m, bits, awgn):
    """-> (decoded bits, hard decisions of the coded bits, the coded bits), all on the host"""
    coded = code.encode(modulation.DeviceBits(ctx, bits.size, bits))
    rx = m.modulate_awgn(coded, awgn) if awgn is not None else m.modulate(coded)
    soft = m.demod_soft(rx, SOFT_SCALE)
    decoded = code.decode_stream(soft)                               # +127 history, flush, delay removed
    return decoded.to_host(), m.demod_naive(rx, compat=False).to_host(), coded.to_host()


def main(nbits=1 << 16, power=POWER, seed=815):
    ctx = ap.Context(0)
    code = ap.ConvCode(ctx, K, POLYS)                                # block 512, warm-up 64, traceback 64
    m = modulation.qpsk(ctx)
    bits = np.random.default_rng(seed).integers(0, 2, nbits, dtype=np.uint8)
    clean, _, _ = chain(ctx, code, m, bits, None)
    decoded, hard, coded = chain(ctx, code, m, bits, noise.new(ctx, power, seed))
    raw, errors, quiet = int((hard != coded).sum()), int((decoded != bits).sum()), int((clean != bits).sum())
    print(f"{nbits} bits, K = {K} rate 1/{len(POLYS)}, QPSK + AWGN(power {power}): raw errors {raw} of {coded.size} coded bits "
          f"({100.0 * raw / coded.size:.2f} %), decoded errors {errors}, noise-free errors {quiet}")
    return errors


if __name__ == "__main__":
    main()
