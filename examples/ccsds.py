#!/usr/bin/env python3
"""The classic concatenated link on the device: payload bytes -> RS(255, 223), symbol-interleaved to depth 4 (the CCSDS
frame) -> bits -> K = 7 rate 1/2 convolutional code (0o171, 0o133) -> QPSK + AWGN -> soft demodulation -> Viterbi decoder
-> bytes -> Reed-Solomon decoder.  Only the payload, the records and the summary leave the device.

A Viterbi decoder fails in bursts of a few bytes; the interleaver deals them out over four codewords and the outer code
repairs up to 16 bytes in each.  The records say what the Viterbi decoder left behind: `corrected` is the number of
byte errors of a codeword.

The noise.  POWER is the per-component noise deviation against symbols of +-1 per component (examples/fec.py).  It was
chosen with the CPU restatement of the inner code (tests/cc_truth.py, the same frames, numpy noise, three seeds): at 0.66
the Viterbi decoder leaves one wrong byte in sixteen codewords or none, at 0.78 between 0 and 7 in every codeword (40 to
46 in all), at 0.82 up to 13, and from 0.86 on single codewords pass 16.  0.78 keeps every codeword well inside the bound
and leaves none of the three runs without errors (the device's own noise: 26 wrong bytes, at most 4 in a codeword)."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import aether_primitives_amd as ap
from aether_primitives_amd import crc, modulation, noise

CODE, DEPTH = "ccsds-255-223", 4
K, POLYS = 7, (0o171, 0o133)
POWER, SOFT_SCALE = 0.78, 8.0                  # L = 4 * component * scale: +-32 at the noise-free points
FRAMES = 4


def main(power=POWER, frames=FRAMES, seed=815, diagnose=False):
    """-> dict(sent, payload, records, summary); with diagnose=True also `received` and `coded`, the frames behind the
    Viterbi decoder and as sent, for a test that counts the byte errors itself"""
    ctx = ap.Context(0)
    outer = ap.Rs(ctx, CODE)
    inner = ap.ConvCode(ctx, K, POLYS)                                   # block 512, warm-up 64, traceback 64
    m = modulation.qpsk(ctx)
    sent = np.random.default_rng(seed).integers(0, 256, frames * DEPTH * outer.k, dtype=np.uint8)
    coded = outer.encode(sent, depth=DEPTH)                              # frames of 4 * 255 bytes
    bits = crc.unpack_bits(coded)
    rx = m.modulate_awgn(inner.encode(bits), noise.new(ctx, power, seed))
    decoded = inner.decode_stream(m.demod_soft(rx, SOFT_SCALE))
    received = crc.pack_bits(decoded)
    payload, records, summary = outer.decode(received, depth=DEPTH, payload=True)
    res = dict(sent=sent, payload=payload.to_host(), records=records.to_host(), summary=summary.to_host())
    if diagnose:
        res.update(received=received.to_host(), coded=coded.to_host())
    rec = res["records"]
    wrong = int((res["payload"] != sent).sum())
    print(f"{frames} frames of {DEPTH} x RS(255, 223) behind K = {K} rate 1/{len(POLYS)}, QPSK + AWGN(power {power}): the Viterbi decoder left "
          f"{int(rec['corrected'].sum())} wrong bytes in {int((rec['corrected'] != 0).sum())} of {rec.size} codewords (at most "
          f"{int(rec['corrected'].max())} in one); {int(res['summary']['n_failed'])} codewords failed, {wrong} payload bytes wrong")
    outer.close()
    ctx.close()
    return res


if __name__ == "__main__":
    main()
