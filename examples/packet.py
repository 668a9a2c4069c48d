#!/usr/bin/env python3
"""Packets with a frame check end to end on the device: only the verdict and the good payloads leave it.

Transmit, per frame of N_BYTES payload bytes:
  1. `unpack_bits` LSB first: 8 N_BYTES bits, one byte each;
  2. `Crc.named("crc-32").attach`: the 32 bits of the 802.3 / 802.11 FCS behind every frame;
  3. `Sequence.scramble` with x^7 + x^4 + 1 over the whole stream;
  4. `ConvCode` K = 7 (0o133, 0o171), rate 1/2;
  5. QPSK.
Then AWGN.  Receive: `demod_soft`, `ConvCode.decode_stream`, the scrambler again, and ONE `Crc.check` that compares every
frame's check bits and strips the payload, which `pack_bits` packs LSB first.  What leaves the device: the two words of the
summary, one `diff` word per frame, and the packed payload of every frame whose diff is 0.

It runs at two noise levels.  POWERS is the noise deviation per component against QPSK symbols (+-1, +-1): Eb/N0 =
1 / POWER^2 at one data bit per symbol, 10.5 dB and 3.1 dB.  Per level it prints the frames the CRC calls bad beside the
frames whose decoded bits differ from the sent ones (counted on the host from a download made for that comparison only):
over the whole frame, and over the payload alone -- an error burst that falls into the 32 check bits makes a bad frame with
an intact payload.

Measured on MI355X (seed 815, 256 frames of 256 bytes): at 0.3 no frame is bad; at 0.7 the CRC calls 33 frames bad (the
first is frame 12), the same 33 whose decoded bits differ from the sent ones, 32 of them in the payload and one only in its
check bits; the packed payloads of the other 223 equal the sent bytes."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import aether_primitives_amd as ap
from aether_primitives_amd import crc, modulation, noise

N_BYTES = 256
POLYS = (0o133, 0o171)
SCRAMBLER, SCRAMBLER_INIT = (4, 7), 0b1011101                       # s[n] = s[n - 4] ^ s[n - 7]
POWERS, SOFT_SCALE = (0.3, 0.7), 8.0                                # L = 8 (d1^2 - d0^2): +-32 at a noise-free symbol


def run(ctx, parts, data, n_frames, n_bytes, awgn):
    """-> what left the device: summary, diff words, {frame: payload bytes} of the good frames; and, for the comparison
    only, the decoded frames"""
    fcs, scr, code, m = parts
    L = 8 * n_bytes
    bits = ap.unpack_bits(ap.DeviceBits(ctx, data.size, data), crc.LSB_FIRST)
    framed = fcs.attach(bits, L)
    x = m.modulate(code.encode(scr.scramble(SCRAMBLER_INIT, framed)))
    awgn.apply(x)
    decoded = scr.scramble(SCRAMBLER_INIT, code.decode_stream(m.demod_soft(x, SOFT_SCALE)))
    diff, payload, summary = fcs.check(decoded, L, summary="host")
    packed = ap.pack_bits(payload, crc.LSB_FIRST)
    diff = diff.to_host()
    good = {}
    for f in np.flatnonzero(diff == 0):
        good[int(f)] = np.empty(n_bytes, np.uint8)
        ctx.download(packed.ptr + int(f) * n_bytes, good[int(f)])
    return summary, diff, good, decoded.to_host().reshape(n_frames, L + fcs.r), framed.to_host().reshape(n_frames, L + fcs.r)


def main(n_frames=256, n_bytes=N_BYTES, powers=POWERS, seed=815):
    ctx = ap.Context(0)
    parts = (ap.Crc.named(ctx, "crc-32"), ap.Sequence(ctx, SCRAMBLER), ap.ConvCode(ctx, 7, POLYS), modulation.qpsk(ctx))
    data = np.random.default_rng(seed).integers(0, 256, n_frames * n_bytes, dtype=np.uint8)
    results = []
    for i, power in enumerate(powers):
        summary, diff, good, decoded, framed = run(ctx, parts, data, n_frames, n_bytes, noise.new(ctx, power, seed + i))
        differ = (decoded != framed).any(axis=1)                      # the frame as sent: payload and check bits
        differ_payload = (decoded[:, :8 * n_bytes] != framed[:, :8 * n_bytes]).any(axis=1)
        ok = all(payload.tobytes() == data[f * n_bytes:(f + 1) * n_bytes].tobytes() for f, payload in good.items())
        print(f"power {power}: {n_frames} frames of {n_bytes} bytes + FCS: bad by CRC {summary[0]} (first {summary[1]}), "
              f"decoded frame differs in {int(differ.sum())} (payload in {int(differ_payload.sum())}), good payloads equal the sent bytes: {ok}")
        results.append(dict(power=power, summary=summary, diff=diff, good=good, differ=differ, differ_payload=differ_payload, data=data))
    ctx.close()
    return results


if __name__ == "__main__":
    main()
