#!/usr/bin/env python3
"""A CRC-aided SC-Flip polar link end to end on the device: only CRC verdicts, records and the final payloads leave it.

Transmit: N_FRAMES frames of 240 payload bits -> `Crc.attach` (crc-16/xmodem, the 0x1021 polynomial) gives K = 256 ->
`Polar.encode` with `polar.mask(9, 256)` (N = 512, rate 1/2) -> QPSK.  Then AWGN.  Receive: `demod_soft` -> `Polar.decode`
with records -> `Crc.check`.  Then up to four more rounds: in round r a frame whose `diff` word is still non-zero is
decoded with flip = index[r - 1] of its first-pass record, the r-th least reliable information decision of plain
successive cancellation; every other frame keeps the flip it was last decoded with (none for a frame that passed at
once), so a frame once repaired stays repaired.  Every round decodes all frames.  What leaves the device: the `diff` words
of every round, the first pass's records and the final payloads.

POWER is the noise deviation per component against QPSK symbols (+-1, +-1): Eb/N0 = 1 / POWER^2 at one information bit
per symbol, 1.9 dB.  SOFT_SCALE 6 gives soft values of +-24 at a noise-free symbol.  The raw error count is made on the
host from a download of the soft values for that comparison only.

Measured on MI355X (seed 815, 256 frames): 13932 of 131072 hard decisions in front of the decoder are wrong (10.6 %);
40 frames fail the CRC after plain successive cancellation, 33, 28, 26 and 23 after the four flip rounds, so four flips
repair 17 of the 40; in every round the frames the CRC calls good are exactly those whose payload is the sent one.  (A
numpy simulation of the same code at the same deviation with its own noise: 29 of 300 fail, four flips repair 16.)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import aether_primitives_amd as ap
from aether_primitives_amd import modulation, noise, polar

N_LOG2, PAYLOAD, CRC = 9, 240, "crc-16/xmodem"
POWER, SOFT_SCALE, ROUNDS = 0.8, 6.0, 4


def main(n_frames=256, power=POWER, seed=815):
    ctx = ap.Context(0)
    crc = ap.Crc.named(ctx, CRC)
    K = PAYLOAD + crc.r
    msk = polar.mask(N_LOG2, K)
    code = ap.Polar(ctx, N_LOG2, msk)
    m = modulation.qpsk(ctx)
    sent = np.random.default_rng(seed).integers(0, 2, n_frames * PAYLOAD, dtype=np.uint8)
    coded = code.encode(crc.attach(sent, PAYLOAD))
    x = m.modulate(coded)
    noise.new(ctx, power, seed).apply(x)
    soft = m.demod_soft(x, SOFT_SCALE)

    flip = np.full(n_frames, polar.NONE, np.uint32)
    rounds = []                                                       # per round: flips used, diff words, (bits, records: the test's)
    first = None
    for r in range(ROUNDS + 1):
        bits, records = code.decode(soft, flip=None if r == 0 else flip, records=True)
        diff, payload, _ = crc.check(bits, PAYLOAD, summary=False)
        bad = diff.to_host() != 0                                     # what leaves the device in every round
        if r == 0:
            first = records.to_host()
        rounds.append(dict(flip=flip.copy(), bad=bad, bits=bits, records=records))
        if r == ROUNDS or not bad.any():
            break
        flip = np.where(bad, first["index"][:, r], flip).astype(np.uint32)
    got = payload.to_host().reshape(n_frames, PAYLOAD)               # the final payloads

    soft_host, coded_host = soft.to_host(), coded.to_host()           # for the comparison only
    raw = int(((soft_host < 0) != (coded_host != 0)).sum())
    failed = [int(rd["bad"].sum()) for rd in rounds]
    wrong = int((got != sent.reshape(n_frames, PAYLOAD)).any(axis=1).sum())
    print(f"power {power}: {n_frames} frames of {PAYLOAD} + {crc.r} bits in N = {code.n} ({code.lanes} lanes per codeword, {code.group} "
          f"codewords per workgroup): raw hard-decision errors {raw} of {soft_host.size}; frames failing the CRC after plain SC "
          f"{failed[0]}, after each flip round {failed[1:]}; frames with a wrong payload at the end {wrong}")
    for rd in rounds:                                                 # for the test only: every round's bytes
        rd["bits"], rd["records"] = rd["bits"].to_host(), rd["records"].to_host()
    res = dict(n=N_LOG2, mask=msk, sent=sent, coded=coded_host, soft=soft_host, rounds=rounds, payload=got, raw=raw, failed=failed, wrong=wrong)
    code.close()
    crc.close()
    ctx.close()
    return res


if __name__ == "__main__":
    main()
