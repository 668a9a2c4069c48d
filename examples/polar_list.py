#!/usr/bin/env python3
"""A CRC-aided polar list decoder end to end on the device: only the picked rows' numbers and payloads leave it.

The link, seed and frame count are those of examples/polar.py: N_FRAMES frames of 240 payload bits -> `Crc.attach`
(crc-16/xmodem) gives K = 256 -> `Polar.encode` with `polar.mask(9, 256)` (N = 512, rate 1/2) -> QPSK -> AWGN ->
`demod_soft`.  Then for L = 1, 2, 4, 8, one decode each: `PolarList.decode(all=True)` gives the L paths of every frame in
the order of their metrics -> `Crc.check` over the F L rows strips the payloads and gives F L `diff` words -> `polar.pick`
takes, per frame, the first row whose word is zero (row 0 when none is).  What leaves the device: `which` and the picked
payloads.  The count "wrong if row 0 is taken" is made on the host from a download of all rows, for that comparison only.

Measured on MI355X (seed 815, 256 frames; the soft values are those of examples/polar.py, where 40 frames fail plain
successive cancellation and 23 still fail after four flip rounds), per L = 1, 2, 4, 8: frames with no row passing the CRC
40, 11, 4, 3; wrong payloads after the pick 40, 11, 4, 3; wrong payloads if row 0 is taken 40, 16, 13, 13.  Every frame
whose picked payload is the sent one was called good.  (A numpy simulation of the same code at the same deviation with its
own noise: 37, 6, 2, 1 frames failing.)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import aether_primitives_amd as ap
from aether_primitives_amd import modulation, noise, polar

N_LOG2, PAYLOAD, CRC = 9, 240, "crc-16/xmodem"
POWER, SOFT_SCALE = 0.8, 6.0
LISTS = (1, 2, 4, 8)


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

    want = sent.reshape(n_frames, PAYLOAD)
    lists = {}
    for L in LISTS:
        dec = ap.PolarList(ctx, N_LOG2, msk, L)
        rows, records = dec.decode(soft, all=True)                    # F L rows of K bits, best metric first
        diff, payloads, _ = crc.check(rows, PAYLOAD, summary=False)   # F L words, F L payloads
        picked, which = polar.pick(ctx, payloads, PAYLOAD, L, diff)
        which_host = which.to_host()                                  # what leaves the device
        got = picked.to_host().reshape(n_frames, PAYLOAD)
        none = int((which_host == polar.NONE).sum())
        wrong = int((got != want).any(axis=1).sum())
        rows_host = rows.to_host().reshape(n_frames, L, K)            # for the comparison (and the test) only
        wrong0 = int((rows_host[:, 0, :PAYLOAD] != want).any(axis=1).sum())
        print(f"L = {L} ({dec.lanes} lanes per path, {dec.group} codewords per workgroup): frames with no row passing the CRC {none}; "
              f"wrong payloads after the pick {wrong}; wrong payloads if row 0 is taken {wrong0}")
        lists[L] = dict(rows=rows_host, records=records.to_host(), which=which_host, payload=got, none=none, wrong=wrong, wrong0=wrong0)
        dec.close()
    sc_bits, _ = code.decode(soft, records=False)
    sc_wrong = int((sc_bits.to_host().reshape(n_frames, K)[:, :PAYLOAD] != want).any(axis=1).sum())
    res = dict(n=N_LOG2, mask=msk, sent=sent, soft=soft.to_host(), lists=lists, sc_wrong=sc_wrong)
    code.close()
    crc.close()
    ctx.close()
    return res


if __name__ == "__main__":
    main()
