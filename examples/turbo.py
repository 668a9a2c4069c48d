#!/usr/bin/env python3
"""An LTE-style turbo link end to end on the device: only records, CRC verdicts and the payloads of good frames leave it.

Transmit: N_FRAMES frames of 488 payload bits -> `Crc.attach` (crc-24/lte-a) gives K = 512 -> `Turbo.encode` with
`turbo.named("lte")`, `turbo.qpp(512, 31, 64)`, windows of 32 steps and a warm-up of 16 (N = 1548, rate 1/3 with the
tails) -> QPSK.  Then AWGN.  Receive: `demod_soft` -> `Turbo.decode` with early stop at max_iter = 1, 2, 4 and 8 ->
`Crc.check`.  What leaves the device: the records and `diff` words of every round and the final payloads.

POWER is the noise deviation per component against QPSK symbols (+-1, +-1); SOFT_SCALE 4 gives soft values of +-16 at a
noise-free symbol.  The level was chosen on the host from the restatement alone (tests/turbo_truth.py, numpy noise,
seeds 5, 815 and 816): at 1.0 nearly every frame is right after two iterations, at 1.2 more than half still fail after
eight, at 1.1 all but 0 .. 3 of 64 frames fail the first iteration and at most 3 the eighth, and the mean number of
iterations with early stop is 3.3 .. 4.0.  The raw error count is made on the host from a download of the soft values for
that comparison only."""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import aether_primitives_amd as ap
from aether_primitives_amd import modulation, noise, turbo

K, PAYLOAD, CRC = 512, 488, "crc-24/lte-a"
CODE, F1, F2, WINDOW, WARMUP = "lte", 31, 64, 32, 16
POWER, SOFT_SCALE, ROUNDS = 1.1, 4.0, (1, 2, 4, 8)


def main(n_frames=64, power=POWER, seed=815):
    ctx = ap.Context(0)
    crc = ap.Crc.named(ctx, CRC)
    assert PAYLOAD + crc.r == K
    pi = turbo.qpp(K, F1, F2)
    code = ap.Turbo(ctx, CODE, pi, WINDOW, WARMUP)
    m = modulation.qpsk(ctx)
    sent = np.random.default_rng(seed).integers(0, 2, n_frames * PAYLOAD, dtype=np.uint8)
    coded = code.encode(crc.attach(sent, PAYLOAD))
    x = m.modulate(coded)
    noise.new(ctx, power, seed).apply(x)
    soft = m.demod_soft(x, SOFT_SCALE)

    rounds = []                                                       # per round: max_iter, diff words, records (bits: the test's)
    for max_iter in ROUNDS:
        bits, records = code.decode(soft, max_iter=max_iter, early=True)
        diff, payload, _ = crc.check(bits, PAYLOAD, summary=False)
        rounds.append(dict(max_iter=max_iter, bad=diff.to_host() != 0, records=records.to_host(), bits=bits))
    good = ~rounds[-1]["bad"]
    got = payload.to_host().reshape(n_frames, PAYLOAD)               # the final payloads; only the good frames' are used

    soft_host, coded_host = soft.to_host(), coded.to_host()           # for the comparison only
    raw = int(((soft_host < 0) != (coded_host != 0)).sum())
    failed = [int(rd["bad"].sum()) for rd in rounds]
    mean_iter = [float(rd["records"]["iterations"].mean()) for rd in rounds]
    wrong = int((got[good] != sent.reshape(n_frames, PAYLOAD)[good]).any(axis=1).sum())
    print(f"power {power}: {n_frames} frames of {PAYLOAD} + {crc.r} bits in N = {code.n} ({code.windows} windows per codeword, {code.group} "
          f"codewords per workgroup): raw hard-decision errors {raw} of {soft_host.size}; frames failing the CRC at max_iter {list(ROUNDS)}: "
          f"{failed}; mean iterations {[round(v, 2) for v in mean_iter]}; good frames with a wrong payload {wrong}")
    for rd in rounds:                                                 # for the test only: every round's bytes
        rd["bits"] = rd["bits"].to_host()
    res = dict(pi=pi, sent=sent, coded=coded_host, soft=soft_host, rounds=rounds, payload=got, raw=raw, failed=failed, mean_iter=mean_iter,
               wrong=wrong)
    code.close()
    crc.close()
    ctx.close()
    return res


if __name__ == "__main__":
    main()
