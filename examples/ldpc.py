#!/usr/bin/env python3
"""An LDPC-coded link end to end on the device: only the decoded bits and one record per codeword leave it.

Transmit: N_CODEWORDS blocks of K information bits -> `Ldpc.encode` with `ldpc.staircase(12, 24, 81)` (N = 1944, K = 972,
rate 1/2) -> QPSK.  Then AWGN.  Receive: `demod_soft` -> `Ldpc.decode` with early stop, at most MAX_ITER iterations of the
layered integer min-sum decoder.  What leaves the device: the K payload bits of every codeword and its record
{iterations, unsatisfied}; a codeword whose record says unsatisfied = 0 satisfies every parity check.

POWER is the noise deviation per component against QPSK symbols (+-1, +-1): Eb/N0 = 1 / POWER^2 at one information bit
per symbol, 6.0 dB.  SOFT_SCALE 4 gives soft values of +-16 at a noise-free symbol, so nothing clamps.  The raw error
count is made on the host from a download of the soft values for that comparison only.

Measured on MI355X (seed 815, 64 codewords): 2774 of 124416 hard decisions in front of the decoder are wrong (2.2 %);
every codeword decodes to the sent bits with unsatisfied = 0, in 1 to 4 iterations.  (At 0.6 per component, 4.4 dB and
4.8 % raw errors, 63 of 64 converge; the last keeps two unsatisfied checks in its parity part after 20 iterations.)"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import aether_primitives_amd as ap
from aether_primitives_amd import ldpc, modulation, noise

SHAPE = (12, 24, 81)
POWER, SOFT_SCALE, MAX_ITER = 0.5, 4.0, 20


def main(n_codewords=64, power=POWER, seed=815):
    ctx = ap.Context(0)
    shift = ldpc.staircase(*SHAPE)
    code = ap.Ldpc(ctx, shift, SHAPE[2])
    m = modulation.qpsk(ctx)
    sent = np.random.default_rng(seed).integers(0, 2, n_codewords * code.k, dtype=np.uint8)
    coded = code.encode(sent)
    x = m.modulate(coded)
    noise.new(ctx, power, seed).apply(x)
    soft = m.demod_soft(x, SOFT_SCALE)
    bits, records = code.decode(soft, max_iter=MAX_ITER, early=True, payload=True)
    got, rec = bits.to_host(), records.to_host()                      # what leaves the device
    soft_host, coded_host = soft.to_host(), coded.to_host()           # for the comparison only
    raw = int(((soft_host < 0) != (coded_host != 0)).sum())
    wrong = int((got != sent).sum())
    print(f"power {power}: {n_codewords} codewords of N = {code.n}, K = {code.k} ({code.group} per workgroup): raw hard-decision errors "
          f"{raw} of {soft_host.size}, errors after decoding {wrong}, codewords with unsatisfied checks "
          f"{int((rec['unsatisfied'] != 0).sum())}, iterations {int(rec['iterations'].min())} .. {int(rec['iterations'].max())}")
    res = dict(shift=shift, z=SHAPE[2], sent=sent, coded=coded_host, soft=soft_host, bits=got, records=rec, raw=raw, wrong=wrong)
    code.close()
    ctx.close()
    return res


if __name__ == "__main__":
    main()
