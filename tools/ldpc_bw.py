#!/usr/bin/env python3
"""Speed of the LDPC kernels (csrc/aeth_ldpc.hip).

Device events around every call, 5 warm-up rounds, REPS (>= 20) timed rounds; the paths alternate inside a round and
rotate over four sets of buffers.  Every path handles about 2^24 information bits (whole codewords).  Per path: median
and min-max in us.

    path                               reported as                            yardstick
    decode (r, c, z), 10 iterations    Gbit/s of information at the median    the issue-rate model below
    decode (12, 24, 81), early stop    the same, at the noise of examples/ldpc.py (soft values made on the device)
    encode (12, 24, 81)                Gbit/s of information                  aeth_copy_dev of its K + N bytes per codeword
    aeth_cc_decode K = 7 (512, 64, 64) Gbit/s of information on the same bit count

The decoder is bound by instruction issue and LDS latency, not by memory (N bytes in, N out per codeword).  The model
counts the layer loop of the shipped code object (llvm-objdump -d of the gfx950 image, ldpc_decode_kernel, the two inner
loops of a layer): per edge the first pass (minima, argmin, sign parity) is 18 VALU instructions, two LDS reads and one
scalar load, the second (write back) 16 VALU instructions, two LDS reads, two LDS writes and one scalar load: 34 VALU and
6 LDS instructions per edge and iteration.  A wave64 VALU instruction occupies its SIMD for 2 cycles, so a wave retires
an edge of 64 checks per 68 cycles at best.  A codeword has E z edge-checks per iteration; 1024 SIMDs at 2.4 GHz then do
1024 * 2.4e9 * 64 / (68 E z) codeword-iterations per second, K information bits each -- before the dependent LDS reads
(each pass waits for its Q value before it can compare), the scalar load's wait, the barrier per layer and the syndrome
pass are counted.

Nothing here is a condition; the numbers are reported as they come (profiles/ldpc_bw.txt)."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aether_primitives_amd as ap                                       # noqa: E402
from aether_primitives_amd import _lib, ldpc, modulation, noise          # noqa: E402
from aether_primitives_amd.modulation import DeviceBits, DeviceSoft      # noqa: E402

WARMUP = 5
NSETS = 4
ITERS = 10
EXAMPLE_POWER, EXAMPLE_SCALE = 0.5, 4.0                                  # examples/ldpc.py
VALU_PER_EDGE = 34


def measure(ctx, calls, reps):
    """calls: [(name, fn(i))]; -> {name: [ms per call]}; the calls alternate inside every round"""
    e0, e1 = ctx.event(), ctx.event()
    out = {name: [] for name, _ in calls}
    for r in range(WARMUP + reps):
        for name, fn in calls:
            e0.record()
            fn(r)
            e1.record()
            e1.sync()
            if r >= WARMUP:
                out[name].append(e0.elapsed_ms(e1))
    return out


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--reps", type=int, default=20)
    ap_.add_argument("--log2n", type=int, default=24)
    args = ap_.parse_args()
    reps = max(args.reps, 20)
    ctx = ap.Context(0)
    lib = _lib.load()
    nbits = 1 << args.log2n
    rng = np.random.default_rng(815)
    calls, info, model = [], {}, {}

    for shape in ((12, 24, 81), (4, 24, 64), (4, 8, 27)):
        code = ap.Ldpc(ctx, ldpc.staircase(*shape), shape[2])
        F = nbits // code.k
        soft = [DeviceSoft(ctx, F * code.n, rng.integers(-128, 128, F * code.n).astype(np.int8)) for _ in range(NSETS)]
        outb = [DeviceBits(ctx, F * code.n) for _ in range(NSETS)]
        name = f"decode {shape} {ITERS} iterations"
        calls.append((name, (lambda c, s, o: lambda i: c.decode(s[i % NSETS], ITERS, early=False, records=False, out=o[i % NSETS]))(code, soft, outb)))
        info[name] = F * code.k
        model[name] = 1024 * 2.4e9 * 64 / (2.0 * VALU_PER_EDGE * code.edges * code.z) / ITERS * code.k
        if shape == (12, 24, 81):
            m = modulation.qpsk(ctx)
            noisy = []
            for k in range(NSETS):
                x = m.modulate(code.encode(DeviceBits(ctx, F * code.k, rng.integers(0, 2, F * code.k, dtype=np.uint8))))
                noise.new(ctx, EXAMPLE_POWER, 815 + k).apply(x)
                noisy.append(m.demod_soft(x, EXAMPLE_SCALE))
            name = f"decode {shape} early stop"
            calls.append((name, (lambda c, s, o: lambda i: c.decode(s[i % NSETS], 20, early=True, records=False, out=o[i % NSETS]))(code, noisy, outb)))
            info[name] = F * code.k
            bits = [DeviceBits(ctx, F * code.k, rng.integers(0, 2, F * code.k, dtype=np.uint8)) for _ in range(NSETS)]
            name = f"encode {shape}"
            calls.append((name, (lambda c, b, o: lambda i: c.encode(b[i % NSETS], out=o[i % NSETS]))(code, bits, outb)))
            info[name] = F * code.k
            half = F * (code.k + code.n) // 2
            calls.append(("copy (encode's bytes)", (lambda s, o, h: lambda i: _lib.check(lib.aeth_copy_dev(ctx.h, C.c_void_p(o[i % NSETS].ptr),
                                                                                                           C.c_void_p(s[i % NSETS].ptr), h)))(soft, outb, half)))
            info["copy (encode's bytes)"] = F * code.k
            _, rec = code.decode(noisy[0], 20, early=True)
            rec = rec.to_host()
            print(f"early stop at power {EXAMPLE_POWER}: {F} codewords, mean {rec['iterations'].mean():.2f} iterations "
                  f"(max {rec['iterations'].max()}), {int((rec['unsatisfied'] != 0).sum())} with unsatisfied checks")

    cc = ap.ConvCode(ctx, 7, (0o171, 0o133), 512, 64, 64)
    cc_soft = [DeviceSoft(ctx, 2 * nbits, rng.integers(-128, 128, 2 * nbits).astype(np.int8)) for _ in range(NSETS)]
    cc_out = [DeviceBits(ctx, nbits) for _ in range(NSETS)]
    calls.append(("cc decode K=7 (512, 64, 64)", lambda i: cc.decode(cc_soft[i % NSETS], None, cc_out[i % NSETS])))
    info["cc decode K=7 (512, 64, 64)"] = nbits

    print(f"about 2^{args.log2n} information bits per call, {NSETS} buffer sets in rotation, {reps} repetitions after {WARMUP} warm-ups")
    t = measure(ctx, calls, reps)
    med = {}
    for name, _ in calls:
        ms = t[name]
        med[name] = statistics.median(ms)
        mod = f"; issue-rate model {model[name] / 1e9:6.1f} Gbit/s" if name in model else ""
        print(f"  {name:36s} {med[name] * 1e3:9.1f} us  (min {min(ms) * 1e3:8.1f}  max {max(ms) * 1e3:8.1f})  "
              f"{info[name] / med[name] / 1e6:7.2f} Gbit/s of information{mod}", flush=True)
    enc = "encode (12, 24, 81)"
    print(f"  -> {enc}: {med[enc] / med['copy (encode' + chr(39) + 's bytes)']:.2f} x copy of the same bytes")
    del calls
    ctx.close()


if __name__ == "__main__":
    main()
