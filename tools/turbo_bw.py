#!/usr/bin/env python3
"""Speed of the turbo kernels (csrc/aeth_turbo.hip).

Device events around every call, 5 warm-up rounds, REPS (>= 20) timed rounds; the paths alternate inside a round and
rotate over four sets of buffers.  Every path handles about 2^24 information bits (whole codewords).  Per path: median
and min-max in us.

    path                                         reported as                            yardstick
    decode (code, K, W, A), 1 and 8 iterations   Gbit/s of information at the median    the issue-rate model below
    the same, 8 iterations with early stop       the same, and the mean iterations run
    encode                                       Gbit/s of information                  aeth_copy_dev of its K + N bytes per codeword
    aeth_ldpc_decode (12, 24, 81), 10 iterations; aeth_cc_decode K = 7 (512, 64, 64): the same bit count, same run

The decoder's input is what examples/turbo.py decodes: random frames, encoded, through QPSK and noise of deviation 1.1 per
component, soft values of +-16 at a noise-free symbol -- all made on the device.  Without early stop the control flow does
not depend on the data.

The decoder is bound by instruction issue and by the round trip of its alpha store, not by the frame's bytes.  The model
counts the shipped code object (llvm-objdump -d of the gfx950 image; basic blocks of the two loops of window_pass): a
forward step of a lane is 36, 60 and 108 VALU instructions for S = 4, 8, 16, a backward step with its output 91, 127 and
222; a warm-up step is counted like a window step.  A codeword then costs, per iteration,
2 * windows * (W + A) * (forward + backward) lane-steps, 64 of which make a wave-level instruction that holds its SIMD for
2 cycles: 1024 SIMDs at 2.4 GHz do 1024 * 2.4e9 / (2 * that / 64) codewords per second, K information bits each -- before
the scalar instructions that make the signs (41 and 58 per step at S = 8), the waits for LDS and for the alpha store, idle
lanes of clipped windows and idle SIMDs where the LDS allows few waves are counted.

Nothing here is a condition; the numbers are reported as they come (profiles/turbo_bw.txt)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import argparse                                                           # noqa: E402
import ctypes as C                                                        # noqa: E402
import statistics                                                         # noqa: E402

import numpy as np                                                        # noqa: E402

sys.path.insert(0, ROOT)
import aether_primitives_amd as ap                                       # noqa: E402
from aether_primitives_amd import _lib, ldpc, modulation, noise, turbo   # noqa: E402
from aether_primitives_amd.modulation import DeviceBits, DeviceSoft      # noqa: E402

WARMUP = 5
NSETS = 4
SHAPES = (("lte", 6144, (263, 480), 32, 32), ("lte", 512, (31, 64), 32, 16), ("lte", 40, (3, 10), 40, 0))
VALU = {4: (36, 91), 8: (60, 127), 16: (108, 222)}
POWER, SOFT_SCALE = 1.1, 4.0


def model(K, W, A, S, iters):
    windows = (K - 1) // W + 1
    valu = 2 * iters * windows * (min(W, K) + A) * sum(VALU[S]) / 64.0
    return 1024 * 2.4e9 / (2.0 * valu) * K


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
    calls, info, mod, notes = [], {}, {}, {}
    keep = []
    m = modulation.qpsk(ctx)

    for cname, K, (f1, f2), W, A in SHAPES:
        F = (nbits // K) & ~1                                            # an even number of coded bits for QPSK at any N
        code = ap.Turbo(ctx, cname, turbo.qpp(K, f1, f2), W, A)
        keep.append(code)
        N = code.n
        bits = [DeviceBits(ctx, F * K, rng.integers(0, 2, F * K, dtype=np.uint8)) for _ in range(NSETS)]
        soft = []
        for s in range(NSETS):
            x = m.modulate(code.encode(bits[s]))
            noise.new(ctx, POWER, 815 + s).apply(x)
            soft.append(m.demod_soft(x, SOFT_SCALE))
        outk = [DeviceBits(ctx, F * K) for _ in range(NSETS)]
        outn = [DeviceBits(ctx, F * N) for _ in range(NSETS)]
        recs = turbo.DeviceRecords(ctx, F)
        tag = f"decode ({cname}, {K}, {W}, {A})"
        for iters, early in ((1, False), (8, False), (8, True)):
            name = f"{tag} {iters} it" + (" early" if early else "")
            fn = (lambda c, it, fl, soft=soft, outk=outk, recs=recs, F=F, N=N, K=K: lambda i: _lib.check(lib.aeth_turbo_decode(
                c.h, C.c_void_p(soft[i % NSETS].ptr), F * N, it, fl, C.c_void_p(outk[i % NSETS].ptr), F * K, C.c_void_p(recs.ptr))))(
                    code, iters, turbo.EARLY if early else 0)
            calls.append((name, fn))
            info[name] = F * K
            if not early:
                mod[name] = model(K, W, A, code.states, iters)
            else:
                fn(0)
                notes[name] = f"; mean iterations {recs.to_host()['iterations'].mean():.2f}"
        name = f"encode ({cname}, {K})"
        calls.append((name, (lambda c, b, o: lambda i: c.encode(b[i % NSETS], out=o[i % NSETS]))(code, bits, outn)))
        info[name] = F * K
        half = F * (K + N) // 2
        cn = f"copy (encode ({cname}, {K})'s bytes)"
        calls.append((cn, (lambda s, o, h: lambda i: _lib.check(lib.aeth_copy_dev(ctx.h, C.c_void_p(o[i % NSETS].ptr), C.c_void_p(s[i % NSETS].ptr), h)))(
            soft, outn, half)))
        info[cn] = F * K
        print(f"({cname}, {K}, {W}, {A}): {F} codewords, {code.windows} windows, {code.group} codewords per workgroup, {code.lds_bytes} bytes of LDS",
              flush=True)

    shape = (12, 24, 81)
    lcode = ap.Ldpc(ctx, ldpc.staircase(*shape), shape[2])
    LF = nbits // lcode.k
    lsoft = [DeviceSoft(ctx, LF * lcode.n, rng.integers(-128, 128, LF * lcode.n).astype(np.int8)) for _ in range(NSETS)]
    lout = [DeviceBits(ctx, LF * lcode.n) for _ in range(NSETS)]
    calls.append((f"ldpc decode {shape} 10 iterations", lambda i: lcode.decode(lsoft[i % NSETS], 10, early=False, records=False, out=lout[i % NSETS])))
    info[f"ldpc decode {shape} 10 iterations"] = LF * lcode.k
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
        rate = info[name] / med[name] / 1e6
        mtxt = f"; issue-rate model {mod[name] / 1e9:6.2f} Gbit/s, reached {100 * rate * 1e9 / mod[name]:.0f} %" if name in mod else ""
        print(f"  {name:40s} {med[name] * 1e3:9.1f} us  (min {min(ms) * 1e3:8.1f}  max {max(ms) * 1e3:8.1f})  "
              f"{rate:7.2f} Gbit/s of information{mtxt}{notes.get(name, '')}", flush=True)
    for cname, K, _, _, _ in SHAPES:
        print(f"  -> encode ({cname}, {K}): {med[f'encode ({cname}, {K})'] / med[f'copy (encode ({cname}, {K})' + chr(39) + 's bytes)']:.2f} x copy of the same bytes")
    del calls
    for c in keep:
        c.close()
    ctx.close()


if __name__ == "__main__":
    main()
