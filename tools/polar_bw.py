#!/usr/bin/env python3
"""Speed of the polar kernels (csrc/aeth_polar.hip).

Device events around every call, 5 warm-up rounds, REPS (>= 20) timed rounds; the paths alternate inside a round and
rotate over four sets of buffers.  Every path handles about 2^24 information bits (whole codewords).  Per path: median
and min-max in us.

    path                                 reported as                            yardstick
    decode (n, K) with T lanes           Gbit/s of information at the median    the issue-rate model below
    the same with records, with flips    the same
    encode (n, K)                        Gbit/s of information                  aeth_copy_dev of its K + N bytes per codeword
    aeth_ldpc_decode (12, 24, 81), 10 iterations; aeth_cc_decode K = 7 (512, 64, 64): the same bit count, same run

Every T the library holds is measured for every shape: the knob AETH_POLAR_LANES exists only in the lab build
(`make -C aether_primitives_amd/csrc LAB=1`), which this tool loads; T = 0 is what aeth_polar_create chooses.

The decoder is bound by instruction issue, not by memory (N bytes in, K out per codeword).  The model counts the shipped
code object (llvm-objdump -d of the gfx950 image): a lane-step of an LDS level is 9 VALU and 3 LDS instructions for f,
15 and 4 for g (12 on average); the subtree in registers grows by its own size with T -- 538, 682 and 968 VALU in the
whole kernel for T = 4, 8, 16, so about 35 VALU per leaf with the record's four min / max pairs.  A codeword then costs
N / 64 * (12 (n - log2 T) + 35 T) wave-level VALU instructions, each holding its SIMD for 2 cycles: 1024 SIMDs at 2.4 GHz do
1024 * 2.4e9 / (2 * that) codewords per second, K information bits each -- before the waits for LDS and the cross-lane
moves, the scalar load per schedule word and idle SIMDs where the LDS allows few waves are counted.

Nothing here is a condition; the numbers are reported as they come (profiles/polar_bw.txt)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAB = os.path.exists(os.path.join(ROOT, "aether_primitives_amd", "lib", "libaether_hip_lab.so"))
if LAB:
    os.environ.setdefault("AETH_LAB_LIB", "1")       # AETH_POLAR_LANES exists only in the lab build
    os.environ["AETH_TUNING"] = "1"

import argparse                                                           # noqa: E402
import ctypes as C                                                        # noqa: E402
import statistics                                                         # noqa: E402

import numpy as np                                                        # noqa: E402

sys.path.insert(0, ROOT)
import aether_primitives_amd as ap                                       # noqa: E402
from aether_primitives_amd import _lib, ldpc, polar                      # noqa: E402
from aether_primitives_amd.modulation import DeviceBits, DeviceSoft      # noqa: E402

WARMUP = 5
NSETS = 4
SHAPES = ((10, 512), (9, 256), (8, 128), (7, 64), (6, 32), (5, 16))
VALU_STEP, VALU_LEAF = 12, 35


def model(n, K, T):
    valu = (1 << n) / 64 * (VALU_STEP * (n - T.bit_length() + 1) + VALU_LEAF * T)
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
    calls, info, mod = [], {}, {}
    keep = []

    for n, K in SHAPES:
        N = 1 << n
        F = nbits // K
        msk = polar.mask(n, K)
        host = rng.integers(-128, 128, F * N).astype(np.int8)
        soft = [DeviceSoft(ctx, F * N, host) for _ in range(NSETS)]
        outb = [DeviceBits(ctx, F * N) for _ in range(NSETS)]
        outk = [DeviceBits(ctx, F * K) for _ in range(NSETS)]
        flips = polar.DeviceFlips(ctx, F, rng.integers(0, N, F).astype(np.uint32))
        recs = polar.DeviceRecords(ctx, F)
        chosen = None
        for T in ((0, 4, 8, 16) if LAB else (0,)):
            if T and 2 * T > N:
                continue
            os.environ["AETH_POLAR_LANES"] = str(T)
            code = ap.Polar(ctx, n, msk)
            keep.append(code)
            if T == 0:
                chosen = code.lanes
            tag = f"decode ({n}, {K}) T={code.lanes}" + (" (chosen)" if T == 0 else "")

            variants = (("", None, None),) if T != 0 else (("", None, None), (" +records", None, recs), (" +records +flips", flips, recs))
            for suffix, flip, rec in variants:
                # closures over this shape's buffers: bind them now
                fn = (lambda c, flip, rec, soft=soft, outk=outk, F=F, N=N, K=K: lambda i: _lib.check(lib.aeth_polar_decode(
                    c.h, C.c_void_p(soft[i % NSETS].ptr), F * N, C.c_void_p(flip.ptr) if flip else None, 0, C.c_void_p(outk[i % NSETS].ptr), F * K,
                    C.c_void_p(rec.ptr) if rec else None)))(code, flip, rec)
                calls.append((tag + suffix, fn))
                info[tag + suffix] = F * K
                mod[tag + suffix] = model(n, K, code.lanes)
        os.environ["AETH_POLAR_LANES"] = "0"
        code = keep[-1]
        host = rng.integers(0, 2, F * K, dtype=np.uint8)
        bits = [DeviceBits(ctx, F * K, host) for _ in range(NSETS)]
        name = f"encode ({n}, {K})"
        calls.append((name, (lambda c, b, o: lambda i: c.encode(b[i % NSETS], out=o[i % NSETS]))(code, bits, outb)))
        info[name] = F * K
        half = F * (K + N) // 2
        cname = f"copy (encode ({n}, {K})'s bytes)"
        calls.append((cname, (lambda s, o, h: lambda i: _lib.check(lib.aeth_copy_dev(ctx.h, C.c_void_p(o[i % NSETS].ptr), C.c_void_p(s[i % NSETS].ptr), h)))(soft, outb, half)))
        info[cname] = F * K
        print(f"({n}, {K}): {F} codewords, aeth_polar_create chooses T = {chosen}", flush=True)

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

    print(f"about 2^{args.log2n} information bits per call, {NSETS} buffer sets in rotation, {reps} repetitions after {WARMUP} warm-ups"
          + ("" if LAB else "; no lab build: only the chosen T"))
    t = measure(ctx, calls, reps)
    med = {}
    for name, _ in calls:
        ms = t[name]
        med[name] = statistics.median(ms)
        m = f"; issue-rate model {mod[name] / 1e9:6.1f} Gbit/s" if name in mod else ""
        print(f"  {name:40s} {med[name] * 1e3:9.1f} us  (min {min(ms) * 1e3:8.1f}  max {max(ms) * 1e3:8.1f})  "
              f"{info[name] / med[name] / 1e6:7.2f} Gbit/s of information{m}", flush=True)
    for n, K in SHAPES:
        print(f"  -> encode ({n}, {K}): {med[f'encode ({n}, {K})'] / med[f'copy (encode ({n}, {K})' + chr(39) + 's bytes)']:.2f} x copy of the same bytes")
    del calls
    for c in keep:
        c.close()
    ctx.close()


if __name__ == "__main__":
    main()
