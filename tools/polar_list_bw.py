#!/usr/bin/env python3
"""Speed of the polar list decoder and of the pick (csrc/aeth_polar.hip, polar_list_kernel and polar_pick_kernel).

Device events around every call, 5 warm-up rounds, REPS (>= 20) timed rounds; the paths alternate inside a round and
rotate over four sets of buffers.  Every decode handles about 2^24 information bits (whole codewords) of a rate-1/2 code
`polar.mask(n, N / 2)`, n = 5 .. 10.  Per path: median and min-max in us.

    path                                       reported as                                  beside
    list decode (n, L), best row, no record    Gbit/s of information, and the quotient to   aeth_polar_decode of the same
    the same with ALL and records              the SC time                                  codewords, same run
    pick of L rows of K bytes                  us, and the quotient to the copy             aeth_copy_dev of its F L K bytes

T is what aeth_polar_list_create chooses (the largest T <= 16 with T L <= 64 and 2 T <= N); it is printed per shape.
Nothing here is a condition; the numbers are reported as they come (profiles/polar_list_bw.txt)."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import aether_primitives_amd as ap                                       # noqa: E402
from aether_primitives_amd import _lib, crc, polar                       # noqa: E402
from aether_primitives_amd.modulation import DeviceBits, DeviceSoft      # noqa: E402

WARMUP = 5
NSETS = 4
LISTS = (1, 2, 4, 8)


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
    ap_.add_argument("--shapes", type=int, nargs="*", default=[10, 9, 8, 7, 6, 5])
    args = ap_.parse_args()
    reps = max(args.reps, 20)
    ctx = ap.Context(0)
    lib = _lib.load()
    nbits = 1 << args.log2n
    rng = np.random.default_rng(815)
    keep = []
    print(f"about 2^{args.log2n} information bits per call, {NSETS} buffer sets in rotation, {reps} repetitions after {WARMUP} warm-ups")

    for n in args.shapes:
        N, K = 1 << n, 1 << (n - 1)
        F = nbits // K
        msk = polar.mask(n, K)
        host = rng.integers(-128, 128, F * N).astype(np.int8)
        soft = [DeviceSoft(ctx, F * N, host) for _ in range(NSETS)]
        outk = [DeviceBits(ctx, F * K) for _ in range(NSETS)]
        outall = [DeviceBits(ctx, F * 8 * K) for _ in range(2)]
        recs = polar.DeviceListRecords(ctx, F)
        diff = crc.DeviceU64(ctx, F * 8, (rng.integers(0, 3, F * 8) == 0).astype(np.uint64))     # a third of the rows pass
        which = polar.DeviceWhich(ctx, F)
        sc = ap.Polar(ctx, n, msk)
        keep.append(sc)
        calls, lanes = [], {}
        calls.append(("sc", (lambda c: lambda i: _lib.check(lib.aeth_polar_decode(
            c.h, C.c_void_p(soft[i % NSETS].ptr), F * N, None, 0, C.c_void_p(outk[i % NSETS].ptr), F * K, None)))(sc)))
        for L in LISTS:
            code = ap.PolarList(ctx, n, msk, L)
            keep.append(code)
            lanes[L] = (code.lanes, code.group, code.lds_bytes)
            calls.append((f"list L={L}", (lambda c: lambda i: _lib.check(lib.aeth_polar_list_decode(
                c.h, C.c_void_p(soft[i % NSETS].ptr), F * N, 0, C.c_void_p(outk[i % NSETS].ptr), F * K, None)))(code)))
            calls.append((f"list L={L} ALL +records", (lambda c, L: lambda i: _lib.check(lib.aeth_polar_list_decode(
                c.h, C.c_void_p(soft[i % NSETS].ptr), F * N, polar.ALL, C.c_void_p(outall[i % 2].ptr), F * L * K, recs._p())))(code, L)))
            calls.append((f"pick L={L}", (lambda L: lambda i: _lib.check(lib.aeth_polar_list_pick(
                ctx.h, C.c_void_p(outall[0].ptr), K, F, L, diff._p(), C.c_void_p(outk[i % NSETS].ptr), which._p())))(L)))
            calls.append((f"copy of pick L={L}'s rows", (lambda L: lambda i: _lib.check(lib.aeth_copy_dev(
                ctx.h, C.c_void_p(outall[1].ptr), C.c_void_p(outall[0].ptr), F * L * K // 2)))(L)))
        t = measure(ctx, calls, reps)
        med = {name: statistics.median(ms) for name, ms in t.items()}
        print(f"({n}, {K}): {F} codewords; aeth_polar_decode with T = {sc.lanes}: {med['sc'] * 1e3:9.1f} us "
              f"(min {min(t['sc']) * 1e3:8.1f} max {max(t['sc']) * 1e3:8.1f}) {F * K / med['sc'] / 1e6:7.2f} Gbit/s of information", flush=True)
        for L in LISTS:
            T, G, lds = lanes[L]
            for name in (f"list L={L}", f"list L={L} ALL +records"):
                ms = t[name]
                print(f"  {name:26s} T={T:2d} G={G:2d} LDS {lds:6d}: {med[name] * 1e3:9.1f} us  (min {min(ms) * 1e3:8.1f}  max {max(ms) * 1e3:8.1f})  "
                      f"{F * K / med[name] / 1e6:7.2f} Gbit/s of information  {med[name] / med['sc']:6.2f} x SC", flush=True)
            p, c = f"pick L={L}", f"copy of pick L={L}'s rows"
            print(f"  {p:26s} {med[p] * 1e3:9.1f} us  (min {min(t[p]) * 1e3:8.1f}  max {max(t[p]) * 1e3:8.1f});  aeth_copy_dev of its {F * L * K} bytes "
                  f"(half read, half written) {med[c] * 1e3:9.1f} us:  {med[p] / med[c]:5.2f} x", flush=True)
        del calls
        for c in keep:
            c.close()
        keep = []
        del soft, outk, outall, recs, diff, which
    ctx.close()


if __name__ == "__main__":
    main()
