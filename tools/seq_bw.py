#!/usr/bin/env python3
"""Speed of the device LFSR sequence calls, each beside a yardstick that moves the same bytes in the same process.

Device events around every call, 5 warm-up rounds, REPS (>= 50) timed rounds; the paths alternate inside a round, and
every path rotates over buffers that together exceed 1 GiB (no call finds its operand in the 256 MiB cache).  Per
path: median and min-max in us, bytes per position as the call moves them, TB/s at the median; then the ratio
yardstick time / path time (1.00: as fast as the yardstick).  2^28 positions, the order-7 m-sequence; the Gold rows use
the LTE pair of registers.

    path                           B/position     yardstick
    chips                          8              aeth_vec_zero
    spread sf = 1, sf = 127        16, 8 + 8/127  aeth_vec_clone (sf = 127: aeth_vec_zero, the bytes it moves)
    spread sf = 1 in place         16             aeth_vec_conj
    bits                           1              aeth_vec_zero over the same byte count
    scramble                       2              aeth_copy_dev

Nothing here is a condition; the numbers are reported as they come (profiles/seq_bw.txt).

`--only NAME[,NAME]` runs just those paths (for a kernel trace of its own)."""
import argparse
import ctypes as C
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aether_primitives_amd as ap                                       # noqa: E402
from aether_primitives_amd._lib import check                              # noqa: E402
from aether_primitives_amd.modulation import DeviceBits                   # noqa: E402

WARMUP = 5


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


def report(name, ms, bpp, n):
    med, lo, hi = statistics.median(ms), min(ms), max(ms)
    print(f"  {name:28s} {med * 1e3:9.1f} us  (min {lo * 1e3:8.1f}  max {hi * 1e3:8.1f})  {bpp:6.2f} B/position"
          f"  {bpp * n / med / 1e9:6.2f} TB/s", flush=True)
    return med


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--reps", type=int, default=50)
    ap_.add_argument("--only", default="")
    ap_.add_argument("--log2n", type=int, default=28)
    args = ap_.parse_args()
    only = set(filter(None, args.only.split(",")))
    reps = max(args.reps, 50) if not only else args.reps
    ctx = ap.Context(0)
    lib = ctx._lib
    n = 1 << args.log2n
    m7, gold = ap.Sequence(ctx, (6, 7)), ap.Sequence(ctx, (28, 31), (28, 29, 30, 31))
    I7, IG = 0x7f, (1, 0x12345)
    nv = max(3, (1 << 30) // (8 * n) + 2)                            # cf32 buffers in rotation: more than 1 GiB
    nb = max(6, 2 * ((1 << 30) // n + 1))                            # byte buffers likewise (scramble uses two halves)
    V = [ctx.empty(n) for _ in range(nv)]
    B = [DeviceBits(ctx, n) for _ in range(nb)]
    S127 = [ctx.empty(n // 127) for _ in range(2)]
    n127 = (n // 127) * 127
    for v in V + S127:
        m7.chips(I7, v.n, out=v)                                     # symbols that are numbers
    for b in B:
        m7.bits(I7, n, out=b)
    half = nb // 2

    def vec_zero_bytes(i):                                           # aeth_vec_zero over n bytes
        check(lib.aeth_vec_zero(ctx.h, C.c_void_p(B[i % nb].ptr), n // 8))

    def copy_dev(i):
        check(lib.aeth_copy_dev(ctx.h, C.c_void_p(B[(i + half) % nb].ptr), C.c_void_p(B[i % nb].ptr), n))

    # (name, fn, bytes per position, yardstick)
    rows = [
        ("chips", lambda i: m7.chips(I7, n, out=V[i % nv]), 8.0, "vec_zero"),
        ("chips gold", lambda i: gold.chips(IG, n, skip=1600, out=V[i % nv]), 8.0, "vec_zero"),
        ("vec_zero", lambda i: V[i % nv].vec_zero(), 8.0, None),
        ("spread sf=1", lambda i: m7.spread(I7, V[i % nv], 1, out=V[(i + 1) % nv]), 16.0, "vec_clone"),
        ("vec_clone", lambda i: V[(i + 1) % nv].vec_clone(V[i % nv]), 16.0, None),
        ("spread sf=127", lambda i: m7.spread(I7, S127[i % 2], 127, out=V[i % nv].slice(0, n127)), 8.0 + 8.0 / 127, "vec_zero"),
        ("spread sf=1 in place", lambda i: m7.spread(I7, V[i % nv], 1, out=V[i % nv]), 16.0, "vec_conj"),
        ("vec_conj", lambda i: V[i % nv].vec_conj(), 16.0, None),
        ("bits", lambda i: m7.bits(I7, n, out=B[i % nb]), 1.0, "vec_zero (bytes)"),
        ("bits gold", lambda i: gold.bits(IG, n, skip=1600, out=B[i % nb]), 1.0, "vec_zero (bytes)"),
        ("vec_zero (bytes)", vec_zero_bytes, 1.0, None),
        ("scramble", lambda i: m7.scramble(I7, B[i % nb], out=B[(i + half) % nb]), 2.0, "copy_dev"),
        ("copy_dev", copy_dev, 2.0, None),
    ]
    rows = [r for r in rows if not only or r[0] in only]
    print(f"n = 2^{args.log2n} positions, {nv} cf32 and {nb} byte buffers in rotation, {reps} repetitions after {WARMUP} warm-ups; "
          f"chunk {m7.chunk} positions per wave")
    t = measure(ctx, [(r[0], r[1]) for r in rows], reps)
    med = {r[0]: report(r[0], t[r[0]], r[2], n) for r in rows}
    for name, _, _, yard in rows:
        if yard and yard in med:
            print(f"  -> {name}: {med[yard] / med[name]:.2f} of {yard} ({med[name] * 1e3:.1f} us against {med[yard] * 1e3:.1f} us)")
    del V, B, S127
    ctx.close()


if __name__ == "__main__":
    main()
