#!/usr/bin/env python3
"""Speed of the averaged spectra (csrc/aeth_spec.hip), each path beside its yardstick in the same process.

The method of tools/chan_bw.py: device events around every call, 5 warm-up rounds, REPS (>= 50) timed rounds; the paths
alternate inside a round, and every path rotates over input buffers that together exceed 1 GiB (no call finds its operand
in the 256 MiB cache).  Every call takes 2^25 input samples.  Per path: median and min-max in us, and TB/s at the median
over the bytes the path moves algorithmically (per INPUT sample).

    path                      bytes per input sample                         yardstick
    sums fused (M, D)         8 read (overlapping frames come from cache)    levels of the same call; sums general; vec_clone
    sums general, 3 slices    (16 fold + 16 transform + 8 chunk sums) M / D  --
    levels (M, D)             (16 fold + 12 transform with levels) M / D     --
    frame_sums 1024           8 read                                         vec_stats of the same buffer

`sums general` runs with the whole call, 64 MiB and 16 MiB of spectrum per slice (AETH_SPEC_SLICE_KIB; the library reads it
because this tool starts it with AETH_TUNING=1).  Nothing here is a condition; the numbers are reported as they come
(profiles/spec_bw.txt).

`--only NAME[,NAME]` runs just those paths (for a kernel trace of its own)."""
import argparse
import os
import statistics
import sys

os.environ["AETH_TUNING"] = "1"                                          # before the library is loaded
os.environ.pop("AETH_NT", None)

import numpy as np                                                       # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aether_primitives_amd as ap                                       # noqa: E402
from aether_primitives_amd import chan                                    # noqa: E402

WARMUP = 5
SHAPES = ((1024, 1024, "rect"), (1024, 512, "hann"), (2048, 1024, "hann"), (4096, 4096, "rect"))
SLICES = (("whole", 1 << 21), ("64MiB", 64 << 10), ("16MiB", 16 << 10))  # KiB of spectrum per slice


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


def report(name, ms, bps, n):
    med, lo, hi = statistics.median(ms), min(ms), max(ms)
    print(f"  {name:34s} {med * 1e3:9.1f} us  (min {lo * 1e3:8.1f}  max {hi * 1e3:8.1f})  {bps:6.2f} B/sample"
          f"  {bps * n / med / 1e9:6.2f} TB/s", flush=True)
    return med


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--reps", type=int, default=50)
    ap_.add_argument("--only", default="")
    ap_.add_argument("--log2n", type=int, default=25)
    args = ap_.parse_args()
    only = set(filter(None, args.only.split(",")))
    reps = max(args.reps, 50) if not only else args.reps
    ctx = ap.Context(0)
    lib = ctx._lib
    n = 1 << args.log2n                                              # input samples per call
    nv = max(3, (1 << 30) // (8 * n) + 2)                            # cf32 buffers in rotation: more than 1 GiB
    rng = np.random.default_rng(815)
    first = ctx.vec((rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64))
    V = [first] + [ctx.empty(n).vec_clone(first) for _ in range(nv - 1)]
    most = max(n // D * M for M, D, _ in SHAPES)
    LV = [ap.DeviceF32(ctx, most) for _ in range(3)]
    planes = {M: [(ap.DeviceF64(ctx, M), ap.DeviceF64(ctx, M)) for _ in range(3)] for M in {s[0] for s in SHAPES}}

    def sums_call(ch, M, general, kib=None):
        def fn(i):
            if kib is not None:
                os.environ["AETH_SPEC_SLICE_KIB"] = str(kib)
            s, m = planes[M][i % 3]
            ap._lib.check(lib.aeth_chan_exec_sums(ch.h, None, V[i % nv]._p(), n, 0, ap.SIGN_REF_FWD, ap.Scale.SN.kind, 0.0, 0, 0,
                                                  1 if general else 0, s._p(), m._p(), M))
        return fn

    rows = [("vec_clone", lambda i: V[(i + 1) % nv].vec_clone(V[i % nv]), 16.0, ())]
    keep = []
    for M, D, window in SHAPES:
        ch = ap.Channelizer(ctx, chan.prototype(window, M, 1), M, D)
        keep.append(ch)
        tag = f"({M},{D})"
        r = M / D
        rows.append((f"sums fused {tag}", sums_call(ch, M, False), 8.0, (f"levels {tag}", f"sums general 64MiB {tag}", "vec_clone")))
        for name, kib in SLICES:
            rows.append((f"sums general {name} {tag}", sums_call(ch, M, True, kib), 40.0 * r, ()))
        rows.append((f"levels {tag}", lambda i, ch=ch, M=M, D=D: ch.levels(V[i % nv], s=ap.Scale.SN, kind=ap.LEVEL_POWER_DB,
                                                                           out=LV[i % 3].slice(0, n // D * M)), 28.0 * r, ()))
        print(f"{tag} {window}: {n // D} frames per call, chunks of {ch.sums_chunk} frames, fused {ch.sums_fused}, route {ch.route}")
    fs_planes = [(ap.DeviceF64(ctx, 1024), ap.DeviceF64(ctx, 1024)) for _ in range(3)]

    def fs(i):
        s, m = fs_planes[i % 3]
        ap._lib.check(lib.aeth_vec_frame_sums(ctx.h, V[i % nv]._p(), n, 1024, 0, 32, s._p(), m._p(), 1024))

    rows += [("frame_sums 1024", fs, 8.0, ("vec_stats",)), ("vec_stats", lambda i: V[i % nv].stats(), 8.0, ())]
    rows = [r for r in rows if not only or r[0] in only]
    print(f"n = 2^{args.log2n} input samples per call, {nv} cf32 buffers in rotation, {reps} repetitions after {WARMUP} warm-ups")
    t = measure(ctx, [(r[0], r[1]) for r in rows], reps)
    med = {r[0]: report(r[0], t[r[0]], r[2], n) for r in rows}
    for name, _, _, yards in rows:
        for yard in yards:
            if yard in med:
                print(f"  -> {name}: {med[name] / med[yard]:.2f} x {yard} ({med[name] * 1e3:.1f} us against {med[yard] * 1e3:.1f} us)")
    del V, LV, keep, rows, planes, fs_planes
    ctx.close()


if __name__ == "__main__":
    main()
