#!/usr/bin/env python3
"""Speed of aeth_vec_stats, aeth_vec_levels and aeth_fft_exec_levels against calls that move more bytes per sample.

Device events around every single call, 5 warm-up rounds, REPS (>= 50) timed rounds; the compared calls alternate inside
a round, and every call rotates over enough buffers that the working set exceeds 1 GiB (no call finds its operand in
the 256 MiB cache).  Per call: median and min-max in us, bytes per sample, TB/s at the median.

  group A, 2^25 samples:   vec_conj (16 B/sample, the yardstick), vec_stats (8 B; the time includes its wait and the
                           64-byte download), vec_levels NORM / DB / POWER_DB (12 B)
  group B, N = 2048 x 8192 frames, Scale::SN, mirrored:
                           fft_exec_mirrored (16 B, the yardstick), fft_exec_levels NORM / DB / POWER_DB (12 B), and the
                           three calls the fused one replaces (fft_exec + vec_mirror_frames + vec_levels: 16 + 16 + 12 B)

Condition: vec_stats, vec_levels NORM <= vec_conj and fft_exec_levels NORM <= fft_exec_mirrored, each with the min-max
spread of the yardstick's own repetitions as margin.  The dB kinds are reported without a condition.

`--only NAME[,NAME]` runs just those calls (for a kernel trace of its own: `rocprofv3 --kernel-trace --stats -- python
tools/stats_levels_bw.py --only vec_stats`)."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aether_primitives_amd as ap                                       # noqa: E402
from aether_primitives_amd import Scale                                   # noqa: E402

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


def report(name, ms, bytes_per_sample, samples):
    med, lo, hi = statistics.median(ms), min(ms), max(ms)
    print(f"  {name:34s} {med * 1e3:9.1f} us  (min {lo * 1e3:8.1f}  max {hi * 1e3:8.1f})  {bytes_per_sample:3d} B/sample"
          f"  {bytes_per_sample * samples / med / 1e9:6.2f} TB/s", flush=True)
    return med, lo, hi


def verdict(name, med, yard_name, yard):
    ymed, ylo, yhi = yard
    ok = med <= ymed + (yhi - ylo)
    print(f"  -> {name} {'no slower than' if ok else 'SLOWER than'} {yard_name}: {med * 1e3:.1f} us against {ymed * 1e3:.1f} us"
          f" (margin: {yard_name}'s own spread, {(yhi - ylo) * 1e3:.1f} us)")


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--reps", type=int, default=50)
    ap_.add_argument("--only", default="")
    args = ap_.parse_args()
    only = set(filter(None, args.only.split(",")))
    reps = max(args.reps, 50) if not only else args.reps
    ctx = ap.Context(0)
    rng = np.random.default_rng(815)
    keep = lambda calls: [c for c in calls if not only or c[0] in only]

    # ---- group A: one vector of 2^25 samples (256 MiB), five of them in rotation (1.25 GiB)
    n, nb = 1 << 25, 5
    host = (rng.standard_normal(2 * n, dtype=np.float32) * 0.7).view(np.complex64)
    A = [ctx.vec(host) for _ in range(nb)]
    L = [ap.DeviceF32(ctx, n) for _ in range(nb)]
    calls = keep([("vec_conj", lambda i: A[i % nb].vec_conj()),
                  ("vec_stats", lambda i: A[i % nb].stats()),
                  ("vec_levels NORM", lambda i: A[i % nb].levels(ap.LEVEL_NORM, out=L[i % nb])),
                  ("vec_levels DB", lambda i: A[i % nb].levels(ap.LEVEL_DB, out=L[i % nb])),
                  ("vec_levels POWER_DB", lambda i: A[i % nb].levels(ap.LEVEL_POWER_DB, out=L[i % nb]))])
    if calls:
        print(f"group A: n = 2^25 samples, {nb} buffers in rotation, {reps} repetitions after {WARMUP} warm-ups")
        t = measure(ctx, calls, reps)
        bps = {"vec_conj": 16, "vec_stats": 8}
        res = {name: report(name, t[name], bps.get(name, 12), n) for name, _ in calls}
        if "vec_conj" in res:
            for name in ("vec_stats", "vec_levels NORM"):
                if name in res:
                    verdict(name, res[name][0], "vec_conj", res["vec_conj"])
    del A, L

    # ---- group B: 8192 frames of 2048 (128 MiB), nine of them in rotation (1.125 GiB) plus outputs
    N, batch, nb = 2048, 8192, 9
    m = N * batch
    f = ap.HipFft(ctx, N, max_batch=batch)
    X = [ctx.vec(host[:m]) for _ in range(nb)]
    S = [ctx.empty(m) for _ in range(2)]
    L = [ap.DeviceF32(ctx, m) for _ in range(nb)]

    def three(i):
        s = S[i % 2]
        f.fwd(X[i % nb], s, Scale.SN)
        s.vec_mirror_frames(N)
        s.levels(ap.LEVEL_NORM, out=L[i % nb])

    calls = keep([("fft_exec_mirrored", lambda i: f.rfft_mirror(X[i % nb], Scale.SN)),
                  ("fft_exec_levels NORM", lambda i: f.levels(X[i % nb], Scale.SN, mirror=True, kind=ap.LEVEL_NORM, out=L[i % nb])),
                  ("fft_exec_levels DB", lambda i: f.levels(X[i % nb], Scale.SN, mirror=True, kind=ap.LEVEL_DB, out=L[i % nb])),
                  ("fft_exec_levels POWER_DB", lambda i: f.levels(X[i % nb], Scale.SN, mirror=True, kind=ap.LEVEL_POWER_DB, out=L[i % nb])),
                  ("exec + mirror_frames + levels", three)])
    if calls:
        print(f"group B: N = {N}, batch {batch}, Scale::SN, mirrored, {nb} buffers in rotation, {reps} repetitions after {WARMUP} warm-ups")
        t = measure(ctx, calls, reps)
        bps = {"fft_exec_mirrored": 16, "exec + mirror_frames + levels": 44}
        res = {name: report(name, t[name], bps.get(name, 12), m) for name, _ in calls}
        if "fft_exec_mirrored" in res and "fft_exec_levels NORM" in res:
            verdict("fft_exec_levels NORM", res["fft_exec_levels NORM"][0], "fft_exec_mirrored", res["fft_exec_mirrored"])
    ctx.close()


if __name__ == "__main__":
    main()
