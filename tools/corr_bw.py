#!/usr/bin/env python3
"""Speed of the two fused correlator calls against the unfused paths they replace.

Device events around every compared path (a path of two calls is timed as one region), 5 warm-up rounds, REPS (>= 50)
timed rounds; the paths alternate inside a round, and every path rotates over enough input buffers that the working set
exceeds 1 GiB (no call finds its operand in the 256 MiB cache).  Per path: median and min-max in us, bytes per sample as
the calls move them, TB/s at the median.  fft_len 2048, a 64-sample template, 2^24 and 2^25 samples.

    corr_exec_levels KIND       12 B/sample     against   fir_exec + vec_levels KIND     8 + 8 + 8 + 4 = 28 B/sample
    corr_search                  8 B/sample     against   fir_exec + vec_stats           8 + 8 + 8     = 24 B/sample
    (both searches include their wait and the download of the record, as vec_stats does)
    fir_exec alone              16 B/sample     the yardstick in the same process

Nothing here is a condition; the numbers are reported as they come (profiles/corr_bw.txt).

`--only NAME[,NAME]` runs just those paths (for a kernel trace of its own)."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aether_primitives_amd as ap                                       # noqa: E402
from aether_primitives_amd._lib import check                              # noqa: E402

WARMUP = 5
KINDS = (("NORM", ap.LEVEL_NORM), ("DB", ap.LEVEL_DB), ("POWER_DB", ap.LEVEL_POWER_DB))


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
    return med


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--reps", type=int, default=50)
    ap_.add_argument("--only", default="")
    ap_.add_argument("--log2n", default="24,25")
    args = ap_.parse_args()
    only = set(filter(None, args.only.split(",")))
    reps = max(args.reps, 50) if not only else args.reps
    ctx = ap.Context(0)
    rng = np.random.default_rng(815)
    ref = (rng.standard_normal(128, dtype=np.float32) * 0.7).view(np.complex64)
    corr = ap.Corr(ctx, ref, 2048)
    fir = ap.Fir(ctx, np.conj(ref[::-1]), 2048)
    lib = corr._lib
    for log2n in (int(v) for v in args.log2n.split(",")):
        n = 1 << log2n
        nb = (1 << 30) // (8 * n) + 1                                # inputs in rotation: more than 1 GiB
        host = (rng.standard_normal(2 * n, dtype=np.float32) * 0.7).view(np.complex64)
        X = [ctx.vec(host) for _ in range(nb)]
        S = [ctx.empty(n) for _ in range(2)]                         # the unfused paths' intermediate
        L = [ap.DeviceF32(ctx, n) for _ in range(3)]
        npk = corr.n_blocks(n)
        P = [ctx.alloc(npk * 16) for _ in range(2)]
        best = (C.c_char * 16)()

        def unfused_levels(kind):
            def fn(i):
                s = S[i % 2]
                fir.filter(X[i % nb], out=s)
                s.levels(kind, out=L[i % 3])
            return fn

        def unfused_search(i):
            s = S[i % 2]
            fir.filter(X[i % nb], out=s)
            s.stats()

        def search(peaks):
            def fn(i):
                x = X[i % nb]
                check(lib.aeth_corr_search(corr.h, None, x._p(), x.n, C.c_void_p(P[i % 2]) if peaks else None,
                                           npk if peaks else 0, best))
            return fn

        calls = [("fir_exec", lambda i: fir.filter(X[i % nb], out=S[i % 2]))]
        bps = {"fir_exec": 16, "fir_exec + vec_stats": 24, "corr_search (best)": 8, "corr_search (records + best)": 8}
        for name, kind in KINDS:
            calls.append((f"corr_exec_levels {name}", (lambda k: lambda i: corr.levels(X[i % nb], k, out=L[i % 3]))(kind)))
            calls.append((f"fir_exec + vec_levels {name}", unfused_levels(kind)))
            bps[f"corr_exec_levels {name}"], bps[f"fir_exec + vec_levels {name}"] = 12, 28
        calls += [("corr_search (best)", search(False)), ("corr_search (records + best)", search(True)),
                  ("fir_exec + vec_stats", unfused_search)]
        calls = [c for c in calls if not only or c[0] in only]
        print(f"n = 2^{log2n} samples, fft_len 2048, 64-sample template, {nb} inputs in rotation, {reps} repetitions after "
              f"{WARMUP} warm-ups")
        t = measure(ctx, calls, reps)
        med = {name: report(name, t[name], bps[name], n) for name, _ in calls}
        pairs = [(f"corr_exec_levels {k}", f"fir_exec + vec_levels {k}") for k, _ in KINDS]
        pairs += [("corr_search (best)", "fir_exec + vec_stats"), ("corr_search (records + best)", "fir_exec + vec_stats")]
        for fused, unfused in pairs:
            if fused in med and unfused in med:
                word = "faster than" if med[fused] < med[unfused] else "NOT faster than"
                print(f"  -> {fused} {word} {unfused}: {med[fused] * 1e3:.1f} us against {med[unfused] * 1e3:.1f} us"
                      f" (x {med[unfused] / med[fused]:.2f})" + (f"; fir_exec alone {med['fir_exec'] * 1e3:.1f} us" if "fir_exec" in med else ""))
        for p in P:
            ctx.free(p)
        del X, S, L
    ctx.close()


if __name__ == "__main__":
    main()
