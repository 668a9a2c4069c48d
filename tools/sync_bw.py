#!/usr/bin/env python3
"""Speed of the synchronisation estimators (csrc/aeth_sync.hip) beside aeth_vec_stats, which reads the same bytes and
also reduces them through f64 sums, and beside aeth_vec_clone of half the samples (the same bytes moved), in one process.

Device events around every call, 5 warm-up rounds, REPS (>= 50) timed rounds; the paths alternate inside a round, and
every path rotates over buffers that together exceed 1 GiB (no call finds its operand in the 256 MiB cache).  Every path
reads 2^25 samples, 8 B each.  Per path: median and min-max in us, TB/s at the median, and the ratio to aeth_vec_stats.

    line <kind>            every kind, with the oscillator at -1/4 cycle per sample, at block 0 (one record: the total,
                           the call waits like aeth_vec_stats) and at block 4096 (8192 records left on the device, the
                           call does not wait; the events still time the kernels)
    line <kind> plain      words NULL: no phasor is evaluated
    lag <power>            lag 1 with history, the same two block sizes

Nothing here is a condition; the numbers are reported as they come and written to --out (profiles/sync_bw.txt).

`--only NAME[,NAME]` runs just those paths (for a kernel trace of its own)."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import aether_primitives_amd as ap                                       # noqa: E402
from aether_primitives_amd import nco, sync                              # noqa: E402

WARMUP = 5
KIND_NAMES = {sync.SQUARE: "square", sync.POW1: "pow1", sync.POW2: "pow2", sync.POW4: "pow4", sync.POW8: "pow8"}
BLOCK = 4096


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
    ap_.add_argument("--reps", type=int, default=50)
    ap_.add_argument("--only", default="")
    ap_.add_argument("--log2n", type=int, default=25)
    ap_.add_argument("--out", default=os.path.join(ROOT, "profiles", "sync_bw.txt"))
    args = ap_.parse_args()
    only = set(filter(None, args.only.split(",")))
    reps = max(args.reps, 50) if not only else args.reps
    ctx = ap.Context(0)
    n = 1 << args.log2n
    nv = max(3, (1 << 30) // (8 * n) + 2)                            # cf32 buffers in rotation: more than 1 GiB
    rng = np.random.default_rng(815)
    V = [ctx.vec((rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64))]
    for _ in range(nv - 1):
        V.append(ctx.empty(n).vec_clone(V[0]))
    words = (0, nco.word(-0.25), 0)
    rec = sync.DeviceRecords(ctx, sync.n_blocks(n, BLOCK))
    hist = ctx.vec(np.ones(1, np.complex64))

    rows = [("vec_stats", lambda i: V[i % nv].stats(), 8.0 * n),
            ("vec_clone n/2", lambda i: V[(i + 1) % nv].slice(0, n // 2).vec_clone(V[i % nv].slice(0, n // 2)), 8.0 * n)]
    for kind, name in KIND_NAMES.items():
        for w, tag in ((words, ""), (None, " plain")):
            rows.append((f"line {name}{tag} block 0", lambda i, k=kind, w=w: sync.line_into(ctx, V[i % nv], k, None, w, 1 << 40, 0, total=True), 8.0 * n))
            rows.append((f"line {name}{tag} block {BLOCK}", lambda i, k=kind, w=w: sync.line_into(ctx, V[i % nv], k, rec, w, 1 << 40, BLOCK), 8.0 * n))
    for power in (1, 2, 4, 8):
        rows.append((f"lag pow{power} block 0", lambda i, p=power: sync.lag_into(ctx, V[i % nv], p, 1, None, hist, 0, total=True), 8.0 * n))
        rows.append((f"lag pow{power} block {BLOCK}", lambda i, p=power: sync.lag_into(ctx, V[i % nv], p, 1, rec, hist, BLOCK), 8.0 * n))
    rows = [r for r in rows if not only or r[0] in only]
    lines = [f"2^{args.log2n} samples per call, {nv} cf32 buffers in rotation, {reps} repetitions after {WARMUP} warm-ups, "
             f"chunk {sync.chunk()} samples"]
    print(lines[0], flush=True)
    t = measure(ctx, [(r[0], r[1]) for r in rows], reps)
    med = {name: statistics.median(t[name]) for name, _, _ in rows}
    for name, _, nbytes in rows:
        ms = t[name]
        ratio = f"  {med[name] / med['vec_stats']:5.2f} x vec_stats" if "vec_stats" in med else ""
        lines.append(f"  {name:28s} {med[name] * 1e3:9.1f} us  (min {min(ms) * 1e3:8.1f}  max {max(ms) * 1e3:8.1f})  "
                     f"{nbytes / med[name] / 1e9:6.2f} TB/s{ratio}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    del V, rec, hist, rows
    ctx.close()


if __name__ == "__main__":
    main()
