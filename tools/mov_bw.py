#!/usr/bin/env python3
"""Speed of the moving-window detectors (csrc/aeth_mov.hip) beside aeth_vec_clone of the bytes each call moves and beside
aeth_sync_lag at block 4096 on the same buffer, in one process.

Device events around every call, 5 warm-up rounds, REPS (>= 50) timed rounds; the paths alternate inside a round, and
every path rotates over buffers that together exceed 1 GiB (no call finds its operand in the 256 MiB cache).  Every path
works on 2^25 samples.  Bytes moved (algorithmic): 8 B read per sample, plus 8 B written for the p plane and 4 B for each
of r and m; the search writes one record.  Per path: median and min-max in us, TB/s at the median, and the ratio to the
clone of the same bytes (a clone of k samples moves 16 k bytes).

    search / exec / exec m     the lag kind at (W, L) = (16, 64), (32, 32), (144, 2048), (4096, 1): the search over one block
                               (the call waits for its record), all three planes, the metric alone
    power exec / exec m        the power kind at W = 1024
    sync_lag                   aeth_sync_lag at power 1, the same lag, block 4096 (records left on the device)

Nothing here is a condition; the numbers are reported as they come and written to --out (profiles/mov_bw.txt).

`--only NAME[,NAME]` runs just those paths (for a kernel trace of its own)."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import aether_primitives_amd as ap                                       # noqa: E402
from aether_primitives_amd import mov, sync                              # noqa: E402
from aether_primitives_amd.context import DeviceF32                      # noqa: E402

WARMUP = 5
SHAPES = ((16, 64), (32, 32), (144, 2048), (4096, 1))
POWER_W = 1024
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
    ap_.add_argument("--out", default=os.path.join(ROOT, "profiles", "mov_bw.txt"))
    args = ap_.parse_args()
    only = set(filter(None, args.only.split(",")))
    reps = max(args.reps, 50) if not only else args.reps
    ctx = ap.Context(0)
    n = 1 << args.log2n
    big = n + n // 2                                                 # the largest clone: 24 n bytes = 1.5 n samples
    nv = max(3, (1 << 30) // (8 * big) + 2)                          # cf32 buffers in rotation: more than 1 GiB
    rng = np.random.default_rng(815)
    V = [ctx.vec((rng.standard_normal(big) + 1j * rng.standard_normal(big)).astype(np.complex64))]
    for _ in range(nv - 1):
        V.append(ctx.empty(big).vec_clone(V[0]))
    X = [v.slice(0, n) for v in V]
    dst = ctx.empty(big)
    p, r, m = ctx.empty(n), DeviceF32(ctx, n), DeviceF32(ctx, n)
    rec = sync.DeviceRecords(ctx, sync.n_blocks(n, BLOCK))

    def clone(k):
        return lambda i: dst.slice(0, k).vec_clone(V[i % nv].slice(0, k))

    # (name, call, bytes moved, the clone it is compared with)
    rows = [("clone  8 B/sample", clone(n // 2), 8.0 * n, None), ("clone 12 B/sample", clone(3 * n // 4), 12.0 * n, None),
            ("clone 16 B/sample", clone(n), 16.0 * n, None), ("clone 24 B/sample", clone(big), 24.0 * n, None)]
    for W, L in SHAPES:
        hist = ctx.vec(np.ones(mov.history(mov.LAG, W, L), np.complex64))
        lag_hist = ctx.vec(np.ones(L, np.complex64))
        tag = f"W {W} L {L}"
        rows.append((f"search {tag}", lambda i, W=W, L=L, h=hist: mov.search_into(ctx, X[i % nv], mov.LAG, W, L, 0.0, 0.5, None, h, 0, best=True),
                     8.0 * n, "clone  8 B/sample"))
        rows.append((f"exec {tag}", lambda i, W=W, L=L, h=hist: mov.exec_into(ctx, X[i % nv], mov.LAG, W, L, h, p, r, m), 24.0 * n,
                     "clone 24 B/sample"))
        rows.append((f"exec m {tag}", lambda i, W=W, L=L, h=hist: mov.exec_into(ctx, X[i % nv], mov.LAG, W, L, h, None, None, m), 12.0 * n,
                     "clone 12 B/sample"))
        rows.append((f"sync_lag L {L} block {BLOCK}", lambda i, L=L, h=lag_hist: sync.lag_into(ctx, X[i % nv], 1, L, rec, h, BLOCK), 8.0 * n,
                     "clone  8 B/sample"))
    hist = ctx.vec(np.ones(mov.history(mov.POWER, POWER_W), np.complex64))
    rows.append((f"power exec W {POWER_W}", lambda i, h=hist: mov.exec_into(ctx, X[i % nv], mov.POWER, POWER_W, 0, h, None, r, m), 16.0 * n,
                 "clone 16 B/sample"))
    rows.append((f"power exec m W {POWER_W}", lambda i, h=hist: mov.exec_into(ctx, X[i % nv], mov.POWER, POWER_W, 0, h, None, None, m), 12.0 * n,
                 "clone 12 B/sample"))
    rows.append((f"power search W {POWER_W}", lambda i, h=hist: mov.search_into(ctx, X[i % nv], mov.POWER, POWER_W, 0, 0.0, 0.5, None, h, 0, best=True),
                 8.0 * n, "clone  8 B/sample"))
    rows = [row for row in rows if not only or row[0] in only]
    lines = [f"2^{args.log2n} samples per call, {nv} cf32 buffers in rotation, {reps} repetitions after {WARMUP} warm-ups"]
    print(lines[0], flush=True)
    t = measure(ctx, [(row[0], row[1]) for row in rows], reps)
    med = {row[0]: statistics.median(t[row[0]]) for row in rows}
    for name, _, nbytes, beside in rows:
        ms = t[name]
        ratio = f"  {med[name] / med[beside]:5.2f} x its clone" if beside in med else ""
        lines.append(f"  {name:30s} {med[name] * 1e3:9.1f} us  (min {min(ms) * 1e3:8.1f}  max {max(ms) * 1e3:8.1f})  "
                     f"{nbytes / med[name] / 1e9:6.2f} TB/s{ratio}")
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    del V, X, rec, rows, dst, p, r, m
    ctx.close()


if __name__ == "__main__":
    main()
