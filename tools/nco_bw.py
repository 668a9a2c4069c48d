#!/usr/bin/env python3
"""Speed of the oscillator (csrc/aeth_nco.hip) beside the copies that move the same bytes, in the same process.

Device events around every call, 5 warm-up rounds, REPS (>= 50) timed rounds; the paths alternate inside a round, and
every path rotates over buffers that together exceed 1 GiB (no call finds its operand in the 256 MiB cache).  Every path
handles 2^25 samples.  Per path: median and min-max in us, and TB/s at the median over the bytes the path moves
algorithmically.

    path                      bytes per sample                              yardstick
    mix, mix chirp            8 read + 8 written                            aeth_vec_clone of the same samples
    mix in place              8 read + 8 written (one buffer)               aeth_vec_clone
    tone, tone chirp          8 written                                     aeth_vec_zero of the same samples
    vec_mul by a table        16 read + 8 written                           what a caller does today: the phasors are made
                                                                            on the host and uploaded (not timed), then
                                                                            aeth_vec_mul; set beside mix

Nothing here is a condition; the numbers are reported as they come (profiles/nco_bw.txt).

`--only NAME[,NAME]` runs just those paths (for a kernel trace of its own)."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aether_primitives_amd as ap                                       # noqa: E402

WARMUP = 5
FREQ, RATE = -0.2, 1e-9                                                  # cycles per sample, and per sample per sample


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


def report(name, ms, nbytes):
    med, lo, hi = statistics.median(ms), min(ms), max(ms)
    print(f"  {name:30s} {med * 1e3:9.1f} us  (min {lo * 1e3:8.1f}  max {hi * 1e3:8.1f})  {nbytes / 2 ** 20:8.1f} MiB"
          f"  {nbytes / med / 1e9:6.2f} TB/s", flush=True)
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
    n = 1 << args.log2n
    nv = max(3, (1 << 30) // (8 * n) + 2)                            # cf32 buffers in rotation: more than 1 GiB
    rng = np.random.default_rng(815)
    V = [ctx.vec((rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64))]
    for _ in range(nv - 1):
        V.append(ctx.empty(n).vec_clone(V[0]))
    shift, chirp = ap.Nco(ctx, freq=FREQ), ap.Nco(ctx, freq=FREQ, rate=RATE)
    table = shift.tone(n)                                            # stands for the table a caller uploads today
    shift.seek(0)

    def at(o, pos=1 << 40):                                          # every call at the same stream position
        return o.seek(pos)

    rows = [
        ("vec_clone", lambda i: V[(i + 1) % nv].vec_clone(V[i % nv]), 16.0 * n, None),
        ("vec_zero", lambda i: V[i % nv].vec_zero(), 8.0 * n, None),
        ("mix", lambda i: at(shift).mix(V[i % nv], V[(i + 1) % nv]), 16.0 * n, "vec_clone"),
        ("mix in place", lambda i: at(shift).mix(V[i % nv], V[i % nv]), 16.0 * n, "vec_clone"),
        ("mix chirp", lambda i: at(chirp).mix(V[i % nv], V[(i + 1) % nv]), 16.0 * n, "vec_clone"),
        ("tone", lambda i: at(shift).tone(n, 1.0, V[i % nv]), 8.0 * n, "vec_zero"),
        ("tone chirp", lambda i: at(chirp).tone(n, 1.0, V[i % nv]), 8.0 * n, "vec_zero"),
        ("vec_mul by a table", lambda i: V[i % nv].vec_mul(table), 24.0 * n, "mix"),
    ]
    rows = [r for r in rows if not only or r[0] in only]
    print(f"2^{args.log2n} samples per call, {nv} cf32 buffers in rotation, {reps} repetitions after {WARMUP} warm-ups")
    t = measure(ctx, [(r[0], r[1]) for r in rows], reps)
    med = {r[0]: report(r[0], t[r[0]], r[2]) for r in rows}
    for name, _, _, yard in rows:
        if yard and yard in med:
            print(f"  -> {name}: {med[name] / med[yard]:.2f} x {yard} ({med[name] * 1e3:.1f} us against {med[yard] * 1e3:.1f} us)")
    del V, table, rows
    ctx.close()


if __name__ == "__main__":
    main()
