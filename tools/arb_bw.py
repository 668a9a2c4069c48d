#!/usr/bin/env python3
"""Speed of the arbitrary-ratio resampler (csrc/aeth_arb.hip) beside a copy that moves the same bytes and beside the
rational resampler at the nearest rational shape, in the same process.

The protocol of tools/resamp_bw.py: device events around every call, 5 warm-up rounds, REPS (>= 50) timed rounds; the
paths alternate inside a round, and every path rotates over buffers that together exceed 1 GiB (no call finds its operand
in the 256 MiB cache).  Every case (b, P, step) has 2^25 samples on its larger side.  Per path: median and min-max in us,
and TB/s at the median over the bytes the path moves algorithmically.

    path                      bytes                                         yardstick
    arb (b, P, step)          8 n_in read + 8 n_out written                 aeth_vec_clone of (n_in + n_out) / 2 samples
                                                                            aeth_resamp_exec (U, Q, P): U = 2^b, Q = round(U step),
                                                                            but (147, 160) and (160, 147) for those two ratios

Nothing here is a condition; the numbers are reported as they come (profiles/arb_bw.txt).

`--only NAME[,NAME]` runs just those paths (for a kernel trace of its own)."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aether_primitives_amd as ap                                       # noqa: E402
from aether_primitives_amd import resamp                                  # noqa: E402

WARMUP = 5
R441 = 160 / 147 * (1 + 2e-5)
# (b, P, step as a ratio, the rational shape (U, Q) beside it)
CASES = ((6, 16, 1.0000123, (64, 64)), (8, 16, R441, (147, 160)), (8, 16, 1 / R441, (160, 147)), (5, 8, 0.5 + 2.0 ** -20, (32, 16)),
         (6, 16, 4.0001, (64, 256)), (4, 2, 64.3, (16, 1029)), (6, 64, 0.7, (64, 45)))


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
    print(f"  {name:34s} {med * 1e3:9.1f} us  (min {lo * 1e3:8.1f}  max {hi * 1e3:8.1f})  {nbytes / 2 ** 20:8.1f} MiB"
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
    big = 1 << args.log2n                                            # samples on the larger side of every case
    nv = max(3, (1 << 30) // (8 * big) + 2)                          # cf32 buffers in rotation: more than 1 GiB
    rng = np.random.default_rng(815)
    V = [ctx.vec((rng.standard_normal(big) + 1j * rng.standard_normal(big)).astype(np.complex64))]
    for _ in range(nv - 1):
        V.append(ctx.empty(big).vec_clone(V[0]))
    rows, keep = [], []
    for b, P, ratio, (U, Q) in CASES:
        L, step = 1 << b, ap.step_word(ratio)
        ar = ap.ArbResampler(ctx, resamp.prototype(L, -(-L * step >> 32), P), b)
        n_in = big if step >= 1 << 32 else (big * step >> 32)        # the larger side holds 2^25 samples
        n_out, _ = ar.advance(step, 0, n_in)
        assert n_in <= big and n_out <= big, (n_in, n_out)
        tag = f"({b},{P},{ratio:.7g})"
        io = 8.0 * (n_in + n_out)
        half = (n_in + n_out) // 2
        rr = ap.Resampler(ctx, resamp.prototype(U, Q, P), U, Q)
        B = big // max(U, Q)
        keep += [ar, rr]
        rows += [
            (f"vec_clone {tag}", lambda i, k=half: V[(i + 1) % nv].slice(0, k).vec_clone(V[i % nv].slice(0, k)), 16.0 * half, None),
            (f"arb {tag}", lambda i, ar=ar, s=step, a=n_in, c=n_out: ar.exec(V[i % nv].slice(0, a), s, 0, None, V[(i + 1) % nv].slice(0, c)), io,
             f"vec_clone {tag}"),
            (f"resamp ({U},{Q},{P})", lambda i, rr=rr, a=B * Q, c=B * U: rr.exec(V[i % nv].slice(0, a), None, V[(i + 1) % nv].slice(0, c)),
             8.0 * B * (U + Q), None),
        ]
        print(f"{tag}: step {step} / 2^32, route {ar.route(step)}, tile {ar.tile(step)} outputs, {n_in} samples in, {n_out} out; "
              f"resamp ({U},{Q},{P}): route {rr.route}, tile {rr.tile}, {B * Q} in, {B * U} out")
    rows = [r for r in rows if not only or r[0] in only]
    print(f"2^{args.log2n} samples on the larger side, {nv} cf32 buffers of {big} samples in rotation, {reps} repetitions after {WARMUP} warm-ups")
    t = measure(ctx, [(r[0], r[1]) for r in rows], reps)
    med = {r[0]: report(r[0], t[r[0]], r[2]) for r in rows}
    bytes_of = {r[0]: r[2] for r in rows}
    for i, (name, _, _, yard) in enumerate(rows):
        if yard and yard in med:
            line = f"  -> {name}: {med[name] / med[yard]:.2f} x {yard} ({med[name] * 1e3:.1f} us against {med[yard] * 1e3:.1f} us)"
            rat = rows[i + 1][0] if i + 1 < len(rows) and rows[i + 1][0].startswith("resamp ") else None
            if rat in med:                                           # per byte moved: the two calls differ a little in length
                line += f"; {med[name] / bytes_of[name] / (med[rat] / bytes_of[rat]):.2f} x {rat} per byte"
            print(line)
    del V, keep, rows
    ctx.close()


if __name__ == "__main__":
    main()
