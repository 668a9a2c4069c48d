#!/usr/bin/env python3
"""Speed of the rational resampler (csrc/aeth_resamp.hip) beside a copy that moves the same bytes, in the same process.

Device events around every call, 5 warm-up rounds, REPS (>= 50) timed rounds; the paths alternate inside a round, and
every path rotates over buffers that together exceed 1 GiB (no call finds its operand in the 256 MiB cache).  Every
shape (U, Q, P) has 2^25 samples on its larger side (rounded down to whole periods).  Per path: median and min-max in us,
and TB/s at the median over the bytes the path moves algorithmically.

    path                      bytes                                         yardstick
    resamp (U, Q, P)          8 n_in read + 8 n_out written                 aeth_vec_clone of (n_in + n_out) / 2 samples
    resamp (1, 4, 16)         as above                                      also aeth_fir_exec_decim, the same 16 taps, dec 4

Nothing here is a condition; the numbers are reported as they come (profiles/resamp_bw.txt).

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
SHAPES = ((1, 1, 1), (1, 1, 16), (2, 1, 8), (1, 4, 16), (3, 2, 8), (147, 160, 16), (160, 147, 16), (1, 64, 2), (7, 5, 64))
FIR_SHAPE = (1, 4, 16)


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
    big = 1 << args.log2n                                            # samples on the larger side of every shape
    nv = max(3, (1 << 30) // (8 * big) + 2)                          # cf32 buffers in rotation: more than 1 GiB
    rng = np.random.default_rng(815)
    V = [ctx.vec((rng.standard_normal(big) + 1j * rng.standard_normal(big)).astype(np.complex64))]
    for _ in range(nv - 1):
        V.append(ctx.empty(big).vec_clone(V[0]))
    rows, keep = [], []
    for U, Q, P in SHAPES:
        rs = ap.Resampler(ctx, resamp.prototype(U, Q, P), U, Q)
        keep.append(rs)
        B = big // max(U, Q)
        n_in, n_out = B * Q, B * U
        tag = f"({U},{Q},{P})"
        io = 8.0 * (n_in + n_out)
        half = (n_in + n_out) // 2
        rows += [
            (f"vec_clone {tag}", lambda i, k=half: V[(i + 1) % nv].slice(0, k).vec_clone(V[i % nv].slice(0, k)), 16.0 * half, None),
            (f"resamp {tag}", lambda i, rs=rs, a=n_in, b=n_out: rs.exec(V[i % nv].slice(0, a), None, V[(i + 1) % nv].slice(0, b)), io,
             f"vec_clone {tag}"),
        ]
        if (U, Q, P) == FIR_SHAPE:
            fir = ap.Fir(ctx, resamp.prototype(U, Q, P).astype(np.complex64), 2048)
            keep.append(fir)
            rows.append((f"fir_decim {tag}", lambda i, fir=fir, a=n_in, b=n_out: fir.filter_decim(V[i % nv].slice(0, a), 4, V[(i + 1) % nv].slice(0, b)),
                         io, f"vec_clone {tag}"))
        print(f"{tag}: route {rs.route}, tile {rs.tile} outputs, {n_in} samples in, {n_out} out")
    rows = [r for r in rows if not only or r[0] in only]
    print(f"2^{args.log2n} samples on the larger side, {nv} cf32 buffers of {big} samples in rotation, {reps} repetitions after {WARMUP} warm-ups")
    t = measure(ctx, [(r[0], r[1]) for r in rows], reps)
    med = {r[0]: report(r[0], t[r[0]], r[2]) for r in rows}
    for name, _, _, yard in rows:
        if yard and yard in med:
            print(f"  -> {name}: {med[name] / med[yard]:.2f} x {yard} ({med[name] * 1e3:.1f} us against {med[yard] * 1e3:.1f} us)")
    tag = "({},{},{})".format(*FIR_SHAPE)
    if f"resamp {tag}" in med and f"fir_decim {tag}" in med:
        print(f"  -> resamp {tag} / fir_decim {tag} = {med[f'resamp {tag}'] / med[f'fir_decim {tag}']:.2f}")
    del V, keep, rows
    ctx.close()


if __name__ == "__main__":
    main()
