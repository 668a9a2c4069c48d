#!/usr/bin/env python3
"""Speed of the OFDM calls (csrc/aeth_ofdm.hip): the fused route beside the general route of the same object, beside
aeth_fft_exec on the same number of contiguous N-point frames, and beside aeth_vec_clone of the bytes the fused call moves
algorithmically, 8 (N + K) per symbol -- all existing or general-route code, in one process.

Device events around every call, 5 warm-up rounds, REPS (>= 50) timed rounds; the paths alternate inside a round.  Inputs
rotate over six buffers of 2^25 samples (1.5 GiB: no call finds its operand in the 256 MiB cache), outputs over two more.
Shapes (N, G, K): (64, 16, 52), (2048, 144, 1200), (4096, 288, 3276), as many symbols as 2^25 input samples hold.  Per
path: median and min-max in us, TB/s of the bytes the FUSED call moves at the median (so the column compares paths, it is
not each path's own traffic), and the ratio to the fused demod with eq.

Nothing here is a condition; the numbers are reported as they come and written to --out (profiles/ofdm_bw.txt)."""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import aether_primitives_amd as ap                                       # noqa: E402
from aether_primitives_amd import Ofdm, Scale                            # noqa: E402

WARMUP = 5
SHAPES = ((64, 16, 52), (2048, 144, 1200), (4096, 288, 3276))
NIN, NOUT = 6, 2


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


def occupied(n, k):
    """k carriers around DC, DC itself left out: -k/2 .. -1, 1 .. k/2"""
    return np.array(list(range(n - k // 2, n)) + list(range(1, k - k // 2 + 1)))


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--reps", type=int, default=50)
    ap_.add_argument("--log2n", type=int, default=25)
    ap_.add_argument("--out", default=os.path.join(ROOT, "profiles", "ofdm_bw.txt"))
    args = ap_.parse_args()
    reps = max(args.reps, 50)
    ctx = ap.Context(0)
    n = 1 << args.log2n
    rng = np.random.default_rng(815)
    V = [ctx.vec((rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64))]
    for _ in range(NIN - 1):
        V.append(ctx.empty(n).vec_clone(V[0]))
    O = [ctx.empty(n) for _ in range(NOUT)]
    lines = [f"2^{args.log2n} input samples per call, {NIN} input and {NOUT} output buffers in rotation, {reps} repetitions after "
             f"{WARMUP} warm-ups; TB/s of 8 (N + K) bytes per symbol"]
    print(lines[0], flush=True)
    for N, G, K in SHAPES:
        L = N + G
        n_sym = n // L
        bins = occupied(N, K)
        fused, general = Ofdm(ctx, N, G, bins), Ofdm(ctx, N, G, bins, max_symbols=n_sym, general=True)
        plan = ap.HipFft(ctx, N)
        eq = ctx.vec((rng.standard_normal(K) + 1j * rng.standard_normal(K)).astype(np.complex64))
        span, n_car, n_time, half = fused.span(n_sym), n_sym * K, n_sym * L, n_sym * (N + K) // 2
        moved = 8.0 * (N + K) * n_sym

        def demod(o, e):
            return lambda i: o.demod(V[i % NIN].slice(0, span), n_sym, eq=e, scale=Scale.SN, out=O[i % NOUT].slice(0, n_car))

        def mod(o):
            return lambda i: o.mod(V[i % NIN].slice(0, n_car), n_sym, scale=Scale.SN, out=O[i % NOUT].slice(0, n_time))

        rows = [("fused demod + eq", demod(fused, eq)), ("fused demod", demod(fused, None)), ("fused mod", mod(fused)),
                ("general demod + eq", demod(general, eq)), ("general mod", mod(general)),
                ("fft_exec, same frames", lambda i: plan.fwd(V[i % NIN].slice(0, n_sym * N), O[i % NOUT].slice(0, n_sym * N), Scale.SN)),
                ("vec_clone, same bytes", lambda i: O[i % NOUT].slice(0, half).vec_clone(V[i % NIN].slice(0, half)))]
        lines.append(f"N = {N}, G = {G}, K = {K}: {n_sym} symbols, fused route \"{fused.route}\", general route \"{general.route}\"")
        print(lines[-1], flush=True)
        t = measure(ctx, rows, reps)
        med = {name: statistics.median(t[name]) for name, _ in rows}
        for name, _ in rows:
            ms = t[name]
            lines.append(f"  {name:24s} {med[name] * 1e3:9.1f} us  (min {min(ms) * 1e3:8.1f}  max {max(ms) * 1e3:8.1f})  "
                         f"{moved / med[name] / 1e9:6.2f} TB/s  {med[name] / med['fused demod + eq']:5.2f} x fused demod + eq")
            print(lines[-1], flush=True)
        fused.close(); general.close()
        del plan, eq, rows
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    del V, O
    ctx.close()


if __name__ == "__main__":
    main()
