#!/usr/bin/env python3
"""Speed of the filter bank's fold (csrc/aeth_chan.hip) and of the calls built on it, each beside a yardstick in the same
process.

Device events around every call, 5 warm-up rounds, REPS (>= 50) timed rounds; the paths alternate inside a round, and
every path rotates over buffers that together exceed 1 GiB (no call finds its operand in the 256 MiB cache).  Every
shape makes 2^25 output samples per call.  Per path: median and min-max in us, and TB/s at the median over the bytes the
path moves algorithmically.

    path                      bytes per output sample                       yardstick
    fold (M, P, D)            16: the fold's algorithmic traffic at D = M   aeth_vec_clone of the output's sample count
                              (8 D / M read + 8 written in general)
    exec                      fold + aeth_fft_exec: 16 + 16                 aeth_fft_exec on the same frame count
    levels                    fold + aeth_fft_exec_levels: 16 + 12          aeth_fft_exec_levels on the same frame count

The ring kernel re-reads P - 1 halo rows per tile of T frames: fold's fair share over the clone is 1 + (P - 1) / (2 T).
Nothing here is a condition; the numbers are reported as they come (profiles/chan_bw.txt).

`--only NAME[,NAME]` runs just those paths (for a kernel trace of its own)."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aether_primitives_amd as ap                                       # noqa: E402
from aether_primitives_amd import chan                                    # noqa: E402

WARMUP = 5
SHAPES = ((1024, 8, 1024), (2048, 16, 2048), (1024, 1, 512), (1024, 8, 256))


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
    print(f"  {name:30s} {med * 1e3:9.1f} us  (min {lo * 1e3:8.1f}  max {hi * 1e3:8.1f})  {bps:6.2f} B/sample"
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
    n = 1 << args.log2n                                              # output samples per call
    nv = max(3, (1 << 30) // (8 * n) + 2)                            # cf32 buffers in rotation: more than 1 GiB
    rng = np.random.default_rng(815)
    first = ctx.vec((rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64))
    V = [first] + [ctx.empty(n).vec_clone(first) for _ in range(nv - 1)]
    LV = [ap.DeviceF32(ctx, n) for _ in range(3)]
    rows = [("vec_clone", lambda i: V[(i + 1) % nv].vec_clone(V[i % nv]), 16.0, None)]
    keep = []
    for M, P, D in SHAPES:
        ch = ap.Channelizer(ctx, chan.prototype("sinc_hamming" if P > 1 else "hann", M, P), M, D, "stream")
        f = ap.HipFft(ctx, M)
        keep += [ch, f]
        frames = n // M
        n_in = frames * D
        tag = f"({M},{P},{D})"
        fold_bytes = 8.0 * D / M + 8.0

        def src(i, n_in=n_in):
            return V[i % nv].slice(0, n_in)

        rows += [
            (f"fold {tag}", lambda i, ch=ch, src=src: ch.fold(src(i), out=V[(i + 1) % nv]), fold_bytes, "vec_clone"),
            (f"exec {tag}", lambda i, ch=ch, src=src: ch.exec(src(i), s=ap.Scale.SN, out=V[(i + 1) % nv]), fold_bytes + 16.0, f"fft_exec {M}"),
            (f"levels {tag}", lambda i, ch=ch, src=src: ch.levels(src(i), s=ap.Scale.SN, kind=ap.LEVEL_POWER_DB, out=LV[i % 3]),
             fold_bytes + 12.0, f"fft_levels {M}"),
        ]
        if not any(r[0] == f"fft_exec {M}" for r in rows):
            rows += [
                (f"fft_exec {M}", lambda i, f=f: f.exec(V[i % nv], V[(i + 1) % nv], ap.SIGN_REF_FWD, ap.Scale.SN), 16.0, None),
                (f"fft_levels {M}", lambda i, f=f: f.levels(V[i % nv], ap.Scale.SN, kind=ap.LEVEL_POWER_DB, out=LV[i % 3]), 12.0, None),
            ]
        print(f"{tag}: tile {ch.tile} frames, {frames} frames per call, route {ch.route}")
    rows = [r for r in rows if not only or r[0] in only]
    print(f"n = 2^{args.log2n} output samples per call, {nv} cf32 buffers in rotation, {reps} repetitions after {WARMUP} warm-ups")
    t = measure(ctx, [(r[0], r[1]) for r in rows], reps)
    med = {r[0]: report(r[0], t[r[0]], r[2], n) for r in rows}
    for name, _, _, yard in rows:
        if yard and yard in med:
            print(f"  -> {name}: {med[name] / med[yard]:.2f} x {yard} ({med[name] * 1e3:.1f} us against {med[yard] * 1e3:.1f} us)")
    for M, P, D in SHAPES:
        tag = f"({M},{P},{D})"
        if all(k in med for k in (f"fold {tag}", f"exec {tag}", f"fft_exec {M}", f"levels {tag}", f"fft_levels {M}")):
            print(f"  -> {tag}: exec - fft_exec = {(med[f'exec {tag}'] - med[f'fft_exec {M}']) * 1e3:.1f} us, levels - fft_levels = "
                  f"{(med[f'levels {tag}'] - med[f'fft_levels {M}']) * 1e3:.1f} us, fold alone {med[f'fold {tag}'] * 1e3:.1f} us")
    del V, LV, keep, rows
    ctx.close()


if __name__ == "__main__":
    main()
