#!/usr/bin/env python3
"""Speed of the synthesis bank's overlap-add (csrc/aeth_synth.hip) and of `exec` built on it, each beside a yardstick in
the same process.

Device events around every call, 5 warm-up rounds, REPS (>= 50) timed rounds; the paths alternate inside a round, and
every path rotates over buffers that together exceed 1 GiB (no call finds its operand in the 256 MiB cache).  Every
shape makes 2^25 output samples per call out of F = 2^25 / D frames.  Per path: median and min-max in us, and TB/s at the
median over the bytes the path moves algorithmically.

    path                      bytes per frame                               yardstick
    unfold (M, P, D)          8 M read + 8 D written                        aeth_vec_clone of F * M samples (the larger of
                                                                            input and output), aeth_chan_fold of the same
                                                                            shape and frame count (8 D read + 8 M written)
    exec                      aeth_fft_exec (16 M) + unfold                 aeth_fft_exec on the same F frames

The ring kernel re-reads K - 1 halo frames per tile of T frames; the general kernel leaves the P-fold re-read of a frame
to L2.  Nothing here is a condition; the numbers are reported as they come (profiles/synth_bw.txt).

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
SHAPES = ((1024, 8, 1024), (1024, 1, 512), (1024, 1, 256), (1024, 8, 256), (1024, 1, 384))


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
    n = 1 << args.log2n                                              # output samples per call
    big = max(-(-n // D) * M for M, _, D in SHAPES)                  # samples of the largest input
    nv = max(3, (1 << 30) // (8 * big) + 2)                          # cf32 buffers in rotation: more than 1 GiB
    rng = np.random.default_rng(815)
    seed = ctx.vec((rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64))
    V = []
    for _ in range(nv):
        v = ctx.empty(big)
        for o in range(0, big, n):
            v.slice(o, min(o + n, big)).vec_clone(seed.slice(0, min(n, big - o)))
        V.append(v)
    rows, keep, shapes = [], [], []
    for M, P, D in SHAPES:
        proto = chan.prototype("sinc_hamming" if P > 1 else "hann", M, P)
        sy = ap.Synthesizer(ctx, proto, M, D, "stream")
        ch = ap.Channelizer(ctx, proto, M, D, "stream")
        f = ap.HipFft(ctx, M)
        keep += [sy, ch, f]
        F = n // D
        n_in, n_out = F * M, F * D
        tag = f"({M},{P},{D})"
        shapes.append((tag, M))
        io = 8.0 * (n_in + n_out)

        def src(i, k=n_in):
            return V[i % nv].slice(0, k)

        def dst(i, k=n_out):
            return V[(i + 1) % nv].slice(0, k)

        rows += [
            (f"vec_clone {tag}", lambda i, src=src, k=n_in: V[(i + 1) % nv].slice(0, k).vec_clone(src(i)), 16.0 * n_in, None),
            (f"unfold {tag}", lambda i, sy=sy, src=src, dst=dst: sy.unfold(src(i), out=dst(i)), io, f"vec_clone {tag}"),
            (f"chan_fold {tag}", lambda i, ch=ch, src=src, k=n_out, kk=n_in: ch.fold(V[i % nv].slice(0, k), out=V[(i + 1) % nv].slice(0, kk)),
             io, f"vec_clone {tag}"),
            (f"fft_exec {tag}", lambda i, f=f, src=src, k=n_in: f.exec(src(i), V[(i + 1) % nv].slice(0, k), ap.SIGN_REF_BWD, ap.Scale.N),
             16.0 * n_in, None),
            (f"exec {tag}", lambda i, sy=sy, src=src, dst=dst: sy.exec(src(i), s=ap.Scale.N, out=dst(i)), 16.0 * n_in + io, f"fft_exec {tag}"),
        ]
        print(f"{tag}: K = {sy.history + 1}, tile {sy.tile} frames, {F} frames per call, route {sy.route}")
    rows = [r for r in rows if not only or r[0] in only]
    print(f"2^{args.log2n} output samples per call, {nv} cf32 buffers of {big} samples in rotation, {reps} repetitions after {WARMUP} warm-ups")
    t = measure(ctx, [(r[0], r[1]) for r in rows], reps)
    med = {r[0]: report(r[0], t[r[0]], r[2]) for r in rows}
    for name, _, _, yard in rows:
        if yard and yard in med:
            print(f"  -> {name}: {med[name] / med[yard]:.2f} x {yard} ({med[name] * 1e3:.1f} us against {med[yard] * 1e3:.1f} us)")
    for tag, M in shapes:
        if all(k in med for k in (f"unfold {tag}", f"chan_fold {tag}", f"exec {tag}", f"fft_exec {tag}")):
            print(f"  -> {tag}: unfold / chan_fold = {med[f'unfold {tag}'] / med[f'chan_fold {tag}']:.2f}, exec - fft_exec = "
                  f"{(med[f'exec {tag}'] - med[f'fft_exec {tag}']) * 1e3:.1f} us, unfold alone {med[f'unfold {tag}'] * 1e3:.1f} us")
    del V, keep, rows
    ctx.close()


if __name__ == "__main__":
    main()
