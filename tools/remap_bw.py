#!/usr/bin/env python3
"""Speed of the rate-matching kernels (csrc/aeth_remap.hip) beside a device copy that moves the same bytes.

Device events around every call, 5 warm-up rounds, REPS (>= 20) timed rounds; the calls alternate inside a round and rotate
over four sets of buffers.  Every shape writes 2^28 output bytes (rounded down to whole periods) and reads n_in =
aeth_remap_in_count of them.  Its yardstick is aeth_copy_dev of (n_in + n_out) / 2 bytes between the same buffers: that
copy reads and writes n_in + n_out bytes in all, the traffic of the remap call.  Per call: median and min-max in us, TB/s
over n_in + n_out; per shape the ratio of the medians.

    identity 192                 map[i] = i
    bicm16(192, 4)               the 802.11a interleaver of a 16-QAM symbol
    puncture 3/4                 6 -> 4, keep [1, 1, 1, 0, 0, 1]
    depuncture 3/4               4 -> 6, its inverse
    puncture + bicm16            the composed 288 -> 192 map of examples/wifi.py
    its inverse                  192 -> 288
    rows_cols(32, 193)           a 6176-byte block interleaver
    rows_cols(255, 257)          65535 bytes: the gather route

Nothing here is a condition; the numbers are reported as they come (profiles/remap_bw.txt)."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import aether_primitives_amd as ap                                       # noqa: E402
from aether_primitives_amd import _lib, remap                            # noqa: E402

WARMUP = 5
NSETS = 4
KEEP = (1, 1, 1, 0, 0, 1)


def shapes(ctx):
    punct = ap.Remap.puncture(ctx, KEEP)
    both = punct.then(ap.Remap.bicm16(ctx, 192, 4))
    return [("identity 192", ap.Remap(ctx, np.arange(192, dtype=np.int32), 192)),
            ("bicm16(192, 4)", ap.Remap.bicm16(ctx, 192, 4)),
            ("puncture 3/4", punct),
            ("depuncture 3/4", punct.inverse()),
            ("puncture + bicm16 (288 -> 192)", both),
            ("its inverse (192 -> 288)", both.inverse()),
            ("rows_cols(32, 193)", ap.Remap.rows_cols(ctx, 32, 193)),
            ("rows_cols(255, 257)", ap.Remap.rows_cols(ctx, 255, 257))]


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--reps", type=int, default=20)
    ap_.add_argument("--log2n", type=int, default=28)
    ap_.add_argument("--out", default=os.path.join(ROOT, "profiles", "remap_bw.txt"))
    args = ap_.parse_args()
    reps = max(args.reps, 20)
    ctx = ap.Context(0)
    lib = _lib.load()
    todo = []
    for name, rm in shapes(ctx):
        n_out = ((1 << args.log2n) // rm.r_out) * rm.r_out
        todo.append((name, rm, rm.in_count(n_out), n_out))
    cap = max(max(n_in, n_out) for _, _, n_in, n_out in todo)
    host = np.random.default_rng(815).integers(0, 256, cap, dtype=np.uint8)
    bufs = []
    for _ in range(NSETS):
        a, b = ctx.alloc(cap), ctx.alloc(cap)
        ctx.upload(a, host); ctx.upload(b, host)
        bufs.append((a, b))
    lines = [f"2^{args.log2n} output bytes per call (whole periods), {NSETS} buffer sets in rotation, {reps} repetitions after {WARMUP} "
             f"warm-ups; the copy moves (n_in + n_out) / 2 bytes: n_in + n_out read and written"]
    print(lines[0], flush=True)
    e0, e1 = ctx.event(), ctx.event()
    for name, rm, n_in, n_out in todo:
        half = (n_in + n_out) // 2
        calls = (("remap", lambda i: _lib.check(lib.aeth_remap_exec(rm.h, C.c_void_p(bufs[i % NSETS][0]), n_in, C.c_void_p(bufs[i % NSETS][1]), n_out, 0))),
                 ("copy", lambda i: _lib.check(lib.aeth_copy_dev(ctx.h, C.c_void_p(bufs[i % NSETS][1]), C.c_void_p(bufs[i % NSETS][0]), half))))
        t = {k: [] for k, _ in calls}
        for r in range(WARMUP + reps):
            for k, fn in calls:
                e0.record()
                fn(r)
                e1.record()
                e1.sync()
                if r >= WARMUP:
                    t[k].append(e0.elapsed_ms(e1))
        med = {k: statistics.median(v) for k, v in t.items()}
        route = "tile, g = %d" % rm.tile if rm.route == remap.ROUTE_TILE else "gather"
        row = (f"  {name:32s} ({route:14s}) {med['remap'] * 1e3:8.1f} us  (min {min(t['remap']) * 1e3:7.1f}  max {max(t['remap']) * 1e3:7.1f})  "
               f"{(n_in + n_out) / 2 ** 20:6.1f} MiB  {(n_in + n_out) / med['remap'] / 1e9:5.2f} TB/s;  copy {med['copy'] * 1e3:7.1f} us  "
               f"(min {min(t['copy']) * 1e3:7.1f}  max {max(t['copy']) * 1e3:7.1f})  {(n_in + n_out) / med['copy'] / 1e9:5.2f} TB/s;  "
               f"{med['remap'] / med['copy']:.2f} x the copy")
        print(row, flush=True)
        lines.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    for a, b in bufs:
        ctx.free(a); ctx.free(b)
    for _, rm, _, _ in todo:                                             # the objects go before their context
        rm.close()
    ctx.close()


if __name__ == "__main__":
    main()
