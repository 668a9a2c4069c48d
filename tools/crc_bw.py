#!/usr/bin/env python3
"""Speed of the frame-check and bit-packing kernels (csrc/aeth_crc.hip) beside a device copy that moves the same bytes.

Device events around every call, 5 warm-up rounds, REPS (>= 20) timed rounds; the calls alternate inside a round and rotate
over four sets of buffers.  Every shape reads about 2^28 input bytes (whole frames).  Its yardstick is aeth_copy_dev of
(n_in + n_out) / 2 bytes between the same buffers: that copy reads and writes n_in + n_out bytes in all, the traffic of the
call.  Per call: median and min-max in us, TB/s over n_in + n_out; per shape the ratio of the medians.

    check  L = 6144,  r = 24     an LTE code block with CRC-24B: diff words, stripped payload and summary
    check  L = 12000, r = 32     a 1500-byte frame with the 802.11 FCS
    check  L = 54,    r = 16     blind-decoding candidates of a control channel
    exec   L = 2^28              one frame: the long route
    attach L = 6144,  r = 24
    pack / unpack                2^28 bits, LSB first

Nothing here is a condition; the numbers are reported as they come (profiles/crc_bw.txt)."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import aether_primitives_amd as ap                                       # noqa: E402
from aether_primitives_amd import _lib                                   # noqa: E402

WARMUP = 5
NSETS = 4


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--reps", type=int, default=20)
    ap_.add_argument("--log2n", type=int, default=28)
    ap_.add_argument("--out", default=os.path.join(ROOT, "profiles", "crc_bw.txt"))
    args = ap_.parse_args()
    reps = max(args.reps, 20)
    n = 1 << args.log2n
    ctx = ap.Context(0)
    lib = _lib.load()
    c16, c24, c32 = (ap.Crc.named(ctx, k) for k in ("crc-16/xmodem", "crc-24/lte-b", "crc-32"))
    cap = n + (n >> 3) + 4096
    host = np.random.default_rng(815).integers(0, 256, cap, dtype=np.uint8)
    bufs = []
    for _ in range(NSETS):
        a, b = ctx.alloc(cap), ctx.alloc(cap)
        ctx.upload(a, host); ctx.upload(b, host)
        bufs.append((a, b))
    p = lambda v: C.c_void_p(v)

    def check(c, L):
        F = n // (L + c.r)
        # the outputs share buffer b: payload, then the diff words, then the summary, 16-byte aligned
        o_diff = (F * L + 15) & ~15
        o_sum = o_diff + 8 * F
        fn = lambda i: lib.aeth_crc_check(c.h, p(bufs[i][0]), L, F, 0, p(bufs[i][1] + o_diff), p(bufs[i][1]), p(bufs[i][1] + o_sum))
        return f"check  L = {L}, r = {c.r}, F = {F}", fn, F * (L + c.r), F * L + 8 * F + 16, c.route(L, F)

    def attach(c, L):
        F = n // (L + c.r)
        fn = lambda i: lib.aeth_crc_attach(c.h, p(bufs[i][0]), L, F, p(bufs[i][1]))
        return f"attach L = {L}, r = {c.r}, F = {F}", fn, F * L, F * (L + c.r), c.route(L, F)

    todo = [check(c24, 6144), check(c32, 12000), check(c16, 54),
            (f"exec   L = 2^{args.log2n}, r = 32, F = 1", lambda i: lib.aeth_crc_exec(c32.h, p(bufs[i][0]), n, 1, None, p(bufs[i][1])), n, 8, c32.route(n, 1)),
            attach(c24, 6144),
            (f"pack   2^{args.log2n} bits", lambda i: lib.aeth_bits_pack(ctx.h, p(bufs[i][0]), n, 0, p(bufs[i][1]), n // 8), n, n // 8, 0),
            (f"unpack 2^{args.log2n} bits", lambda i: lib.aeth_bits_unpack(ctx.h, p(bufs[i][0]), n // 8, 0, p(bufs[i][1]), n), n // 8, n, 0)]
    lines = [f"about 2^{args.log2n} input bytes per call (whole frames), {NSETS} buffer sets in rotation, {reps} repetitions after {WARMUP} "
             f"warm-ups; the copy moves (n_in + n_out) / 2 bytes: n_in + n_out read and written"]
    print(lines[0], flush=True)
    e0, e1 = ctx.event(), ctx.event()
    for name, fn, n_in, n_out, route in todo:
        half = (n_in + n_out) // 2
        calls = (("crc", lambda i: _lib.check(fn(i % NSETS))),
                 ("copy", lambda i: _lib.check(lib.aeth_copy_dev(ctx.h, p(bufs[i % NSETS][1]), p(bufs[i % NSETS][0]), half))))
        t = {k: [] for k, _ in calls}
        for r in range(WARMUP + reps):
            for k, call in calls:
                e0.record()
                call(r)
                e1.record()
                e1.sync()
                if r >= WARMUP:
                    t[k].append(e0.elapsed_ms(e1))
        med = {k: statistics.median(v) for k, v in t.items()}
        tag = {0: "stream", 1: "frames", 2: "long"}[route]
        row = (f"  {name:40s} ({tag:6s}) {med['crc'] * 1e3:8.1f} us  (min {min(t['crc']) * 1e3:7.1f}  max {max(t['crc']) * 1e3:7.1f})  "
               f"{(n_in + n_out) / 2 ** 20:6.1f} MiB  {(n_in + n_out) / med['crc'] / 1e9:5.2f} TB/s;  copy {med['copy'] * 1e3:7.1f} us  "
               f"(min {min(t['copy']) * 1e3:7.1f}  max {max(t['copy']) * 1e3:7.1f})  {(n_in + n_out) / med['copy'] / 1e9:5.2f} TB/s;  "
               f"{med['crc'] / med['copy']:.2f} x the copy")
        print(row, flush=True)
        lines.append(row)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    for a, b in bufs:
        ctx.free(a); ctx.free(b)
    for c in (c16, c24, c32):                                            # the objects go before their context
        c.close()
    ctx.close()


if __name__ == "__main__":
    main()
