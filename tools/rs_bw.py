#!/usr/bin/env python3
"""Speed of the Reed-Solomon kernels (csrc/aeth_rs.hip).

Device events around every call, 5 warm-up rounds, REPS (>= 20) timed rounds; the paths alternate inside a round and
rotate over four sets of buffers.  Every path handles about 2^28 coded bytes (whole frames): a tile of about 2^20 bytes
is made on the host (random data, the host encoder, damage planted at random positions of the chosen codewords) and
doubled on the device to the full length, so the share of damaged codewords is exact.  Per path: median and min-max in
us, GB/s of input plus output at the median, and the ratio to aeth_copy_dev of the same n_in + n_out bytes.

    path                           input
    encode                         random data bytes
    decode clean                   codewords as encoded
    decode 1 % / 10 % / 100 % x 8  that share of the codewords carries 8 symbol errors (every 100th, 10th, each)
    decode 16 errors               every codeword carries 16 errors and no erasure
    decode 32 erasures             every codeword has 32 erased positions (their symbols intact) and no error
                                   (dvb-204-188, r = 16: 8 errors and 16 erasures in the last two rows)

Nothing here is a condition; the numbers are reported as they come (profiles/rs_bw.txt)."""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aether_primitives_amd as ap                                       # noqa: E402
from aether_primitives_amd import _lib, rs                               # noqa: E402
from aether_primitives_amd.modulation import DeviceBits                  # noqa: E402

WARMUP = 5
NSETS = 4
CONFIGS = (("ccsds-255-223", 1), ("ccsds-255-223", 4), ("dvb-204-188", 1))


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


def grown(ctx, lib, tile, copies):
    """a device buffer holding `tile` `copies` times (a power of two): one upload, then doubling copies"""
    buf = DeviceBits(ctx, tile.size * copies, None)
    ctx.upload(buf.ptr, tile)
    have = tile.size
    while have < tile.size * copies:
        _lib.check(lib.aeth_copy_dev(ctx.h, C.c_void_p(buf.ptr + have), C.c_void_p(buf.ptr), have))
        have *= 2
    return buf


def damaged(rng, words, every, errors, erasures):
    """words [W][n] -> (copy with `errors` symbol errors in every `every`-th codeword, erasure flags or None)"""
    words = words.copy()
    era = np.zeros_like(words) if erasures else None
    n = words.shape[1]
    for w in range(0, words.shape[0], every):
        pos = rng.permutation(n)
        words[w, pos[:errors]] ^= rng.integers(1, 256, errors).astype(np.uint8)
        if erasures:
            era[w, pos[errors:errors + erasures]] = 1
    return words, era


def main():
    ap_ = argparse.ArgumentParser()
    ap_.add_argument("--reps", type=int, default=20)
    ap_.add_argument("--log2n", type=int, default=28)
    args = ap_.parse_args()
    reps = max(args.reps, 20)
    ctx = ap.Context(0)
    lib = _lib.load()
    rng = np.random.default_rng(815)
    print(f"about 2^{args.log2n} coded bytes per call, {NSETS} buffer sets in rotation, {reps} repetitions after {WARMUP} warm-ups", flush=True)

    for name, depth in CONFIGS:
        code = ap.Rs(ctx, name)
        n, k, r = code.n, code.k, code.nroots
        tile_frames = max((1 << 20) // (depth * n), 1)
        copies = 1 << max(args.log2n - 20, 0)
        F = tile_frames * copies
        W = tile_frames * depth
        data = rng.integers(0, 256, W * k).astype(np.uint8)
        clean = rs.host_encode(code.code, data, depth)
        words = clean.reshape(tile_frames, n, depth).transpose(0, 2, 1).reshape(W, n)
        fr = lambda a: np.ascontiguousarray(a.reshape(tile_frames, depth, n).transpose(0, 2, 1)).ravel()        # noqa: E731
        heavy = (16, 0) if r >= 32 else (r // 2, 0)
        erased = (0, 32) if r >= 32 else (0, r)
        paths = [("decode clean", clean, None)]
        for label, every in (("decode   1 % x 8 errors", 100), ("decode  10 % x 8 errors", 10), ("decode 100 % x 8 errors", 1)):
            w, _ = damaged(rng, words, every, 8, 0)
            paths.append((label, fr(w), None))
        w, _ = damaged(rng, words, 1, *heavy)
        paths.append((f"decode {heavy[0]} errors + 0 erasures", fr(w), None))
        w, e = damaged(rng, words, 1, *erased)
        paths.append((f"decode 0 errors + {erased[1]} erasures", fr(w), fr(e)))

        outs = [DeviceBits(ctx, F * depth * n) for _ in range(NSETS)]
        calls, nbytes = [], {}
        enc_in = [grown(ctx, lib, data, copies) for _ in range(NSETS)]
        calls.append(("encode", (lambda c, s, o: lambda i: c.encode(s[i % NSETS], depth=depth, out=o[i % NSETS]))(code, enc_in, outs)))
        nbytes["encode"] = F * depth * (k + n)
        held = [enc_in]
        for label, tile, era in paths:
            ins = [grown(ctx, lib, tile, copies) for _ in range(NSETS)]
            eras = [grown(ctx, lib, era, copies) for _ in range(NSETS)] if era is not None else None
            held += [ins, eras]
            calls.append((label, (lambda c, s, e, o: lambda i: c.decode(s[i % NSETS], e[i % NSETS] if e else None, depth=depth, records=False,
                                                                        summary=False, out=o[i % NSETS]))(code, ins, eras, outs)))
            nbytes[label] = F * depth * n * (3 if era is not None else 2)
        for kind, total in (("copy (encode's bytes)", nbytes["encode"]), ("copy (decode's bytes)", 2 * F * depth * n)):
            calls.append((kind, (lambda s, o, h: lambda i: _lib.check(lib.aeth_copy_dev(ctx.h, C.c_void_p(o[i % NSETS].ptr), C.c_void_p(s[i % NSETS].ptr), h)))(
                held[1], outs, total // 2)))
            nbytes[kind] = total

        # what the decoder says about the inputs it is timed on
        for label, tile, era in paths:
            _, rec, summ = rs.host_decode(code.code, tile[:64 * depth * n], None if era is None else era[:64 * depth * n], depth)
            assert not rec["status"].any(), label

        print(f"{name} (n = {n}, k = {k}, r = {r}) at depth {depth}: {F} frames, {F * depth} codewords, {F * depth * n} coded bytes, "
              f"group {code.group}, {code.lds_bytes(depth)} bytes of LDS", flush=True)
        t = measure(ctx, calls, reps)
        med = {label: statistics.median(t[label]) for label, _ in calls}
        for label, _ in calls:
            ms = t[label]
            ref = med["copy (encode's bytes)"] if label == "encode" else med["copy (decode's bytes)"]
            ratio = "" if label.startswith("copy") else f"  {med[label] / ref:7.2f} x copy"
            print(f"  {label:34s} {med[label] * 1e3:10.1f} us  (min {min(ms) * 1e3:9.1f}  max {max(ms) * 1e3:9.1f})  "
                  f"{nbytes[label] / med[label] / 1e6:8.2f} GB/s{ratio}", flush=True)
        del calls, held, outs
        code.close()
    ctx.close()


if __name__ == "__main__":
    main()
