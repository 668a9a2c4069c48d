#!/usr/bin/env python3
"""Speed of the convolutional-code kernels (csrc/aeth_cc.hip) and of the soft demodulator (csrc/aeth_modulation.hip).

Device events around every call, 5 warm-up rounds, REPS (>= 20) timed rounds; the paths alternate inside a round and
rotate over four sets of buffers.  Every path handles 2^24 information bits.  Per path: median and min-max in us.

    path                      reported as                                   yardstick
    decode K, (D, A, T)       Gbit/s of information at the median           the issue-rate model below
    encode                    TB/s over nbits read + n nbits written        aeth_vec_clone of the same bytes
    demod_soft (QPSK)         TB/s over 8 B read + 2 B written per symbol   aeth_vec_clone of the same bytes

The decoder is bound by instruction issue, not by memory (n + 1 bytes per information bit).  The model counts the K = 7
forward loop of the shipped code object (llvm-objdump -d of the gfx950 image, cc_decode_kernel<7>, the straight-line group
of six trellis steps up to its backward branch): 65 VALU instructions -- 12 v_dot4c_i32_i8, 10 v_mov_b32_dpp and 4
v_permlane16/32_swap_b32 with the 8 v_mov_b32 that feed them, 6 v_readlane_b32, 6 v_add_u32, 6 v_cmp_gt_i32, 13
v_cndmask_b32 -- beside 7 scalar instructions, 16 s_nop and one branch, and about 5 more VALU instructions when a group's
word is packed and stored: 70 per group, 11.7 per step.  A wave64 VALU instruction occupies its SIMD for 2 cycles, so
with enough waves a SIMD retires a step per 23.3 cycles.  1024 SIMDs at 2.4 GHz then do 105.3 G steps/s, and a window of
A + T + D steps yields D bits: the model is 105.3 * D / (A + T + D) Gbit/s, before the traceback (one dependent LDS read
per group of K - 1 steps, by one lane of each block) and the wait states are counted.  It is printed for K = 7 only: the
shorter codes decode 64 / 2^(K-1) blocks per wave, take their soft values by ds_bpermute_b32 and pay the end of a group
every K - 1 steps, and their loops have not been counted.

Nothing here is a condition; the numbers are reported as they come (profiles/cc_bw.txt)."""
import argparse
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import aether_primitives_amd as ap                                       # noqa: E402
from aether_primitives_amd.modulation import DeviceBits, DeviceSoft      # noqa: E402

WARMUP = 5
NSETS = 4
STEPS_PER_SECOND = 1024 * 2.4e9 / (2.0 * 70.0 / 6.0)                     # the model of the docstring: wave-steps per second


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
    ap_.add_argument("--reps", type=int, default=20)
    ap_.add_argument("--log2n", type=int, default=24)
    args = ap_.parse_args()
    reps = max(args.reps, 20)
    ctx = ap.Context(0)
    nbits = 1 << args.log2n
    rng = np.random.default_rng(815)

    decoders = [("decode K=7 (512, 64, 64)", ap.ConvCode(ctx, 7, (0o171, 0o133), 512, 64, 64)),
                ("decode K=7 (2048, 64, 64)", ap.ConvCode(ctx, 7, (0o171, 0o133), 2048, 64, 64)),
                ("decode K=5 (512, 64, 64)", ap.ConvCode(ctx, 5, (0o23, 0o35), 512, 64, 64)),
                ("decode K=3 (512, 64, 64)", ap.ConvCode(ctx, 3, (0o7, 0o5), 512, 64, 64))]
    enc = decoders[0][1]
    bits = [DeviceBits(ctx, nbits, rng.integers(0, 2, nbits, dtype=np.uint8)) for _ in range(NSETS)]
    coded = [DeviceBits(ctx, 2 * nbits) for _ in range(NSETS)]
    soft = [DeviceSoft(ctx, 2 * nbits, rng.integers(-128, 128, 2 * nbits).astype(np.int8)) for _ in range(NSETS)]
    outb = [DeviceBits(ctx, nbits) for _ in range(NSETS)]
    m = ap.modulation.qpsk(ctx)
    nsym = nbits                                                         # 2^24 QPSK symbols: 2 soft values each
    sym = [ctx.vec((rng.standard_normal(nsym) + 1j * rng.standard_normal(nsym)).astype(np.complex64)) for _ in range(NSETS)]
    n_enc, n_dem = 3 * nbits // 16, 10 * nsym // 16                      # cf32 samples whose clone moves the same bytes
    clone_enc = [(ctx.empty(n_enc), ctx.empty(n_enc)) for _ in range(NSETS)]
    clone_dem = [(ctx.empty(n_dem), ctx.empty(n_dem)) for _ in range(NSETS)]
    for a, b in clone_enc + clone_dem:
        a.vec_zero(); b.vec_zero()

    calls = [(name, (lambda cc: lambda i: cc.decode(soft[i % NSETS], None, outb[i % NSETS]))(cc)) for name, cc in decoders]
    calls += [("encode K=7 n=2", lambda i: enc.encode(bits[i % NSETS], None, coded[i % NSETS])),
              ("vec_clone (encode's bytes)", lambda i: clone_enc[i % NSETS][1].vec_clone(clone_enc[i % NSETS][0])),
              ("demod_soft QPSK", lambda i: m.demod_soft(sym[i % NSETS], 8.0, soft[i % NSETS])),
              ("vec_clone (demod_soft's bytes)", lambda i: clone_dem[i % NSETS][1].vec_clone(clone_dem[i % NSETS][0]))]
    print(f"2^{args.log2n} information bits per call, {NSETS} buffer sets in rotation, {reps} repetitions after {WARMUP} warm-ups")
    t = measure(ctx, calls, reps)
    med = {}
    for name, cc in decoders:
        ms = t[name]
        med[name] = statistics.median(ms)
        D, A, T = cc.block, cc.warmup, cc.traceback
        model = f"; issue-rate model {STEPS_PER_SECOND * D / (A + T + D) / 1e9:6.1f} Gbit/s" if cc.k == 7 else ""
        print(f"  {name:32s} {med[name] * 1e3:9.1f} us  (min {min(ms) * 1e3:8.1f}  max {max(ms) * 1e3:8.1f})  "
              f"{nbits / med[name] / 1e6:7.2f} Gbit/s of information{model}", flush=True)
    for name, nbytes in (("encode K=7 n=2", 3.0 * nbits), ("vec_clone (encode's bytes)", 16.0 * n_enc), ("demod_soft QPSK", 10.0 * nsym),
                         ("vec_clone (demod_soft's bytes)", 16.0 * n_dem)):
        ms = t[name]
        med[name] = statistics.median(ms)
        print(f"  {name:32s} {med[name] * 1e3:9.1f} us  (min {min(ms) * 1e3:8.1f}  max {max(ms) * 1e3:8.1f})  {nbytes / 2 ** 20:8.1f} MiB"
              f"  {nbytes / med[name] / 1e9:6.2f} TB/s", flush=True)
    for name, yard in (("encode K=7 n=2", "vec_clone (encode's bytes)"), ("demod_soft QPSK", "vec_clone (demod_soft's bytes)")):
        print(f"  -> {name}: {med[name] / med[yard]:.2f} x {yard} ({med[name] * 1e3:.1f} us against {med[yard] * 1e3:.1f} us)")
    del calls, bits, coded, soft, outb, sym, clone_enc, clone_dem, decoders, enc
    ctx.close()


if __name__ == "__main__":
    main()
