"""GPU: every kernel whose grid is capped at a few workgroups per CU, called with more than twice the cap's worth of work,
so that every workgroup goes at least twice round its `for (g = blockIdx.x; g < n; g += gridDim.x)` loop and a third of
them three times.  State that lives from one trip to the next (an LDS table kept, an image parity, counters and flags
rewritten per group, a staging area reused) is live only then.  Everything is compared byte for byte.

The capped grids under aether_primitives_amd/csrc/ (caps in workgroups; 256 CUs on an MI355X):

  kernel                    cap (file:line)                                  carried between trips                    past the cap in
  ------------------------  -----------------------------------------------  ---------------------------------------  ------------------------------------
  fft_pow2_kernel           min(groups, 8 CUs)  aeth_fft.hip:232-233         LDS staging area shared with the single  test_fft_pow2_staged_batch_equals_short_calls
    (loop aeth_fft.hip:87)                                                   exchange image, `par`
  fft_pow2_stream_kernel    min(batch, CUs 512/WG)  aeth_fft.hip:237-238     the prefetched frame `nx`, `par`, two    tests/test_gpu_large.py::test_fft2048_batch_beyond_4gib
    (loop aeth_fft.hip:200)                                                  exchange images                          (262149 frames, cap 1024)
  fft_mixed_kernel          min(groups, 8 CUs)  aeth_fft.hip:633-634         LDS images, the pass twiddles copied to  test_fft_mixed_batch_equals_short_calls
    (loop aeth_fft.hip:532)                                                  LDS once per workgroup
  fft_ragged_kernel         min(groups, CUs LANES/WG)                        LDS staging area, `par`, two images      tests/test_gpu_fft.py::test_ragged_streaming_batch_matches_small_batches
    (aeth_fft_ragged.h:156)   aeth_fft_ragged.hip:23-24                                                               ([3] 3.1 M frames, cap 2048 x 128; [196] 48151, cap 4096 x 4;
                                                                                                                      [2401] 3933, cap 512; [6000] 1575, cap 1024)
  blu_pre, blu_mul,         min(blocks, 8 CUs)  aeth_fft_big.hip:254-259     none                                     test_bluestein_copies_batch_equals_short_calls
    blu_post (aeth_fft_big.hip:222, 237, 246)
  fmi_kernel                min(groups, CUs 8/(WG/64))  aeth_fir.hip:60, 73  the prefetched window, `par`, two images tests/test_gpu_large.py::test_fir_stream_beyond_4gib
    (aeth_fir_kernel.h:535)                                                                                           (270 k blocks of 1985 outputs, cap 1024)
  ofdm_fused_kernel         min(groups, 8 CUs)  aeth_ofdm.hip:316-317        staged lengths: one LDS area for input   test_ofdm_fused (64, 128, 256, 1024);
    (loop aeth_ofdm.hip:113)                                                 staging, exchange image, output staging; tests/test_gpu_ofdm.py::test_more_symbols_than_the_resident_grid
                                                                             `par`                                    (512: 2051 symbols, cap 2048 -- past the cap, not twice)
  ofdm_strip, pick, place,  min(blocks, 32 CUs)  aeth_ofdm.hip:306-310       none                                     test_ofdm_general_route_copies
    prefix (aeth_ofdm.hip:229, 240, 252, 262)
  remap_tile_kernel         min(tiles, 4 CUs)  aeth_remap.hip:301            `have` and the LDS table it stands for,  test_remap_tile_route
    (loop aeth_remap.hip:68)                                                 the staging image
  remap_gather_kernel       min(blocks, 8 CUs)  aeth_remap.hip:314-315       none                                     test_remap_gather_route
    (loop aeth_remap.hip:135)
  turbo_decode_kernel       slots = min(128 MiB / slab, 8 CUs)               LDS frames, a-priori arrays, counts[],   test_turbo_decode
    (loop aeth_turbo.hip:203) aeth_turbo.hip:354-355, 440                    going[], the alpha slab
  bits_pack_kernel,         min(blocks, 16 CUs)  aeth_crc.hip:644-645,       none                                     test_bits_pack_and_unpack
    bits_unpack_kernel (aeth_crc.hip:327, 342)   665-666

No loop: in aeth_noise.hip:35, 47, 82 and aeth_modulation.hip:248, 263 `gridDim.x * kBlock` is the distance between the
kPairs = 2 pairs of one lane; those grids are not capped (pair_grid, grid_for).  Lengths 512 .. 4096 of the fused OFDM
kernel all have an even number of exchanges per transform (fft_next_par<C>(0) == 0: NPASS = 3), so 2048 and 4096 add
no parity class to 512 and 1024; 64, 128 and 256 (NPASS = 2) have an odd one.

remap_tile_kernel, a finding: a workgroup's tiles lie gridDim.x tiles apart, and past the cap gridDim.x = 4 CUs, a multiple
of 16 on every device whose CU count is a multiple of 4.  The phases sh and osh of its tiles are then the same on every
trip whatever the tile lengths are, `have` never changes after the first tile and the table is never rebuilt on a
later trip.  The maps below still have tile lengths that are no multiples of 16 (asserted), so that neighbouring
workgroups build different tables; that the phase moves between one workgroup's trips cannot be arranged from outside
on such a device, and test_remap_tile_route prints which it is.

The functions without the `gpu` mark need no device: the tile geometry of the remap maps from the host formula
(tile_periods of aeth_remap.hip), the early and late stops among the turbo frames, and the restatements' run time."""
import ctypes as C
import math
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import aether_primitives_amd as ap                    # noqa: E402
from aether_primitives_amd import HipFft, Ofdm, Scale, _lib, crc, remap   # noqa: E402
import crc_truth                                      # noqa: E402
import remap_truth                                    # noqa: E402
import turbo_truth as T                               # noqa: E402

gpu = pytest.mark.gpu

CUS_MI355X = 256
FILL = 0x3c


HIP_ATTR_MULTIPROCESSOR_COUNT = 63                    # hipDeviceAttributeMultiprocessorCount (hip_runtime_api.h)


def cus_of(ctx):
    """the CU count the library reads for the context's device (multiProcessorCount), from the HIP runtime the library is
    bound to.  Not through torch: importing it brings a second HIP runtime into the test process (see test_gpu_overlap.py),
    and that one finds no device here."""
    hip, v = _lib.load(), C.c_int(0)
    assert hip.hipDeviceGetAttribute(C.byref(v), HIP_ATTR_MULTIPROCESSOR_COUNT, ctx.device) == 0 and v.value > 0
    return v.value


def looped(what, units, cap):
    """the loop check of every test: more than twice the cap, said aloud"""
    msg = f"{what}: {units} work units against a cap of {cap} workgroups = {units / cap:.3f} trips"
    assert units > 2 * cap, msg
    print(msg)


def bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def signal(n, seed):
    r = np.random.default_rng(seed)
    return ((r.standard_normal(n) + 1j * r.standard_normal(n)) * 0.7).astype(np.complex64)


# ---- a, b: remap -----------------------------------------------------------------------------------------------------
def pad(j):
    return j + ((j >> 7) << 2)


def tile_periods(r_in, r_out):
    """tile_periods of aeth_remap.hip: the periods per tile, 0 for the gather route"""
    def fits(g):
        t_in, t_out = g * r_in, g * r_out
        stage = (pad(t_in + 15) + 1 + 15) & ~15
        return t_in < 65536 and t_out < 65536 and stage + 32 * ((t_out + 30) >> 4) <= 32768
    if not fits(1):
        return 0
    lo, hi = 1, 32768
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    u = math.lcm(16 // math.gcd(r_in, 16), 16 // math.gcd(r_out, 16))
    return lo - lo % u if lo >= u else lo


# (r_out, r_in, t_in % 16 == 0, t_out % 16 == 0, the pointer offsets)
TILE_MAPS = {
    "both_odd": (3001, 2999, False, False, ((0, 0), (5, 11))),        # 3 and 5 would do for the periods alone, but their tile
    #                                                                   is 16 k periods long: both lengths multiples of 16
    "both_16": (192, 288, True, True, ((0, 0),)),
    "out_odd": (3001, 4096, True, False, ((0, 0), (5, 11))),
}


def tile_map(name):
    r_out, r_in = TILE_MAPS[name][:2]
    rng = np.random.default_rng(r_out * 7 + r_in)
    m = rng.integers(0, r_in, r_out).astype(np.int32)
    m[rng.integers(0, 6, r_out) == 0] = -1
    return m


def tile_call(name, cap):
    """-> (n_out, tiles): 2 cap + cap / 3 whole tiles, then a tile of one period and a partial period that ends in fills"""
    r_out, r_in = TILE_MAPS[name][:2]
    g = tile_periods(r_in, r_out)
    m = tile_map(name)
    part = int(np.flatnonzero(m[:r_out - 1] < 0)[-1]) + 1            # the partial period's last output is a fill
    whole = 2 * cap + cap // 3
    n_out = whole * g * r_out + r_out + part
    return n_out, whole + 1


def test_remap_tile_lengths_have_the_phases_the_maps_are_named_for():
    for name, (r_out, r_in, in16, out16, _) in TILE_MAPS.items():
        g = tile_periods(r_in, r_out)
        assert g >= 2, (name, g)                                      # the last tile (one period and a bit) is a partial one
        assert ((g * r_in) % 16 == 0, (g * r_out) % 16 == 0) == (in16, out16), (name, g, g * r_in % 16, g * r_out % 16)
        m = tile_map(name)
        assert (m < 0).any() and (m >= 0).any()
        n_out, tiles = tile_call(name, 4 * CUS_MI355X)
        assert tiles > 2 * 4 * CUS_MI355X and m[(n_out - 1) % r_out] == -1 and n_out % (g * r_out) < g * r_out
        assert n_out + remap_truth.in_count(m, r_in, n_out) < 100 << 20
    g = tile_periods(5, 3)
    assert (g * 5) % 16 == 0 and (g * 3) % 16 == 0, "periods 3 and 5 would serve as the odd map"


def test_remap_restatement_is_quick():
    m = tile_map("both_odd")
    n_out, _ = tile_call("both_odd", 4 * CUS_MI355X)
    x = np.random.default_rng(1).integers(0, 256, remap_truth.in_count(m, 2999, n_out), dtype=np.uint8)
    t = time.perf_counter()
    remap_truth.remap(x, m, 2999, n_out, FILL)
    assert time.perf_counter() - t < 5.0


@gpu
@pytest.mark.parametrize("name", sorted(TILE_MAPS))
def test_remap_tile_route(ctx, name):
    from test_gpu_remap import check
    r_out, r_in, in16, out16, offsets = TILE_MAPS[name]
    rm = ap.Remap(ctx, tile_map(name), r_in)
    g = rm.tile
    assert rm.route == remap.ROUTE_TILE and g == tile_periods(r_in, r_out)
    assert ((g * r_in) % 16 == 0, (g * r_out) % 16 == 0) == (in16, out16), (g, r_in, r_out)
    cap = 4 * cus_of(ctx)
    n_out, tiles = tile_call(name, cap)
    assert tiles == -(-n_out // (g * r_out)) and n_out % (g * r_out) and rm.map[(n_out - 1) % r_out] == -1
    looped(f"remap_tile_kernel {name} (g = {g}, tiles of {g * r_in} -> {g * r_out} bytes)", tiles, cap)
    moves = (cap * g * r_in) % 16 != 0 or (cap * g * r_out) % 16 != 0
    print(f"  phases of one workgroup's tiles {'move' if moves else 'stay'} from trip to trip (stride {cap} tiles); "
          f"neighbouring tiles differ by ({g * r_in % 16}, {g * r_out % 16}) mod 16")
    for in_off, out_off in offsets:
        check(ctx, rm, n_out, 100 + in_off, fill=FILL, in_off=in_off, out_off=out_off)
    rm.close()


@gpu
@pytest.mark.parametrize("out_off", (0, 15))
def test_remap_gather_route(ctx, out_off):
    from test_gpu_remap import check
    m, r_in = remap.rows_cols_map(255, 257)
    rm = ap.Remap(ctx, m, r_in)
    assert rm.route == remap.ROUTE_GATHER and rm.tile == 0
    cap = 8 * cus_of(ctx)
    n_out = 16 * 256 * (2 * cap + cap // 3) + 16 * 77 + 5
    assert n_out > 2 * 8 * cus_of(ctx) * 256 * 16
    looped("remap_gather_kernel (blocks of 256 lanes x 16 bytes)", -(-((n_out + out_off + 15) // 16) // 256), cap)
    check(ctx, rm, n_out, 7 + out_off, fill=FILL, in_off=3, out_off=out_off)
    rm.close()


# ---- c: turbo decode -------------------------------------------------------------------------------------------------
TURBO = dict(name="ccsds", K=1024, f1=31, f2=64, W=64, A=32, G=5, windows=16, S=16, P=11, quiet=7)
TURBO_BUDGET = 128 << 20
TURBO_ITERS = (1, 4)
_TURBO = {}


def turbo_slots(G, windows, S, W, K, cus):
    """(slots, the budget's share of it): aeth_turbo_create, from store_words of aeth_turbo_core.h"""
    slab_bytes = 4 * min(W, K) * S * G * windows
    by_budget = max(1, TURBO_BUDGET // slab_bytes)
    return min(by_budget, 8 * cus), by_budget


def turbo_frames():
    """P distinct frames, the first `quiet` at sigma 1.0 and the others at 2.5 -> (soft [P][N], history of max(TURBO_ITERS)
    iterations of the restatement)"""
    if not _TURBO:
        c = TURBO
        code, pi = T.named(c["name"]), T.qpp(c["K"], c["f1"], c["f2"])
        rng = np.random.default_rng(20261)
        coded = T.encode(code, pi, rng.integers(0, 2, c["P"] * c["K"], dtype=np.uint8)).reshape(c["P"], -1)
        soft = np.stack([T.noisy_soft(rng, coded[f], 1.0 if f < c["quiet"] else 2.5) for f in range(c["P"])])
        history = []
        t = time.perf_counter()
        T.decode(code, pi, c["W"], c["A"], soft.ravel(), max(TURBO_ITERS), 0, None, history)
        _TURBO.update(soft=soft, history=history, pi=pi, secs=time.perf_counter() - t)
    return _TURBO


def turbo_truth(F, max_iter, flags):
    """frame f of the call is frame f % P of turbo_frames() -> (bits [F][K], records [F])"""
    tf = turbo_frames()
    bits, rec = T.from_history(tf["history"], max_iter, flags)
    pick = np.arange(F) % TURBO["P"]
    return bits.reshape(TURBO["P"], -1)[pick], rec[pick]


def test_turbo_frames_stop_early_and_late_on_a_second_trip():
    c = TURBO
    tf = turbo_frames()
    assert tf["secs"] < 20.0, tf["secs"]
    slots, by_budget = turbo_slots(c["G"], c["windows"], c["S"], c["W"], c["K"], CUS_MI355X)
    assert slots == by_budget == 409 and (c["G"] * slots) % c["P"] != 0
    F = c["G"] * 2 * slots + 3
    rec = turbo_truth(F, 4, T.EARLY)[1]
    its = rec["iterations"][:(F // c["G"]) * c["G"]].reshape(-1, c["G"])
    second = its[slots:2 * slots]                                    # the groups of every workgroup's second trip
    early, late = second.max(axis=1) < 4, second.max(axis=1) == 4
    assert early.sum() >= slots // 8 and late.sum() >= slots // 8, (early.sum(), late.sum())
    assert (second.min(axis=1) < second.max(axis=1)).sum() >= slots // 2    # neighbours in a group stop at different iterations
    assert (rec["disagreements"][rec["iterations"] == 4] > 0).any()
    # a workgroup's consecutive trips hold different frames, and so do the frames of one group
    first = (np.arange(3 * slots) * c["G"]) % c["P"]
    assert (first[:slots] != first[slots:2 * slots]).all() and (first[slots:2 * slots] != first[2 * slots:]).all()
    # one iteration leaves disagreements everywhere: the counters of a group end a trip non-zero
    assert (turbo_truth(F, 1, 0)[1]["disagreements"] > 0).all()


@gpu
def test_turbo_decode(ctx):
    from test_gpu_turbo import Mem, d_decode
    c = TURBO
    tf = turbo_frames()
    code = ap.Turbo(ctx, c["name"], tf["pi"], c["W"], c["A"])
    mem = Mem(ctx)
    try:
        assert (code.group, code.windows, code.states) == (c["G"], c["windows"], c["S"])
        slots, by_budget = turbo_slots(code.group, code.windows, code.states, c["W"], c["K"], cus_of(ctx))
        assert slots == by_budget < 8 * cus_of(ctx), "the slot count is to come from the 128 MiB budget"
        F = code.group * (2 * slots) + 3
        assert (code.group * slots) % c["P"] != 0
        looped(f"turbo_decode_kernel (groups of {code.group} codewords, {slots} slots)", -(-F // code.group), slots)
        soft = tf["soft"][np.arange(F) % c["P"]].ravel()
        for max_iter in TURBO_ITERS:
            for flags in (0, T.EARLY):
                want_bits, want_rec = turbo_truth(F, max_iter, flags)
                bits, rec = d_decode(mem, code, soft, max_iter, flags)
                bad = np.flatnonzero(rec != want_rec)
                assert rec.tobytes() == want_rec.tobytes(), (max_iter, flags, bad[:8], rec[bad[:4]], want_rec[bad[:4]])
                assert bits.tobytes() == want_bits.tobytes(), (max_iter, flags, np.flatnonzero((bits != want_bits).any(axis=1))[:8])
                bits, none = d_decode(mem, code, soft, max_iter, flags, records=False)
                assert none is None and bits.tobytes() == want_bits.tobytes(), (max_iter, flags, "no records")
                mem.free()
    finally:
        mem.free()
        code.close()


# ---- d, e: OFDM ------------------------------------------------------------------------------------------------------
OFDM_FUSED = {64: 8, 128: 8, 256: 4, 1024: 1}        # length: symbols per workgroup (CfgFor<N>::F)
_OFDM = {}


def ofdm_case(ctx, n, n_sym, bins_):
    """the inputs of one length and what the chain of existing calls makes of them, computed once"""
    from test_gpu_ofdm import chain_demod, chain_mod
    key = (n, n_sym)
    if key not in _OFDM:
        g, k = n // 4, len(bins_)
        x, eq, car = signal((n_sym - 1) * (n + g) + n, 3 * n), signal(k, 3 * n + 1), signal(n_sym * k, 3 * n + 2)
        _OFDM.clear()                                   # one length's arrays at a time
        _OFDM[key] = (x, eq, car, chain_demod(ctx, x, n, g, bins_, n_sym, eq, Scale.SN), chain_mod(ctx, car, n, g, bins_, n_sym, Scale.SN))
    return _OFDM[key]


def ofdm_both_ways(ctx, o, n, n_sym, bins_, parity):
    from test_gpu_ofdm import Dev, same
    g, k = n // 4, len(bins_)
    x, eq, car, want_d, want_m = ofdm_case(ctx, n, n_sym, bins_)
    xin = Dev(ctx, x.size, parity, x)
    out = Dev(ctx, n_sym * k, parity ^ 1)
    o.demod(xin.v, n_sym, eq=eq, scale=Scale.SN, out=out.v)
    got = out.get()
    assert same(got, want_d), ("demod", n, parity, np.flatnonzero(got.view(np.uint64) != want_d.view(np.uint64))[:8] // k)
    del xin, out
    cin = Dev(ctx, n_sym * k, parity, car)
    out = Dev(ctx, n_sym * (n + g), parity ^ 1)
    o.mod(cin.v, n_sym, scale=Scale.SN, out=out.v)
    got = out.get()
    assert same(got, want_m), ("mod", n, parity, np.flatnonzero(got.view(np.uint64) != want_m.view(np.uint64))[:8] // (n + g))


@gpu
@pytest.mark.parametrize("n,parity", [(n, p) for n, f in OFDM_FUSED.items() for p in ((0, 1) if f > 1 else (0,))])
def test_ofdm_fused(ctx, n, parity):
    from test_gpu_ofdm import carrier_sets
    f = OFDM_FUSED[n]
    cap = 8 * cus_of(ctx)
    n_sym = f * (2 * cap) + f + 1
    bins_ = carrier_sets(n)[1]
    o = Ofdm(ctx, n, n // 4, bins_)
    assert o.route == "fused"
    looped(f"ofdm_fused_kernel N = {n} (groups of {f} symbols)", -(-n_sym // f), cap)
    ofdm_both_ways(ctx, o, n, n_sym, bins_, parity)
    o.close()


@gpu
def test_ofdm_general_route_copies(ctx):
    n, g = 600, 150
    bins_ = np.random.default_rng(n).permutation(n)[:450]
    k = len(bins_)
    cap = 32 * cus_of(ctx)
    n_sym = (2 * cap * 256) // k + cap // 9 + 3
    assert n_sym * n > 2 * 32 * cus_of(ctx) * 256
    o = Ofdm(ctx, n, g, bins_)
    assert o.route.startswith("general: ")
    for what, total in (("strip", n_sym * n), ("pick", n_sym * k), ("place", n_sym * n), ("prefix", n_sym * (n + g))):
        looped(f"ofdm_{what}_kernel (blocks of 256 elements)", -(-total // 256), cap)
    ofdm_both_ways(ctx, o, n, n_sym, bins_, 1)
    o.close()
    _OFDM.clear()


# ---- f: bit packing --------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("order,lsb", ((crc.LSB_FIRST, True), (crc.MSB_FIRST, False)))
def test_bits_pack_and_unpack(ctx, order, lsb):
    from test_gpu_turbo import Mem
    cap = 16 * cus_of(ctx)
    nbits = 16 * 256 * (2 * cap + cap // 3) + 16 * 100 + 7            # odd, the last block and the last chunk partial
    nbytes = (nbits + 7) // 8
    assert nbits % 2 == 1 and nbits // 16 > 2 * 16 * cus_of(ctx) * 256
    looped("bits_pack_kernel (blocks of 256 chunks of 16 bits)", -(-((nbits + 15) // 16) // 256), cap)
    looped("bits_unpack_kernel, output at byte 3 (blocks of 256 chunks of 16 bits)", -(-((nbits + 3 + 15) // 16) // 256), cap)
    x = np.random.default_rng(nbits + order).integers(0, 256, nbits, dtype=np.uint8)
    want = crc_truth.pack(x, lsb)
    assert want.tobytes() == np.packbits(x & 1, bitorder="little" if lsb else "big").tobytes()
    lib, mem = _lib.load(), Mem(ctx)
    try:
        o = mem.out(nbytes, 5)
        _lib.check(lib.aeth_bits_pack(ctx.h, mem.inp(x, 1), nbits, order, mem.ptr(o), nbytes))
        got = mem.get(o)
        assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want)[:8]
        mem.free()
        o = mem.out(nbits, 3)
        _lib.check(lib.aeth_bits_unpack(ctx.h, mem.inp(want, 2), nbytes, order, mem.ptr(o), nbits))
        got = mem.get(o)
        assert got.tobytes() == (x & 1).tobytes(), np.flatnonzero(got != (x & 1))[:8]
    finally:
        mem.free()


# ---- g: the other capped loops: a long call equals the same frames in calls that fit inside the cap --------------------
def long_call_equals_short_calls(ctx, f, n, batch, piece, sign=+1, scale=Scale.SN):
    """one call over `batch` frames against calls of at most `piece` frames, the whole batch, with sentinels behind it"""
    sent = np.complex64(complex(-7.25, 1234.5))
    x = signal(n * batch, n + batch)
    xin = ctx.vec(x)
    big = ctx.vec(np.full(n * batch + 8, sent, np.complex64))
    f.exec(xin, big.slice(0, n * batch), sign, scale)
    got = big.to_host()
    assert (got[n * batch:].view(np.uint64) == np.array([sent]).view(np.uint64)[0]).all(), "wrote behind the output"
    got = got[:n * batch].reshape(batch, n)
    out = ctx.empty(n * piece)
    for lo in range(0, batch, piece):
        hi = min(lo + piece, batch)
        f.exec(xin.slice(lo * n, hi * n), out.slice(0, (hi - lo) * n), sign, scale)
        part = out.slice(0, (hi - lo) * n).to_host().reshape(hi - lo, n)
        assert bits_equal(part, got[lo:hi]), (n, lo, np.flatnonzero((part.view(np.uint64) != got[lo:hi].view(np.uint64)).any(axis=1))[:8] + lo)


POW2_STAGED = {16: 64, 64: 8, 256: 4}                 # length: frames per workgroup, T = N / P < 24 lanes per frame


@gpu
@pytest.mark.parametrize("n", sorted(POW2_STAGED))
def test_fft_pow2_staged_batch_equals_short_calls(ctx, n):
    fr = POW2_STAGED[n]
    cap = 8 * cus_of(ctx)
    batch = fr * (2 * cap + cap // 3) + 1
    f = HipFft(ctx, n)
    assert f.algorithm == "stockham_pow2"
    looped(f"fft_pow2_kernel N = {n} (groups of {fr} frames)", -(-batch // fr), cap)
    long_call_equals_short_calls(ctx, f, n, batch, fr * (cap // 2) - 1, sign=+1 if n != 64 else -1)


def mixed_frames_per_workgroup(n):
    """launch_mixed of aeth_fft.hip for a length with a radix that has no register form: two LDS images per frame"""
    frame_bytes, tpf = 2 * n * 8, 8
    while tpf < 256 and (256 // tpf) * frame_bytes > 36 * 1024:
        tpf <<= 1
    return 256 // tpf


@gpu
def test_fft_mixed_batch_equals_short_calls(ctx):
    n = 2057                                          # 11 * 11 * 17: no row in the ragged table, too long for one-launch chirp-z
    fr = mixed_frames_per_workgroup(n)
    cap = 8 * cus_of(ctx)
    batch = fr * 2 * cap + 3                           # 67 MB each way: no third trip here
    f = HipFft(ctx, n)
    assert f.algorithm == "stockham_mixed" and fr == 1
    looped(f"fft_mixed_kernel N = {n} (groups of {fr} frames)", -(-batch // fr), cap)
    long_call_equals_short_calls(ctx, f, n, batch, fr * (cap // 4))


@gpu
def test_bluestein_copies_batch_equals_short_calls(ctx):
    n, m = 8193, 16875
    cap = 8 * cus_of(ctx)
    batch = (2 * cap * 256) // n + cap // 48 + 3
    piece = (cap * 256) // m - 1                      # blu_pre and blu_mul walk m * frames elements, blu_post n * frames
    f = HipFft(ctx, n, max_batch=batch)
    assert f.algorithm == "bluestein" and f"M={m})" in f.route, f.route
    looped("blu_post (blocks of 256 elements)", -(-(n * batch) // 256), cap)
    looped("blu_pre, blu_mul (blocks of 256 elements)", -(-(m * batch) // 256), cap)
    assert -(-(m * piece) // 256) <= cap
    long_call_equals_short_calls(ctx, f, n, batch, piece)
