"""GPU: the arbitrary-ratio resampler (csrc/aeth_arb.hip, aeth_arb_*) bit for bit against the numpy restatement of its
definition (tests/arb_truth.py), against the rational resampler where the step is an exact fraction, and its refusals.

Launch geometry (T = aeth_arb_tile(step)).  Staged route: a 256-lane workgroup makes T consecutive outputs, T the largest
multiple of 256 (at most 4096) with floor((2^32 - 1 + (T - 1) step) / 2^32) + P <= 4096 samples of LDS, that is
(T - 1) step <= (4096 - P) 2^32; "staged tab" when the table, L rows of ceil(P / 2) 16-byte slots, is at most 512 slots and
lies in LDS too.  Direct route, when not even 256 outputs fit: T = 256, every lane reads its own P samples.
With P = 16 the switch lies between step = 4080 / 255 = 16 exactly (staged, T = 256) and 16 + 2^-32 (direct).  The shapes
below are the smallest at which each mechanism can break; a call makes at least a T + b outputs."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):                             # also run as a script: the AETH_NT child
    if _p not in sys.path:
        sys.path.insert(0, _p)

import arb_truth                                                           # noqa: E402
import chan_truth                                                          # noqa: E402
from helpers import bits_equal, rand_c64                                   # noqa: E402

import aether_primitives_amd as ap                                         # noqa: E402
from aether_primitives_amd import _lib, resamp                             # noqa: E402

pytestmark = pytest.mark.gpu

TOL_DB = -120.0                                   # tests/test_gpu_fft.py:20
GUARD = 16                                        # samples: keeps a 16-byte aligned buffer 16-byte aligned
SENT = np.complex64(-7.5 + 3.25j)
ONE = 1 << 32
MIN_STEP, MAX_STEP = 1 << 20, 1 << 44
PHASES = (0, ONE - 1, 3 * ONE + 12345)            # ONE - 1: r = L - 1 and the largest mu, reaching h[T] = 0


def word(ratio):
    return int(float(ratio) * 4294967296.0)


LAST_STAGED_P16 = ((4096 - 16) << 32) // 255      # (256 - 1) step <= (4096 - 16) 2^32: the tile rule at T = 256

# (b, P, step, (a, b'): at least a T + b' outputs, route)
SHAPES = [
    (0, 1, ONE, (1, 5), "staged tab"),
    (0, 2, ONE - 1, (1, 5), "staged tab"),
    (3, 5, ONE + 1, (1, 5), "staged tab"),
    (5, 8, word(0.731), (2, 3), "staged tab"),                    # two tile edges plus a ragged last tile
    (8, 16, word(160 / 147 * (1 + 2e-5)), (1, 3), "staged"),  # 2048 slots of 16 bytes: the table stays in memory
    (12, 2, MIN_STEP, (1, 5), "staged"),                      # the minimum step: 4096 outputs per input sample
    (6, 64, word(0.7), (1, 9), "staged"),                     # P at its limit
    (4, 64, word(0.7), (1, 9), "staged tab"),                 # ... with the last table that lies in LDS: 512 slots
    (5, 31, word(1.37), (1, 9), "staged tab"),                # an odd P: 16 slots a row, the last half used
    (5, 33, word(1.37), (1, 9), "staged"),                    # 544 slots: the first table that does not
    (4, 16, LAST_STAGED_P16, (2, 3), "staged tab"),               # the last step the staged route takes at P = 16: T = 256
    (4, 16, LAST_STAGED_P16 + 1, (2, 3), "direct"),           # the first it does not
    (4, 3, MAX_STEP, (1, 3), "direct"),                       # the maximum step: 4093 inputs skipped between outputs
]
IDS = [f"b{b}-P{p}-step{s}-{a}T+{r}" for b, p, s, (a, r), _ in SHAPES]
ONE_PER_ROUTE = [SHAPES[3], SHAPES[4], SHAPES[8], SHAPES[10], SHAPES[11], SHAPES[12]]


def taps_of(b, P, seed=0):
    """taps without structure: every tap distinct and nonzero, both signs"""
    return np.random.default_rng(1000 * b + P + seed).standard_normal(P << b).astype(np.float32)


@functools.lru_cache(maxsize=None)
def arb_of(ctx, b, P):
    return ap.ArbResampler(ctx, taps_of(b, P), b)


def case(ctx, shape, phase=0):
    """the object, an input long enough for a T + b' outputs from `phase`, and a history"""
    b, P, step, (a, r), _ = shape
    rs = arb_of(ctx, b, P)
    n = ((phase + (a * rs.tile(step) + r) * step) >> 32) + 1
    x = rand_c64(7 * b + 3 * P + (step & 0xffff), n)
    hist = rand_c64(b + P + 99, P - 1)
    return rs, x, hist


def guarded(ctx, n, off=0):
    """a device vector of n samples `off` samples into a buffer with sentinels on both sides"""
    big = ctx.vec(np.full(n + 2 * GUARD + off, SENT, np.complex64))
    return big, big.slice(GUARD + off, GUARD + off + n)


def guards_intact(big, n, off=0):
    h = big.to_host()
    return bool((h[:GUARD + off] == SENT).all() and (h[GUARD + off + n:] == SENT).all())


def at_offset(ctx, x, off):
    big = ctx.vec(np.concatenate([np.zeros(off, np.complex64), x]))
    return big.slice(off, off + x.size)


def db_apart(got, want):
    got, want = np.asarray(got).astype(np.complex128), np.asarray(want).astype(np.complex128)
    return 20 * np.log10(max(np.linalg.norm(got - want), 1e-300) / np.linalg.norm(want))


# ---- 1. the definition, bit for bit --------------------------------------------------------------------------------------
def test_the_route_switch_follows_the_tile_rule(ctx):
    rs = arb_of(ctx, 4, 16)
    assert LAST_STAGED_P16 == 16 * ONE
    assert (rs.route(LAST_STAGED_P16), rs.tile(LAST_STAGED_P16)) == ("staged tab", 256)
    assert (rs.route(LAST_STAGED_P16 + 1), rs.tile(LAST_STAGED_P16 + 1)) == ("direct", 256)
    assert rs.tile(ONE) == 3840 and rs.tile(MIN_STEP) == 4096         # (4096 - 16) + 1 = 4081 outputs fit: 15 x 256
    assert rs.tile(MIN_STEP - 1) == 0 and rs.route(MAX_STEP + 1) == ""
    for step in (MIN_STEP, word(0.731), ONE, word(4.0001), LAST_STAGED_P16):
        T = rs.tile(step)                                               # the rule itself, and T + 256 breaks it (or the cap)
        assert ((ONE - 1) + (T - 1) * step) // ONE + 16 <= 4096
        assert T == 4096 or ((ONE - 1) + (T + 255) * step) // ONE + 16 > 4096


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exec_is_the_definition_bit_for_bit(ctx, shape):
    b, P, step, (a, r), route = shape
    h = taps_of(b, P)
    for phase in PHASES:
        rs, x, hist = case(ctx, shape, phase)
        assert rs.phases == 1 << b and rs.ntaps == P << b and rs.history == P - 1
        assert rs.route(step) == route, rs.route(step)
        T = rs.tile(step)
        assert T % 256 == 0 and 256 <= T <= 4096 and (route.startswith("staged") or T == 256)
        count, nxt = rs.advance(step, phase, x.size)
        assert count >= a * T + r and (count, nxt) == arb_truth.advance(step, phase, x.size)     # crosses the tile edges it is meant to
        dh = ctx.vec(hist) if hist.size else None
        for use_hist in ((False, True) if hist.size else (False,)):
            want = arb_truth.arb(h, b, x, step, phase, hist if use_hist else None)
            assert want.size == count
            for in_off, out_off in ((0, 0), (1, 0), (0, 1), (1, 1)):
                xin = at_offset(ctx, x, in_off)
                big, out = guarded(ctx, count, out_off)
                rs.exec(xin, step, phase, dh if use_hist else None, out)
                what = (phase, use_hist, in_off, out_off)
                assert bits_equal(out.to_host(), want), what
                assert guards_intact(big, count, out_off), what
        if dh is not None:                                                    # a history that is only 8-byte aligned
            want = arb_truth.arb(h, b, x, step, phase, hist)
            assert bits_equal(rs.exec(ctx.vec(x), step, phase, at_offset(ctx, hist, 1)).to_host(), want)


# ---- 2. special values ------------------------------------------------------------------------------------------------
def test_minus_zero_through_a_single_tap(ctx):
    rs = ap.ArbResampler(ctx, np.array([1.0], np.float32), 0)
    got = rs.exec(ctx.vec(np.array([complex(-0.0, -0.0)] * 5, np.complex64)), ONE, 0).to_host()
    assert got.view(np.uint32).tolist() == [0x80000000] * 10


@pytest.mark.parametrize("shape", ONE_PER_ROUTE, ids=[IDS[SHAPES.index(s)] for s in ONE_PER_ROUTE])
def test_inf_and_nan_poison_exactly_the_outputs_that_cover_them(ctx, shape):
    b, P, step, _, _ = shape
    phase = 12345
    rs, x, hist = case(ctx, shape, phase)
    x = x.copy()
    a_of, _, _ = arb_truth.split(arb_truth.words(step, phase, x.size), b)
    i_inf = x.size // 3
    i_nan = int(a_of.max())                                               # the newest sample any output reads
    x.real[i_inf] = np.inf
    x.imag[i_nan] = np.nan
    want = arb_truth.arb(taps_of(b, P), b, x, step, phase, hist if hist.size else None)
    got = rs.exec(ctx.vec(x), step, phase, ctx.vec(hist) if hist.size else None).to_host()
    assert chan_truth.same_bits(got, want)
    c_inf, c_nan = (arb_truth.covers(a_of, P, i) for i in (i_inf, i_nan))
    assert c_nan.any() and (c_inf.any() or step >= P * ONE)              # a step that skips inputs may skip this one
    assert (~np.isfinite(got.real) == c_inf).all() and (np.isnan(got.imag) == c_nan).all()


def test_null_history_is_a_history_of_plus_zero(ctx):
    """with negative interpolated taps the zeros are still multiplied: -c * +0.0 = -0.0 enters the sum either way.
    Constant taps of -2 interpolate to -2, and behind the last one to -2 + 2 mu <= -2^-23."""
    for b, P, step in ((3, 8, word(0.731)), (4, 2, word(64.3))):
        h = np.full(P << b, -2.0, np.float32)
        rs = ap.ArbResampler(ctx, h, b)
        x = rand_c64(5, 4000)
        x[:P] = 0                                                         # the first output is a sum of signed zeros only
        a = rs.exec(ctx.vec(x), step, 0, None).to_host()
        z = rs.exec(ctx.vec(x), step, 0, ctx.vec(np.zeros(P - 1, np.complex64))).to_host()
        assert bits_equal(a, z) and bits_equal(a, arb_truth.arb(h, b, x, step))
        assert a.view(np.uint32)[0] == 0x80000000                         # (-c) * (+0.0) + ... = -0.0


# ---- 3. chunks of a stream concatenate ------------------------------------------------------------------------------------
# (b, P, step, cuts): the second makes nothing from the one sample between 5 and 6
STREAMS = [(5, 8, word(0.731), (1, 7, 300, 301, 977, 1500)), (4, 4, word(7.3), (5, 6, 300, 301, 977, 1500)),
           (4, 16, LAST_STAGED_P16 + 1, (5, 6, 300, 301, 977, 1500))]


@pytest.mark.parametrize("stream", STREAMS, ids=[f"b{b}-P{p}-step{s}" for b, p, s, _ in STREAMS])
@pytest.mark.parametrize("phase", (0, ONE - 1))
def test_chunks_with_carried_phase_equal_one_call(ctx, stream, phase):
    b, P, step, cuts = stream
    rs = ap.ArbResampler(ctx, taps_of(b, P), b)
    n = ((2 * rs.tile(step) + 77) * step >> 32) + 1                       # the single call crosses two tile edges
    assert n > cuts[-1]
    x = rand_c64(b + P + 5, n)
    xin = ctx.vec(x)
    whole = rs.exec(xin, step, phase).to_host()
    assert bits_equal(whole, arb_truth.arb(taps_of(b, P), b, x, step, phase))
    rs.phase = phase                                                      # the object carries the phase from here on
    parts, empty = [], 0
    for lo, hi in zip((0,) + cuts, cuts + (n,)):
        hist = None
        if lo and P > 1:
            hist = xin.slice(lo - (P - 1), lo) if lo >= P - 1 else ctx.vec(np.concatenate([np.zeros(P - 1 - lo, np.complex64), x[:lo]]))
        before = rs.phase
        part = rs.exec(xin.slice(lo, hi), step, hist=hist)
        assert (part.n, rs.phase) == arb_truth.advance(step, before, hi - lo)
        empty += part.n == 0
        parts.append(part.to_host())
    assert empty >= 1 if step > 2 * ONE else empty == 0                  # a single sample under a step above 2 may make nothing
    assert bits_equal(np.concatenate(parts), whole)
    assert rs.phase == arb_truth.advance(step, phase, n)[1]


def test_a_call_over_no_samples_makes_nothing_and_keeps_the_phase(ctx):
    rs = arb_of(ctx, 5, 8)
    x = ctx.vec(rand_c64(1, 16))
    out = rs.exec(x.slice(3, 3), word(0.731), 777)
    assert out.n == 0 and rs.advance(word(0.731), 777, 0) == (0, 777)


def test_the_step_may_change_between_chunks(ctx):
    b, P = 5, 8
    h = taps_of(b, P)
    rs = ap.ArbResampler(ctx, h, b)
    s1, s2, cut = word(0.731), word(0.7310021), 3001
    x = rand_c64(21, 3001 + 2999)
    xin = ctx.vec(x)
    rs.phase = 4242
    p0 = rs.phase
    first = rs.exec(xin.slice(0, cut), s1).to_host()
    p1 = rs.phase
    second = rs.exec(xin.slice(cut, x.size), s2, hist=xin.slice(cut - (P - 1), cut)).to_host()
    assert p1 == arb_truth.advance(s1, p0, cut)[1] and rs.phase == arb_truth.advance(s2, p1, x.size - cut)[1]
    assert bits_equal(first, arb_truth.arb(h, b, x[:cut], s1, p0))
    assert bits_equal(second, arb_truth.arb(h, b, x[cut:], s2, p1, x[cut - (P - 1):cut]))


# ---- 4. relations to what exists --------------------------------------------------------------------------------------
def test_identity(ctx):
    rs = ap.ArbResampler(ctx, np.array([1.0], np.float32), 0)
    x = rand_c64(3, 2 * rs.tile(ONE) + 77)
    assert bits_equal(rs.exec(ctx.vec(x), ONE, 0).to_host(), x)


@pytest.mark.parametrize("b,Q,P", ((3, 5, 8), (6, 147, 16)))
def test_an_exact_fraction_is_the_rational_resampler(ctx, b, Q, P):
    """step = Q 2^32 / L exactly and phase 0: mu is 0 throughout and c_p = h + 0 * d = h, but for the sign of a zero tap"""
    L = 1 << b
    h = resamp.prototype(L, Q, P)
    step = (Q << 32) >> b
    assert step << b == Q << 32
    ar, rr = ap.ArbResampler(ctx, h, b), ap.Resampler(ctx, h, L, Q)
    B = -(-(2 * max(ar.tile(step), rr.tile) + 9) // L)
    x = rand_c64(31 + b, B * Q)
    hist = rand_c64(32 + b, P - 1)
    xin, dh = ctx.vec(x), ctx.vec(hist)
    for hh in (None, dh):
        got, want = ar.exec(xin, step, 0, hh).to_host(), rr.exec(xin, hh).to_host()
        assert got.size == want.size == B * L
        assert (got == want).all()                                       # values: a tap of -0.0 becomes +0.0 here
    assert ar.advance(step, 0, x.size) == (B * L, 0)


def test_accuracy_against_complex128(ctx):
    b, P, step, phase = 6, 16, word(0.91876), ONE - 1
    h = taps_of(b, P)
    x = rand_c64(8, 900)
    got = ap.ArbResampler(ctx, h, b).exec(ctx.vec(x), step, phase).to_host()
    db = db_apart(got, arb_truth.arb_f64(h, b, x, step, phase))
    print(f"b {b}, P {P}, step {step / ONE:.5f}: {db:.1f} dB")
    assert db <= TOL_DB, db


# ---- 5. reproducible, whatever the cache policy ---------------------------------------------------------------------------
REPRO = ONE_PER_ROUTE


def _repro_bytes(ctx, shape):
    rs, x, hist = case(ctx, shape, ONE - 1)
    return rs.exec(ctx.vec(x), shape[2], ONE - 1, ctx.vec(hist) if hist.size else None).to_host().tobytes()


def _child(outdir):
    ctx = ap.Context(0)
    for nt in ("0", "1"):
        os.environ["AETH_NT"] = nt
        for i, shape in enumerate(REPRO):
            with open(os.path.join(outdir, f"nt{nt}_{i}.bin"), "wb") as f:
                f.write(_repro_bytes(ctx, shape))
    arb_of.cache_clear()
    ctx.close()
    print("arb child ok")


def test_results_are_reproducible_under_both_cache_policies(ctx, tmp_path):
    env = dict(os.environ, AETH_TUNING="1")
    env.pop("AETH_NT", None)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child", str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    for i, shape in enumerate(REPRO):
        want = _repro_bytes(ctx, shape)
        assert _repro_bytes(ctx, shape) == want, "two runs differ"
        for nt in ("0", "1"):
            assert open(tmp_path / f"nt{nt}_{i}.bin", "rb").read() == want, f"AETH_NT={nt} changed the result of {shape}"


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------
def _refused(code, *words):
    class _Ctx:
        def __enter__(self):
            return self

        def __exit__(self, et, ev, tb):
            assert et is not None and issubclass(et, ap.AetherError), "the call was not refused"
            msg = str(ev)
            assert ev.code == code, msg
            assert all(w in msg for w in words), msg
            return True
    return _Ctx()


def _free_bytes():
    hip = _lib.load()                              # hipMemGetInfo of the runtime the library is bound to
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_create_refusals_leave_nothing_allocated(ctx):
    w = np.ones(64, np.float32)
    ctx.sync()
    free0 = _free_bytes()
    for _ in range(20):
        with _refused(_lib.E_ARG, "64 taps", "128 phases"):
            ap.ArbResampler(ctx, w, 7)
        with _refused(_lib.E_ARG, "63 taps", "4 phases"):
            ap.ArbResampler(ctx, w[:63], 2)
        with _refused(_lib.E_UNSUPPORTED, "log2_phases 13", "12"):
            ap.ArbResampler(ctx, np.ones(8192, np.float32), 13)
        with _refused(_lib.E_UNSUPPORTED, "65 taps per phase", "64"):
            ap.ArbResampler(ctx, np.ones(130, np.float32), 1)
    lib, h = _lib.load(), C.c_void_p(0x55)
    assert lib.aeth_arb_create(ctx.h, None, 64, 2, C.byref(h)) == _lib.E_ARG and not h.value
    assert lib.aeth_arb_create(ctx.h, w.ctypes.data_as(C.c_void_p), 0, 2, C.byref(h)) == _lib.E_ARG
    assert b"0 taps" in lib.aeth_last_error()
    assert lib.aeth_arb_create(ctx.h, w.ctypes.data_as(C.c_void_p), 64, 2, None) == _lib.E_ARG
    ctx.sync()
    assert _free_bytes() == free0
    rs = ap.ArbResampler(ctx, np.ones(4096 * 64, np.float32), 12)            # every limit is served
    assert rs.history == 63 and rs.phases == 4096 and rs.ntaps == 4096 * 64


def test_exec_refusals_launch_nothing(ctx):
    b, P, step = 3, 8, word(0.731)
    rs = arb_of(ctx, b, P)
    lib = _lib.load()
    n = 40
    no, _ = arb_truth.advance(step, 0, n)
    x, hist = ctx.vec(rand_c64(1, n + 2)), ctx.vec(rand_c64(2, P - 1))
    sentinel = np.full(no + 2, 1.5 - 2.5j, np.complex64)
    out = ctx.vec(sentinel)
    X, H, O = x.ptr, hist.ptr, out.ptr
    p = C.c_void_p

    def ex(c=rs.h, h=H, i=X, nn=n, st=step, ph=0, o=O, nout=no):
        return lib.aeth_arb_exec(c, p(h), p(i), nn, st, ph, p(o), nout)

    def err(rc, code, *words):
        msg = lib.aeth_last_error().decode()
        assert rc == code, (rc, msg)
        assert all(w in msg for w in words), msg

    ctx.sync()
    free0 = _free_bytes()
    err(ex(c=None), _lib.E_ARG, "arb", "null")
    err(ex(i=None), _lib.E_ARG, "null")
    err(ex(o=None), _lib.E_ARG, "null")
    err(ex(st=MIN_STEP - 1), _lib.E_UNSUPPORTED, f"step {MIN_STEP - 1}")
    err(ex(st=MAX_STEP + 1), _lib.E_UNSUPPORTED, f"step {MAX_STEP + 1}")
    err(ex(ph=1 << 63), _lib.E_UNSUPPORTED, f"phase {1 << 63}")
    err(ex(nn=(1 << 31) + 1), _lib.E_UNSUPPORTED, f"{(1 << 31) + 1} input samples")
    err(ex(nout=no - 1), _lib.E_LEN, f"{no - 1} elements", f"{n} input samples", f"step {step}", f"give {no}")
    err(ex(nout=no + 1), _lib.E_LEN, f"{no + 1} elements")
    err(ex(ph=n * ONE, nout=no), _lib.E_LEN, f"{no} elements", "give 0")      # the phase lies behind the call: nothing to make
    err(ex(i=X + 4), _lib.E_ALIGN, "8-byte aligned")
    err(ex(h=H + 4), _lib.E_ALIGN, "8-byte aligned")
    err(ex(o=O + 4), _lib.E_ALIGN, "8-byte aligned")
    # the output range must be clear of the input and of the history
    err(ex(o=X), _lib.E_ARG, "overlaps")
    err(ex(o=X + 8 * (n - 1)), _lib.E_ARG, "overlaps")
    err(ex(i=O + 8 * (no - 1), o=O), _lib.E_ARG, "overlaps")
    err(ex(h=O + 8 * (no - 1), o=O), _lib.E_ARG, "overlaps")
    err(ex(o=H + 8 * (P - 2)), _lib.E_ARG, "overlaps")
    # a grid of 2^31 workgroups: refused before any pointer is followed
    big_n = 1 << 31
    big_no, _ = arb_truth.advance(MIN_STEP, 0, big_n)
    assert big_no // rs.tile(MIN_STEP) >= 1 << 31
    err(lib.aeth_arb_exec(rs.h, None, p(0x1000), big_n, MIN_STEP, 0, p(2 ** 62), big_no), _lib.E_UNSUPPORTED,
        f"{big_no} outputs", "2^31 workgroups")
    # a valid call that makes nothing returns without a launch
    assert ex(ph=n * ONE + 5, nout=0) == 0 and ex(nn=0, nout=0) == 0
    ctx.sync()
    assert bits_equal(out.to_host(), sentinel)                       # nothing was launched
    assert _free_bytes() == free0                                    # nothing was allocated
    # and the same arguments, made right, run: the object is still usable
    assert ex() == 0
    ctx.sync()
    got = out.to_host()
    assert bits_equal(got[:no], arb_truth.arb(taps_of(b, P), b, x.to_host()[:n], step, 0, hist.to_host()))
    assert bits_equal(got[no:], sentinel[no:])
    with pytest.raises(ap.LengthMismatch):
        rs.exec(x.slice(0, n), step, 0, ctx.vec(rand_c64(3, 5)))     # the Python mirror checks the history's length
    with pytest.raises(ap.LengthMismatch):
        rs.exec(x.slice(0, n), step, 0, None, ctx.empty(no + 1))


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--child":
    _child(sys.argv[2])
