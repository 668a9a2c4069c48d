"""GPU: the polyphase rational resampler (csrc/aeth_resamp.hip, aeth_resamp_*) bit for bit against the numpy restatement
of its definition (tests/resamp_truth.py), against the FIR that exists, and its refusals.

Launch geometry (T = aeth_resamp_tile).  Staged route: a 256-lane workgroup makes T consecutive outputs, T the largest
multiple of 256 (at most 4096) whose input span floor((U - 1 + (T - 1) Q) / U) + P fits 4096 samples of LDS.  Direct
route, when not even 256 outputs fit (Q / U above about 16): T = 256, every lane reads its own P samples.  With P = 16 and
U = 1 the switch lies between Q = 16 (staged, T = 256) and Q = 17 (direct).  The shapes below are the smallest at which
each mechanism can break; a call makes a T + b outputs rounded up to whole periods of U."""
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

import chan_truth                                                          # noqa: E402
import resamp_truth                                                        # noqa: E402
from helpers import bits_equal, rand_c64                                   # noqa: E402

import aether_primitives_amd as ap                                         # noqa: E402
from aether_primitives_amd import _lib                                     # noqa: E402

pytestmark = pytest.mark.gpu

MUTUAL_DB = -114.0                                # two results each within -120 dB of f64 (tests/test_gpu_fft.py:20)
GUARD = 16                                        # samples: keeps a 16-byte aligned buffer 16-byte aligned
SENT = np.complex64(-7.5 + 3.25j)

# (U, Q, P, (a, b): outputs = a T + b rounded up to whole periods, route)
SHAPES = [
    (1, 1, 1, (1, 5), "staged u1"),
    (1, 1, 5, (1, 5), "staged u1"),
    (2, 1, 4, (1, 5), "staged"),
    (1, 2, 4, (1, 7), "staged u1"),
    (3, 2, 8, (2, 3), "staged"),                  # two tile edges plus a ragged last tile
    (2, 3, 3, (1, 5), "staged"),
    (147, 160, 4, (1, 3), "staged"),
    (160, 147, 16, (1, 3), "staged"),
    (7, 5, 64, (1, 9), "staged"),                 # P at its limit
    (64, 1, 1, (1, 3), "staged"),
    (1, 64, 2, (2, 3), "direct u1"),              # inputs skipped
    (5, 4096, 3, (1, 3), "direct"),
    (4096, 4095, 2, (1, 5), "staged"),            # one period wider than a tile
    (1, 16, 16, (2, 3), "staged u1"),             # the last Q / U the staged route takes at P = 16: T = 256
    (1, 17, 16, (2, 3), "direct u1"),             # the first it does not
]
IDS = [f"U{u}-Q{q}-P{p}-{a}T+{b}" for u, q, p, (a, b), _ in SHAPES]
ONE_PER_ROUTE = [SHAPES[4], SHAPES[7], SHAPES[10], SHAPES[11], SHAPES[13]]


def taps_of(U, P, seed=0):
    """taps without structure: every tap distinct and nonzero, both signs"""
    return np.random.default_rng(1000 * U + P + seed).standard_normal(U * P).astype(np.float32)


@functools.lru_cache(maxsize=None)
def resamp_of(ctx, U, Q, P):
    return ap.Resampler(ctx, taps_of(U, P), U, Q)


def case(ctx, shape):
    U, Q, P, (a, b), _ = shape
    rs = resamp_of(ctx, U, Q, P)
    B = -(-(a * rs.tile + b) // U)
    x = rand_c64(U * 7 + Q * 3 + P, B * Q)
    hist = rand_c64(U + Q + P + 99, P - 1)
    return rs, B, x, hist


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
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exec_is_the_definition_bit_for_bit(ctx, shape):
    U, Q, P, (a, b), route = shape
    rs, B, x, hist = case(ctx, shape)
    assert rs.up == U and rs.down == Q and rs.ntaps == U * P and rs.history == P - 1
    assert rs.route == route, rs.route
    assert rs.tile % 256 == 0 and 256 <= rs.tile <= 4096 and (route.startswith("staged") or rs.tile == 256)
    assert rs.out_count(x.size) == B * U and rs.out_count(x.size + 1) == (0 if Q > 1 else (B + 1) * U)
    assert B * U > a * rs.tile                                            # the call crosses the tile edges it is meant to
    h = taps_of(U, P)
    dh = ctx.vec(hist) if hist.size else None
    for use_hist in ((False, True) if hist.size else (False,)):
        want = resamp_truth.resamp(h, U, Q, x, hist if use_hist else None)
        for in_off, out_off in ((0, 0), (1, 0), (0, 1), (1, 1)):
            xin = at_offset(ctx, x, in_off)
            big, out = guarded(ctx, B * U, out_off)
            rs.exec(xin, dh if use_hist else None, out)
            what = (use_hist, in_off, out_off)
            assert bits_equal(out.to_host(), want), what
            assert guards_intact(big, B * U, out_off), what
    if dh is not None:                                                    # a history that is only 8-byte aligned
        want = resamp_truth.resamp(h, U, Q, x, hist)
        assert bits_equal(rs.exec(ctx.vec(x), at_offset(ctx, hist, 1)).to_host(), want)


# ---- 2. special values ------------------------------------------------------------------------------------------------
def test_minus_zero_through_a_single_tap(ctx):
    rs = ap.Resampler(ctx, np.array([1.0], np.float32), 1, 1)
    got = rs.exec(ctx.vec(np.array([complex(-0.0, -0.0)] * 5, np.complex64))).to_host()
    assert got.view(np.uint32).tolist() == [0x80000000] * 10


@pytest.mark.parametrize("shape", ONE_PER_ROUTE, ids=[IDS[SHAPES.index(s)] for s in ONE_PER_ROUTE])
def test_inf_and_nan_poison_exactly_the_outputs_that_cover_them(ctx, shape):
    U, Q, P, _, _ = shape
    rs, B, x, hist = case(ctx, shape)
    x = x.copy()
    i_inf = x.size // 3
    i_nan = int(((np.arange(B * U, dtype=np.int64) * Q) // U).max())      # the newest sample any output reads
    x.real[i_inf] = np.inf
    x.imag[i_nan] = np.nan
    want = resamp_truth.resamp(taps_of(U, P), U, Q, x, hist if hist.size else None)
    got = rs.exec(ctx.vec(x), ctx.vec(hist) if hist.size else None).to_host()
    assert chan_truth.same_bits(got, want)
    c_inf, c_nan = (resamp_truth.covers(U, Q, P, B * U, i) for i in (i_inf, i_nan))
    assert c_nan.any() and (c_inf.any() or Q >= P * U)                    # strong decimation may skip a sample entirely
    assert (~np.isfinite(got.real) == c_inf).all() and (np.isnan(got.imag) == c_nan).all()


def test_null_history_is_a_history_of_plus_zero(ctx):
    """with negative taps the zeros are still multiplied: -t * +0.0 = -0.0 enters the sum either way"""
    for U, Q, P in ((3, 2, 8), (1, 64, 2)):
        h = -np.abs(taps_of(U, P)) - 1.0
        rs = ap.Resampler(ctx, h, U, Q)
        x = rand_c64(5, 40 * Q)
        x[:P] = 0                                                         # the first outputs are sums of signed zeros only
        a = rs.exec(ctx.vec(x), None).to_host()
        b = rs.exec(ctx.vec(x), ctx.vec(np.zeros(P - 1, np.complex64))).to_host()
        assert bits_equal(a, b) and bits_equal(a, resamp_truth.resamp(h, U, Q, x))
        assert a.view(np.uint32)[0] == 0x80000000                         # (-t) * (+0.0) + ... = -0.0


# ---- 3. chunks of a stream concatenate ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_two_calls_with_history_equal_one(ctx, shape):
    U, Q, P, _, _ = shape
    rs, B, x, _ = case(ctx, shape)
    B1 = max(1, -(-(P - 1) // Q))                                         # periods of the first call: enough samples for a history
    while (B1 * U) % rs.tile == 0:                                        # ... and no tile multiple
        B1 += 1
    B += B1
    x = rand_c64(U + Q + P + 5, B * Q)
    xin = ctx.vec(x)
    whole = rs.exec(xin).to_host()
    cut = B1 * Q
    hist = xin.slice(cut - (P - 1), cut) if P > 1 else None
    parts = np.concatenate([rs.exec(xin.slice(0, cut)).to_host(), rs.exec(xin.slice(cut, x.size), hist).to_host()])
    assert bits_equal(parts, whole)
    assert bits_equal(whole, resamp_truth.resamp(taps_of(U, P), U, Q, x))


# ---- 4. relations to what exists --------------------------------------------------------------------------------------
def test_identity(ctx):
    rs = ap.Resampler(ctx, np.array([1.0], np.float32), 1, 1)
    x = rand_c64(3, 2 * rs.tile + 77)
    assert bits_equal(rs.exec(ctx.vec(x)).to_host(), x)


@pytest.mark.parametrize("dec", (1, 4))
def test_against_the_fir(ctx, dec):
    """U = 1 with 64 real taps is aeth_fir_exec (dec = 1) / aeth_fir_exec_decim of the same taps: two roads to the same
    f64 truth, each within -120 dB of it, so at most -114 dB apart"""
    h = taps_of(1, 64, 7)
    n = 1984 * 4
    x = rand_c64(11 + dec, n)
    hist = rand_c64(12, 63)
    fir = ap.Fir(ctx, h.astype(np.complex64), 2048)
    rs = ap.Resampler(ctx, h, 1, dec)
    xin, dh = ctx.vec(x), ctx.vec(hist)
    for hh in (None, dh):
        want = (fir.filter(xin, hist=hh) if dec == 1 else fir.filter_decim(xin, dec, hist=hh)).to_host()
        got = rs.exec(xin, hh).to_host()
        assert got.size == want.size == n // dec
        db = db_apart(got, want)
        print(f"dec {dec}, history {hh is not None}: {db:.1f} dB apart")
        assert db <= MUTUAL_DB, db


# ---- 5. reproducible, whatever the cache policy ---------------------------------------------------------------------------
REPRO = ONE_PER_ROUTE


def _repro_bytes(ctx, shape):
    rs, B, x, hist = case(ctx, shape)
    return rs.exec(ctx.vec(x), ctx.vec(hist) if hist.size else None).to_host().tobytes()


def _child(outdir):
    ctx = ap.Context(0)
    for nt in ("0", "1"):
        os.environ["AETH_NT"] = nt
        for i, shape in enumerate(REPRO):
            with open(os.path.join(outdir, f"nt{nt}_{i}.bin"), "wb") as f:
                f.write(_repro_bytes(ctx, shape))
    resamp_of.cache_clear()
    ctx.close()
    print("resamp child ok")


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
        with _refused(_lib.E_ARG, "64 taps", "up 5"):
            ap.Resampler(ctx, w, 5, 1)
        with _refused(_lib.E_ARG, "up 0"):
            ap.Resampler(ctx, w, 0, 1)
        with _refused(_lib.E_ARG, "down 0"):
            ap.Resampler(ctx, w, 4, 0)
        with _refused(_lib.E_UNSUPPORTED, "65 taps per phase", "64"):
            ap.Resampler(ctx, np.ones(130, np.float32), 2, 3)
        with _refused(_lib.E_UNSUPPORTED, "up 4097", "4096"):
            ap.Resampler(ctx, np.ones(4097, np.float32), 4097, 1)
        with _refused(_lib.E_UNSUPPORTED, "down 4097", "4096"):
            ap.Resampler(ctx, w, 4, 4097)
    lib, h = _lib.load(), C.c_void_p(0x55)
    assert lib.aeth_resamp_create(ctx.h, None, 64, 4, 3, C.byref(h)) == _lib.E_ARG and not h.value
    assert lib.aeth_resamp_create(ctx.h, w.ctypes.data_as(C.c_void_p), 0, 4, 3, C.byref(h)) == _lib.E_ARG
    assert b"0 taps" in lib.aeth_last_error()
    assert lib.aeth_resamp_create(ctx.h, w.ctypes.data_as(C.c_void_p), 64, 4, 3, None) == _lib.E_ARG
    ctx.sync()
    assert _free_bytes() == free0
    rs = ap.Resampler(ctx, np.ones(4096 * 64, np.float32), 4096, 4096)       # every limit is served
    assert rs.history == 63 and rs.out_count(4096) == 4096


def test_exec_refusals_launch_nothing(ctx):
    U, Q, P = 3, 2, 8
    rs = resamp_of(ctx, U, Q, P)
    lib = _lib.load()
    n, no = 5 * Q, 5 * U
    x, hist = ctx.vec(rand_c64(1, n + 2)), ctx.vec(rand_c64(2, P - 1))
    sentinel = np.full(no + 2, 1.5 - 2.5j, np.complex64)
    out = ctx.vec(sentinel)
    X, H, O = x.ptr, hist.ptr, out.ptr
    p = C.c_void_p

    def ex(c=rs.h, h=H, i=X, nn=n, o=O, nout=no):
        return lib.aeth_resamp_exec(c, p(h), p(i), nn, p(o), nout)

    def err(rc, code, *words):
        msg = lib.aeth_last_error().decode()
        assert rc == code, (rc, msg)
        assert all(w in msg for w in words), msg

    err(ex(c=None), _lib.E_ARG, "resamp", "null")
    err(ex(i=None), _lib.E_ARG, "null")
    err(ex(o=None), _lib.E_ARG, "null")
    err(ex(nn=0, nout=0), _lib.E_LEN, "0 input samples")
    err(ex(nn=n + 1), _lib.E_LEN, f"{n + 1} input samples", "down 2")
    err(ex(nout=no - 1), _lib.E_LEN, f"{no - 1} elements", "5 periods", "up 3", f"{no}")
    err(ex(nout=no + 1), _lib.E_LEN, f"{no + 1} elements")
    err(ex(i=X + 4), _lib.E_ALIGN, "8-byte aligned")
    err(ex(h=H + 4), _lib.E_ALIGN, "8-byte aligned")
    err(ex(o=O + 4), _lib.E_ALIGN, "8-byte aligned")
    # the output range must be clear of the input and of the history
    err(ex(o=X), _lib.E_ARG, "overlaps")
    err(ex(o=X + 8 * (n - 1)), _lib.E_ARG, "overlaps")
    err(ex(i=O + 8 * (no - 1), o=O), _lib.E_ARG, "overlaps")
    err(ex(h=O + 8 * (no - 1), o=O), _lib.E_ARG, "overlaps")
    err(ex(o=H + 8 * (P - 2)), _lib.E_ARG, "overlaps")
    # sizes that would overflow an element count or the grid: refused before any pointer is followed
    huge = (2 ** 64 // 16 // U + 2) // Q * Q
    err(ex(nn=huge, nout=huge // Q * U), _lib.E_UNSUPPORTED, f"{huge} input samples", "overflow")
    assert rs.out_count(huge) == 0
    grid_n = (2 ** 31 * rs.tile + U - 1) // U * Q                             # outputs for 2^31 workgroups, in whole periods
    err(lib.aeth_resamp_exec(rs.h, None, p(0x1000), grid_n, p(2 ** 62), grid_n // Q * U), _lib.E_UNSUPPORTED,
        f"{grid_n // Q * U} outputs", "2^31 workgroups")
    ctx.sync()
    assert bits_equal(out.to_host(), sentinel)                       # nothing was launched
    # and the same arguments, made right, run: the object is still usable
    assert ex() == 0
    ctx.sync()
    got = out.to_host()
    assert bits_equal(got[:no], resamp_truth.resamp(taps_of(U, P), U, Q, x.to_host()[:n], hist.to_host()))
    assert bits_equal(got[no:], sentinel[no:])
    with pytest.raises(ap.LengthMismatch):
        rs.exec(x.slice(0, n), ctx.vec(rand_c64(3, 5)))               # the Python mirror checks the history's length
    with pytest.raises(ap.LengthMismatch):
        rs.exec(x.slice(0, n + 1))


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--child":
    _child(sys.argv[2])
