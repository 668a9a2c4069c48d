"""GPU: the polyphase analysis filter bank (csrc/aeth_chan.hip, aeth_chan_*) against a numpy restatement of its
definition (tests/chan_truth.py): the fold bit for bit, fold + transform against complex128 under the bound of
aeth_fft_exec (-120 dB, tests/test_gpu_fft.py).

Launch geometry (T = aeth_chan_tile).  hop == M with P <= 8 runs the ring kernel: a lane owns one column (8-byte
accesses: odd M, or a pointer that is only 8-byte aligned) or two, and walks a tile of T = max(16, 16 (P - 1) rounded up
to a power of two) frames; a workgroup is 256 lanes, min(256, columns) of them along the columns and the rest along the
tiles.  Every other shape runs the general kernel: a workgroup folds T = 4096 / M whole frames (M <= 2048) or 4096
columns of one frame.  The shapes below are the smallest at which each mechanism can break."""
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
from helpers import bits_equal, rand_c64                                   # noqa: E402

import aether_primitives_amd as ap                                         # noqa: E402
from aether_primitives_amd import _lib, Scale                              # noqa: E402
from aether_primitives_amd.chan import PHASE_FRAME as FR, PHASE_STREAM as ST   # noqa: E402

pytestmark = pytest.mark.gpu

TOL_DB = -120.0                                   # tests/test_gpu_fft.py:20
FAR = 2 ** 40 + 3
GUARD = 16                                        # samples: keeps a 16-byte aligned buffer 16-byte aligned

# (M, P, D, (a, b): frames = a T + b, phase)
SHAPES = [
    (4, 1, 4, (0, 5), FR),                        # degenerate: today's framing
    (8, 3, 8, (2, 3), FR),                        # odd P, ring kernel across two tile edges
    (64, 4, 64, (0, 37), FR),
    (5, 2, 5, (0, 11), FR),                       # odd M: no 16-byte pairing
    (6, 2, 6, (0, 7), FR),
    (16, 2, 4, (1, 5), ST),
    (8, 1, 3, (0, 17), ST),                       # hop not dividing M: rot cycles
    (8, 2, 1, (0, 19), ST),
    (100, 4, 50, (0, 33), ST),                    # non-power-of-two route
    (2048, 8, 2048, (0, 64), FR),
    (1024, 16, 256, (0, 64), ST),
    (8, 64, 8, (0, 9), FR),                       # P = 64: the general kernel with hop == M
    (32, 64, 16, (0, 7), ST),
    # what the two kernels' own geometry adds
    (512, 8, 512, (1, 5), FR),                    # ring, one lane row per workgroup, across a tile edge, last tile ragged
    (1030, 2, 1030, (2, 1), FR),                  # ring, three column blocks, the last one partly filled
    (1025, 3, 1025, (1, 2), FR),                  # ring, odd M above one column block
    (64, 7, 64, (1, 3), FR),                      # ring, P = 7: rounds of 7 steps against a tile of 128
    (2048, 16, 2048, (0, 5), FR),                 # P > 8 with hop == M: the general kernel, two frames per workgroup
    (5000, 2, 2500, (0, 3), ST),                  # general kernel, two column chunks per frame
    (48, 3, 48, (0, 5), ST),                      # STREAM with hop == M: rot is identically 0
]
IDS = [f"M{m}-P{p}-D{d}-{a}T+{b}-{'S' if ph else 'F'}" for m, p, d, (a, b), ph in SHAPES]


def proto_of(M, P, seed=0):
    """a prototype without structure: every tap distinct, both signs"""
    rng = np.random.default_rng(1000 * M + P + seed)
    return rng.standard_normal(M * P).astype(np.float32)


@functools.lru_cache(maxsize=None)
def chan_of(ctx, M, P, D, phase):
    return ap.Channelizer(ctx, proto_of(M, P), M, D, phase)


def case(ctx, shape):
    M, P, D, (a, b), phase = shape
    ch = chan_of(ctx, M, P, D, phase)
    frames = a * ch.tile + b
    x = rand_c64(M * 7 + P * 3 + D, frames * D)
    hist = rand_c64(M + P + D + 99, M * P - D)
    return ch, frames, x, hist


def guarded(ctx, n, off=0):
    """a device vector of n samples `off` samples into a buffer with sentinels on both sides"""
    big = ctx.vec(np.full(n + 2 * GUARD + off, -7.5 + 3.25j, np.complex64))
    return big, big.slice(GUARD + off, GUARD + off + n)


def guards_intact(big, n, off=0):
    h = big.to_host()
    return bool((h[:GUARD + off] == np.complex64(-7.5 + 3.25j)).all() and (h[GUARD + off + n:] == np.complex64(-7.5 + 3.25j)).all())


def at_offset(ctx, x, off):
    big = ctx.vec(np.concatenate([np.zeros(off, np.complex64), x]))
    return big.slice(off, off + x.size)


def evm_db(got, want):
    err = np.sum(np.abs(got.astype(np.complex128) - want) ** 2)
    return 10 * np.log10(max(err, 1e-300) / np.sum(np.abs(want) ** 2))


# ---- the fold, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fold_is_the_definition_bit_for_bit(ctx, shape):
    M, P, D, _, phase = shape
    ch, frames, x, hist = case(ctx, shape)
    assert ch.channels == M and ch.ntaps == M * P and ch.hop == D and ch.phase == phase and ch.frames(x.size) == frames
    w = proto_of(M, P)
    dh = ctx.vec(hist) if hist.size else None
    for use_hist in (False, True):
        for first in (0, 1, FAR):
            want = chan_truth.fold(w, M, D, x, hist if use_hist else None, phase, first)
            for in_off, out_off in ((0, 0), (1, 0), (0, 1), (1, 1)):
                xin = at_offset(ctx, x, in_off)
                big, out = guarded(ctx, frames * M, out_off)
                ch.fold(xin, dh if use_hist else None, first, out)
                what = (use_hist, first, in_off, out_off)
                assert bits_equal(out.to_host(), want), what
                assert guards_intact(big, frames * M, out_off), what


def test_fold_of_special_values(ctx):
    """NaN, +-Inf and -0.0 in the stream and in the history; NaN payloads excluded as in tests/test_gpu_vecops.py"""
    for shape in ((8, 3, 8, (0, 21), FR), (5, 2, 5, (0, 11), FR), (16, 2, 4, (0, 37), ST)):
        M, P, D, _, phase = shape
        ch, frames, x, hist = case(ctx, shape)
        x, hist = x.copy(), hist.copy()
        specials = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], np.float32)
        xv, hv = x.view(np.float32), hist.view(np.float32)
        for k, v in enumerate(specials):
            xv[3 + 7 * k] = v
            xv[x.size + 2 * k] = specials[4 - k]
            hv[(1 + 3 * k) % hv.size] = v
        want = chan_truth.fold(proto_of(M, P), M, D, x, hist, phase, 5)
        got = ch.fold(ctx.vec(x), ctx.vec(hist), 5).to_host()
        assert np.isnan(want.view(np.float32)).any() and np.isinf(want.view(np.float32)).any(), shape
        assert chan_truth.same_bits(got, want), shape
    # -0.0 survives a positive tap and flips under a negative one
    ch = ap.Channelizer(ctx, np.array([2.0, -2.0, 2.0, -2.0], np.float32), 4)
    got = ch.fold(ctx.vec(np.array([complex(-0.0, 0.0)] * 4, np.complex64))).to_host().view(np.uint32)
    assert got.tolist() == [0x80000000, 0, 0, 0x80000000, 0x80000000, 0, 0, 0x80000000]


# ---- w = 1, P = 1, D = M is aeth_fft_exec ----------------------------------------------------------------------------
@pytest.mark.parametrize("M", (4, 100, 2048))
def test_rectangular_disjoint_frames_are_fft_exec(ctx, M):
    frames = 9
    x = rand_c64(M, frames * M)
    ch = ap.Channelizer(ctx, ap.chan.prototype("rect", M, 1), M)
    f = ap.HipFft(ctx, M)
    assert ch.route == f.route
    for sign in (ap.SIGN_REF_FWD, ap.SIGN_REF_BWD):
        for s in (Scale.NONE, Scale.SN):
            want = f.exec(ctx.vec(x), ctx.empty(x.size), sign, s).to_host()
            assert bits_equal(ch.exec(ctx.vec(x), sign=sign, s=s).to_host(), want), (sign, s)


# ---- exec = fold + aeth_fft_exec, exec_levels = fold + aeth_fft_exec_levels ---------------------------------------------
FUSED = [s for s in SHAPES if (s[0], s[1], s[2]) in ((8, 3, 8), (64, 4, 64), (100, 4, 50), (16, 2, 4), (5, 2, 5), (1024, 16, 256))]


@pytest.mark.parametrize("shape", FUSED, ids=[IDS[SHAPES.index(s)] for s in FUSED])
def test_exec_and_levels_are_fold_then_the_plan(ctx, shape):
    M, P, D, _, phase = shape
    ch, frames, x, hist = case(ctx, shape)
    xin, dh = ctx.vec(x), ctx.vec(hist)
    f = ap.HipFft(ctx, M)
    folded = ch.fold(xin, dh, 3)
    for sign in (ap.SIGN_REF_FWD, ap.SIGN_REF_BWD):
        for s in (Scale.NONE, Scale.SN, Scale.X(0.37)):
            want = f.exec(folded, ctx.empty(folded.n), sign, s).to_host()
            big, out = guarded(ctx, frames * M)
            ch.exec(xin, dh, 3, sign, s, out)
            assert bits_equal(out.to_host(), want) and guards_intact(big, frames * M), (sign, s)
            for kind in (ap.LEVEL_NORM, ap.LEVEL_DB, ap.LEVEL_POWER_DB):
                for mirror in (False, True):
                    lw = f.levels(folded, s, mirror, kind, sign=sign).to_host()
                    lg = ch.levels(xin, dh, 3, sign, s, mirror, kind).to_host()
                    assert chan_truth.same_bits(lg, lw), (sign, s, kind, mirror)
    assert bits_equal(folded.to_host(), chan_truth.fold(proto_of(M, P), M, D, x, hist, phase, 3))     # the input of both sides


# ---- against complex128 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exec_against_complex128(ctx, shape):
    M, P, D, _, phase = shape
    ch, frames, x, hist = case(ctx, shape)
    w = proto_of(M, P).astype(np.float64)
    # the definition in f64: exact products of the f32 taps and samples, summed in f64
    ext = np.concatenate([hist, x]).astype(np.complex128)
    fr = ext[np.arange(frames)[:, None] * D + np.arange(M * P)[None, :]] * w[None, :]
    u = fr.reshape(frames, P, M).sum(axis=1)
    for m, rot in enumerate(chan_truth.rots(M, D, frames, phase, 2)):
        u[m] = np.roll(u[m], rot)
    xin, dh = ctx.vec(x), (ctx.vec(hist) if hist.size else None)
    for sign in (ap.SIGN_REF_FWD, ap.SIGN_REF_BWD):
        for s in (Scale.NONE, Scale.SN):
            want = chan_truth.transform(u, M, sign, s.factor(M))
            got = ch.exec(xin, dh, 2, sign, s).to_host()
            db = evm_db(got, want)
            print(f"{IDS[SHAPES.index(shape)]} sign {sign:+d} {s}: EVM {db:.1f} dB")
            assert db <= TOL_DB, (sign, s, db)


# ---- chunks of a stream concatenate ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] <= 1030], ids=[i for s, i in zip(SHAPES, IDS) if s[0] <= 1030])
def test_two_calls_with_history_equal_one(ctx, shape):
    M, P, D, _, _ = shape
    L = M * P
    for phase in (FR, ST):
        ch = chan_of(ctx, M, P, D, phase)
        k = -(-(L - D) // D)                                          # frames that cover the history of the second call
        frames, F1 = case(ctx, shape)[1] + k, k + 1
        assert 0 < F1 < frames and F1 * D >= L - D
        x = rand_c64(L + D + 5, frames * D)
        xin = ctx.vec(x)
        for first in (0, FAR):
            whole_f = ch.fold(xin, None, first).to_host()
            whole_x = ch.exec(xin, None, first, s=Scale.SN).to_host()
            a, b = xin.slice(0, F1 * D), xin.slice(F1 * D, x.size)
            h = xin.slice(F1 * D - (L - D), F1 * D) if L > D else None
            parts_f = np.concatenate([ch.fold(a, None, first).to_host(), ch.fold(b, h, first + F1).to_host()])
            parts_x = np.concatenate([ch.exec(a, None, first, s=Scale.SN).to_host(), ch.exec(b, h, first + F1, s=Scale.SN).to_host()])
            assert bits_equal(parts_f, whole_f), (phase, first)
            assert bits_equal(parts_x, whole_x), (phase, first)
            assert bits_equal(whole_f, chan_truth.fold(proto_of(M, P), M, D, x, None, phase, first)), (phase, first)


# ---- reproducible, whatever the cache policy ---------------------------------------------------------------------------
REPRO = [s for s in SHAPES if (s[0], s[1], s[2]) in ((8, 3, 8), (2048, 8, 2048), (1024, 16, 256), (100, 4, 50), (5, 2, 5))]


def _repro_bytes(ctx, shape):
    ch, frames, x, hist = case(ctx, shape)
    xin, dh = ctx.vec(x), ctx.vec(hist)
    return (ch.fold(xin, dh, 7).to_host().tobytes() + ch.exec(xin, dh, 7, s=Scale.SN).to_host().tobytes()
            + ch.levels(xin, dh, 7, kind=ap.LEVEL_POWER_DB).to_host().tobytes())


def _child(outdir):
    ctx = ap.Context(0)
    for nt in ("0", "1"):
        os.environ["AETH_NT"] = nt
        for i, shape in enumerate(REPRO):
            with open(os.path.join(outdir, f"nt{nt}_{i}.bin"), "wb") as f:
                f.write(_repro_bytes(ctx, shape))
    chan_of.cache_clear()
    ctx.close()
    print("chan child ok")


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


# ---- refusals ------------------------------------------------------------------------------------------------------------
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


def test_create_refusals(ctx):
    w = np.ones(64, np.float32)
    with _refused(_lib.E_ARG, "64 taps", "5 channels"):
        ap.Channelizer(ctx, w, 5)
    with _refused(_lib.E_ARG, "0 channels"):
        ap.Channelizer(ctx, w, 0)
    with _refused(_lib.E_ARG, "hop 0"):
        ap.Channelizer(ctx, w, 16, 0)
    with _refused(_lib.E_ARG, "hop 17", "16"):
        ap.Channelizer(ctx, w, 16, 17)
    with _refused(_lib.E_ARG, "phase mode 2"):
        ap.Channelizer(ctx, w, 16, 16, 2)
    with _refused(_lib.E_UNSUPPORTED, "65 taps per channel", "64"):
        ap.Channelizer(ctx, np.ones(130, np.float32), 2)
    lib, h = _lib.load(), C.c_void_p(0x55)
    assert lib.aeth_chan_create(ctx.h, None, 64, 16, 16, 0, 0, C.byref(h)) == _lib.E_ARG and not h.value
    assert lib.aeth_chan_create(ctx.h, w.ctypes.data_as(C.c_void_p), 0, 16, 16, 0, 0, C.byref(h)) == _lib.E_ARG
    assert b"0 taps" in lib.aeth_last_error()
    assert lib.aeth_chan_create(ctx.h, w.ctypes.data_as(C.c_void_p), 64, 16, 16, 0, 0, None) == _lib.E_ARG


def _free_bytes():
    hip = _lib.load()                              # hipMemGetInfo of the runtime the library is bound to
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_a_refused_transform_length_leaves_nothing_allocated(ctx):
    M = 8388609                                    # (2^23, 2^24] without a route: tests/test_gpu_fft_routes.py
    w = np.ones(M, np.float32)
    with pytest.raises(ap.AetherError) as e:
        ap.HipFft(ctx, M)
    fft_msg, fft_code = e.value.message, e.value.code
    ctx.sync()
    free0 = _free_bytes()
    for _ in range(100):
        with _refused(fft_code, f"FFT length {M}:"):
            ap.Channelizer(ctx, w, M)
        assert _lib.load().aeth_last_error().decode() == fft_msg
    assert fft_code == _lib.E_UNSUPPORTED
    ctx.sync()
    assert _free_bytes() == free0
    ch = ap.Channelizer(ctx, w[:64], 16)           # the context plans on as before
    assert ch.fold(ctx.vec(np.ones(16, np.complex64))).to_host().tolist() == [1.0] * 16     # zero history: the newest row alone


def test_exec_refusals_launch_nothing(ctx):
    M, P, D = 16, 2, 4
    ch = chan_of(ctx, M, P, D, ST)
    lib = _lib.load()
    n = 5 * D
    x, hist = ctx.vec(rand_c64(1, n + 2)), ctx.vec(rand_c64(2, M * P - D))
    sentinel = np.full(5 * M + 2, 1.5 - 2.5j, np.complex64)
    out = ctx.vec(sentinel)
    lev = ap.DeviceF32(ctx, 5 * M + 2)
    X, H, O, LV = x.ptr, hist.ptr, out.ptr, lev.ptr
    p = C.c_void_p

    def fold(c=ch.h, h=H, i=X, nn=n, o=O, no=5 * M):
        return lib.aeth_chan_fold(c, p(h), p(i), nn, 0, p(o), no)

    def ex(c=ch.h, h=H, i=X, nn=n, o=O, no=5 * M, sign=1, kind=0):
        return lib.aeth_chan_exec(c, p(h), p(i), nn, 0, sign, kind, 0.0, p(o), no)

    def lv(c=ch.h, h=H, i=X, nn=n, o=LV, no=5 * M, sign=1, kind=0, lk=0):
        return lib.aeth_chan_exec_levels(c, p(h), p(i), nn, 0, sign, kind, 0.0, 0, lk, p(o), no)

    def err(rc, code, *words):
        msg = lib.aeth_last_error().decode()
        assert rc == code, (rc, msg)
        assert all(w in msg for w in words), msg

    for f in (fold, ex, lv):
        err(f(c=None), _lib.E_ARG, "chan", "null")
        err(f(i=None), _lib.E_ARG, "null")
        err(f(o=None), _lib.E_ARG, "null")
        err(f(nn=0, no=0), _lib.E_LEN, "0 input samples")
        err(f(nn=n + 1), _lib.E_LEN, f"{n + 1} input samples", "hop 4")
        err(f(no=5 * M - 1), _lib.E_LEN, f"{5 * M - 1} elements", "5 frames", "16 channels")
        err(f(no=5 * M + 1), _lib.E_LEN, f"{5 * M + 1} elements")
        err(f(i=X + 4), _lib.E_ALIGN, "8-byte aligned")
        err(f(h=H + 4), _lib.E_ALIGN, "8-byte aligned")
    err(fold(o=O + 4), _lib.E_ALIGN, "8-byte aligned")
    err(ex(o=O + 4), _lib.E_ALIGN, "8-byte aligned")
    err(lv(o=LV + 2), _lib.E_ALIGN, "4-byte aligned")
    # the output range must be clear of the input and of the history
    err(fold(o=X), _lib.E_ARG, "overlaps")
    err(ex(o=X + 8), _lib.E_ARG, "overlaps")
    err(fold(i=O + 8 * (5 * M - 1), o=O), _lib.E_ARG, "overlaps")
    err(fold(h=O + 8 * (5 * M - 1), o=O), _lib.E_ARG, "overlaps")
    err(lv(o=X), _lib.E_ARG, "overlaps")
    err(lv(h=LV), _lib.E_ARG, "overlaps")
    err(ex(sign=0), _lib.E_ARG, "sign")
    err(ex(kind=4), _lib.E_ARG, "scale kind 4")
    err(lv(sign=2), _lib.E_ARG, "sign")
    err(lv(kind=-1), _lib.E_ARG, "scale kind -1")
    err(lv(lk=3), _lib.E_ARG, "level kind 3")
    ctx.sync()
    assert bits_equal(out.to_host(), sentinel)                       # nothing was launched
    # and the same arguments, made right, run
    assert fold() == 0 and ex() == 0 and lv() == 0
    ctx.sync()
    assert lib.aeth_chan_tile(None) == 0 and lib.aeth_chan_channels(None) == 0 and lib.aeth_chan_route(None) == b""
    with pytest.raises(ap.LengthMismatch):
        ch.fold(x.slice(0, n), ctx.vec(rand_c64(3, 5)))               # the Python mirror checks the history's length


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--child":
    _child(sys.argv[2])
