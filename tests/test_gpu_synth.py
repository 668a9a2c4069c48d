"""GPU: the polyphase synthesis filter bank (csrc/aeth_synth.hip, aeth_synth_*) against a numpy restatement of its
definition (tests/synth_truth.py): the overlap-add bit for bit, transform + overlap-add against complex128 under the
bound of aeth_fft_exec (-120 dB, tests/test_gpu_fft.py), analysis followed by synthesis against the stream.

Launch geometry (T = aeth_synth_tile, K = ceil(L / D) frames per output sample).  D == M runs aeth_chan_fold's kernels
on the row-reversed prototype (T as in tests/test_gpu_chan.py).  D < M dividing L with K <= 8 runs the accumulator ring:
a lane owns one output offset of every hop (8-byte accesses: odd D or M, or a pointer that is only 8-byte aligned) or
two, and walks a tile of T = max(16, 16 (K - 1) rounded up to a power of two) frames; a workgroup is 256 lanes,
min(256, offsets) of them along the offsets and the rest along the tiles.  Every other shape runs the general gather: a
workgroup makes T = 4096 / D whole hops (D <= 2048) or 4096 offsets of one hop.  The shapes below are the smallest at
which each mechanism can break."""
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
import synth_truth                                                         # noqa: E402
from helpers import bits_equal, rand_c64                                   # noqa: E402

import aether_primitives_amd as ap                                         # noqa: E402
from aether_primitives_amd import _lib, Scale                              # noqa: E402
from aether_primitives_amd.chan import PHASE_FRAME as FR, PHASE_STREAM as ST   # noqa: E402

pytestmark = pytest.mark.gpu

TOL_DB = -120.0                                   # tests/test_gpu_fft.py:20
ROUND_TRIP_DB = -114.0                            # two stages of -120 dB whose errors add in amplitude at worst
FAR = 2 ** 40 + 3
GUARD = 16                                        # samples: keeps a 16-byte aligned buffer 16-byte aligned

# (M, P, D, (a, b): frames = a T + b, phase)
FOLD = [
    (4, 1, 4, (0, 5), FR),                        # K = 1: no history at all
    (8, 3, 8, (2, 3), FR),
    (5, 2, 5, (0, 11), FR),                       # odd M: no 16-byte pairing
    (64, 7, 64, (1, 3), FR),
    (2048, 16, 2048, (0, 5), FR),                 # P > 8: the fold's general kernel
    (48, 3, 48, (0, 5), ST),                      # STREAM with hop == M: rot is identically 0
]
RING = [
    (8, 1, 4, (2, 3), FR),                        # K = 2, two tile edges, last tile ragged
    (16, 1, 4, (2, 5), ST),                       # K = 4
    (16, 2, 4, (2, 7), ST),                       # K = 8: the same v element feeds two taps
    (6, 1, 3, (0, 9), FR),                        # odd D: no pairing
    (100, 1, 50, (1, 3), ST),                     # non-power-of-two route
    (1030, 1, 515, (1, 2), FR),                   # odd D over several lane blocks
    (2048, 1, 256, (0, 21), ST),                  # K = 8
    (5000, 2, 2500, (0, 7), ST),                  # K = 4, ten lane blocks (five when paired)
    (1024, 2, 512, (1, 3), ST),
]
GEN = [
    (8, 1, 3, (1, 3), ST),                        # D does not divide L: 2 or 3 terms, rot cycles
    (8, 2, 1, (1, 5), ST),                        # K = 16
    (1024, 16, 256, (1, 5), ST),                  # K = 64
    (32, 64, 16, (1, 7), ST),                     # K = 128
    (12, 1, 5, (1, 2), FR),
]
SHAPES = FOLD + RING + GEN
IDS = [f"M{m}-P{p}-D{d}-{a}T+{b}-{'S' if ph else 'F'}" for m, p, d, (a, b), ph in SHAPES]
ONE_PER_ROUTE = [FOLD[1], RING[2], GEN[0]]


def ids_of(shapes):
    return [IDS[SHAPES.index(s)] for s in shapes]


def proto_of(M, P, seed=0):
    """a prototype without structure: every tap distinct, both signs"""
    rng = np.random.default_rng(1000 * M + P + seed)
    return rng.standard_normal(M * P).astype(np.float32)


@functools.lru_cache(maxsize=None)
def synth_of(ctx, M, P, D, phase):
    return ap.Synthesizer(ctx, proto_of(M, P), M, D, phase)


def case(ctx, shape):
    M, P, D, (a, b), phase = shape
    sy = synth_of(ctx, M, P, D, phase)
    frames = a * sy.tile + b
    v = rand_c64(M * 7 + P * 3 + D, frames * M)
    hist = rand_c64(M + P + D + 99, sy.history * M)
    return sy, frames, v, hist


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
    err = np.sum(np.abs(np.asarray(got).astype(np.complex128) - want) ** 2)
    return 10 * np.log10(max(err, 1e-300) / np.sum(np.abs(want) ** 2))


# ---- the overlap-add, bit for bit --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_unfold_is_the_definition_bit_for_bit(ctx, shape):
    M, P, D, _, phase = shape
    sy, frames, v, hist = case(ctx, shape)
    K = synth_truth.depth(M * P, D)
    assert sy.channels == M and sy.ntaps == M * P and sy.hop == D and sy.phase == phase and sy.history == K - 1
    assert sy.samples(v.size) == frames * D
    g = proto_of(M, P)
    dh = ctx.vec(hist) if hist.size else None
    for use_hist in (False, True):
        for first in (0, 1, FAR):
            want = synth_truth.unfold(g, M, D, v, hist if use_hist and hist.size else None, phase, first)
            for in_off, out_off in ((0, 0), (1, 0), (0, 1), (1, 1)):
                vin = at_offset(ctx, v, in_off)
                big, out = guarded(ctx, frames * D, out_off)
                sy.unfold(vin, dh if use_hist else None, first, out)
                what = (use_hist, first, in_off, out_off)
                assert bits_equal(out.to_host(), want), what
                assert guards_intact(big, frames * D, out_off), what
    if dh is not None:                                                # a history that is only 8-byte aligned
        want = synth_truth.unfold(g, M, D, v, hist, phase, 1)
        assert bits_equal(sy.unfold(ctx.vec(v), at_offset(ctx, hist, 1), 1).to_host(), want)


def test_unfold_of_special_values(ctx):
    """NaN, +-Inf and -0.0 in the frames and in the history; NaN payloads excluded as in tests/test_gpu_vecops.py"""
    for shape in ONE_PER_ROUTE:
        M, P, D, _, phase = shape
        sy, frames, v, hist = case(ctx, shape)
        v, hist = v.copy(), hist.copy()
        specials = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0], np.float32)
        vv, hv = v.view(np.float32), hist.view(np.float32)
        for k, s in enumerate(specials):
            vv[3 + 7 * k] = s
            vv[v.size + 2 * k] = specials[4 - k]
            hv[(1 + 3 * k) % hv.size] = s
        want = synth_truth.unfold(proto_of(M, P), M, D, v, hist, phase, 5)
        got = sy.unfold(ctx.vec(v), ctx.vec(hist), 5).to_host()
        assert np.isnan(want.view(np.float32)).any() and np.isinf(want.view(np.float32)).any(), shape
        assert synth_truth.same_bits(got, want), shape
        # a history of zeros is multiplied like any other frame: an infinite tap makes NaN of it
        g = proto_of(M, P).copy()
        g[-1] = np.inf
        sy2 = ap.Synthesizer(ctx, g, M, D, phase)
        want = synth_truth.unfold(g, M, D, v, None, phase, 5)
        assert synth_truth.same_bits(sy2.unfold(ctx.vec(v), None, 5).to_host(), want), shape
    # -0.0 survives a positive tap and flips under a negative one
    sy = ap.Synthesizer(ctx, np.array([2.0, -2.0, 2.0, -2.0], np.float32), 4)
    got = sy.unfold(ctx.vec(np.array([complex(-0.0, 0.0)] * 4, np.complex64))).to_host().view(np.uint32)
    assert got.tolist() == [0x80000000, 0, 0, 0x80000000, 0x80000000, 0, 0, 0x80000000]
    want = synth_truth.unfold(np.array([2.0, -2.0, 2.0, -2.0], np.float32), 4, 4, np.array([complex(-0.0, 0.0)] * 4, np.complex64))
    assert want.view(np.uint32).tolist() == got.tolist()


# ---- D == M is the fold of the reversed rows --------------------------------------------------------------------------
@pytest.mark.parametrize("M,P", ((8, 3), (5, 2), (64, 7), (2048, 16)))
def test_hop_equal_channels_is_the_fold_of_the_reversed_rows(ctx, M, P):
    shape = next(s for s in FOLD if s[0] == M and s[1] == P)
    sy, frames, v, hist = case(ctx, shape)
    g = proto_of(M, P)
    ch = ap.Channelizer(ctx, g.reshape(P, M)[::-1].copy().reshape(-1), M)
    assert ch.tile == sy.tile
    vin, dh = ctx.vec(v), ctx.vec(hist)
    for h in (None, dh):
        assert bits_equal(sy.unfold(vin, h, 2).to_host(), ch.fold(vin, h, 2).to_host())


# ---- exec = aeth_fft_exec + unfold -------------------------------------------------------------------------------------
FUSED = ONE_PER_ROUTE + [RING[4]]


@pytest.mark.parametrize("shape", FUSED, ids=ids_of(FUSED))
def test_exec_is_the_plan_then_unfold(ctx, shape):
    M, P, D, _, phase = shape
    sy, frames, v, hist = case(ctx, shape)
    f = ap.HipFft(ctx, M)
    assert sy.route == f.route
    spec, dh = ctx.vec(v), ctx.vec(hist)
    for sign in (ap.SIGN_REF_FWD, ap.SIGN_REF_BWD):
        for s in (Scale.NONE, Scale.SN, Scale.X(0.37)):
            tv = f.exec(spec, ctx.empty(spec.n), sign, s)
            th = f.exec(dh, ctx.empty(dh.n), sign, s)
            for h, t in ((None, None), (dh, th)):
                want = sy.unfold(tv, t, 3).to_host()
                big, out = guarded(ctx, frames * D)
                sy.exec(spec, h, 3, sign, s, out)
                assert bits_equal(out.to_host(), want) and guards_intact(big, frames * D), (sign, s, h is None)
    assert bits_equal(sy.unfold(tv, th, 3).to_host(), synth_truth.unfold(proto_of(M, P), M, D, tv.to_host(), th.to_host(), phase, 3))


# ---- against complex128 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_exec_against_complex128(ctx, shape):
    M, P, D, _, phase = shape
    sy, frames, v, hist = case(ctx, shape)
    g = proto_of(M, P)
    spec, dh = ctx.vec(v), (ctx.vec(hist) if hist.size else None)
    for sign in (ap.SIGN_REF_FWD, ap.SIGN_REF_BWD):
        for s in (Scale.NONE, Scale.SN):
            tv = chan_truth.transform(v, M, sign, s.factor(M))
            th = chan_truth.transform(hist, M, sign, s.factor(M)) if hist.size else None
            want = synth_truth.unfold_f64(g, M, D, tv, th, phase, 2)
            got = sy.exec(spec, dh, 2, sign, s).to_host()
            db = evm_db(got, want)
            print(f"{IDS[SHAPES.index(shape)]} sign {sign:+d} {s}: EVM {db:.1f} dB")
            assert db <= TOL_DB, (sign, s, db)


# ---- chunks of a stream concatenate ------------------------------------------------------------------------------------
SMALL = [s for s in SHAPES if s[0] <= 1030]


@pytest.mark.parametrize("shape", SMALL, ids=ids_of(SMALL))
def test_two_calls_with_history_equal_one(ctx, shape):
    M, P, D, _, _ = shape
    for phase in (FR, ST):
        sy = synth_of(ctx, M, P, D, phase)
        K = sy.history + 1
        frames, F1 = case(ctx, shape)[1] + K, K
        assert 0 < F1 < frames and F1 >= K - 1
        v = rand_c64(M * P + D + 5, frames * M)
        vin = ctx.vec(v)
        for first in (0, FAR):
            whole_u = sy.unfold(vin, None, first).to_host()
            whole_x = sy.exec(vin, None, first, s=Scale.SN).to_host()
            a, b = vin.slice(0, F1 * M), vin.slice(F1 * M, v.size)
            h = vin.slice((F1 - (K - 1)) * M, F1 * M) if K > 1 else None
            parts_u = np.concatenate([sy.unfold(a, None, first).to_host(), sy.unfold(b, h, first + F1).to_host()])
            parts_x = np.concatenate([sy.exec(a, None, first, s=Scale.SN).to_host(), sy.exec(b, h, first + F1, s=Scale.SN).to_host()])
            assert bits_equal(parts_u, whole_u), (phase, first)
            assert bits_equal(parts_x, whole_x), (phase, first)
            assert bits_equal(whole_u, synth_truth.unfold(proto_of(M, P), M, D, v, None, phase, first)), (phase, first)


# ---- analysis, then synthesis with the dual window, is the stream ---------------------------------------------------------
ROUND = [(8, 4, "hann"), (16, 4, "hann"), (100, 50, "hann"), (2048, 512, "hann"), (8, 3, "hamming"), (64, 64, "rect")]


@pytest.mark.parametrize("M,D,kind", ROUND, ids=[f"M{m}-D{d}-{k}" for m, d, k in ROUND])
def test_round_trip_returns_the_stream(ctx, M, D, kind):
    w = ap.chan.prototype(kind, M, 1)
    g = ap.synth.dual_window(w, D)
    frames = 37 if M <= 100 else 9
    s = rand_c64(M + D, frames * D)
    delay = M - D
    for phase in (FR, ST):
        ch = ap.Channelizer(ctx, w, M, D, phase)
        sy = ap.Synthesizer(ctx, g, M, D, phase)
        for first in (0, FAR):
            spec = ch.exec(ctx.vec(s), None, first, ap.SIGN_REF_BWD, Scale.NONE)
            out = sy.exec(spec, None, first, ap.SIGN_REF_FWD, Scale.N).to_host()
            assert out.size == s.size
            db = evm_db(out[delay:], s[:s.size - delay].astype(np.complex128))
            print(f"M{M}-D{D}-{kind} phase {phase} first {first}: round trip {db:.1f} dB")
            assert db <= ROUND_TRIP_DB, (phase, first, db)


# ---- reproducible, whatever the cache policy ---------------------------------------------------------------------------
REPRO = ONE_PER_ROUTE


def _repro_bytes(ctx, shape):
    sy, frames, v, hist = case(ctx, shape)
    vin, dh = ctx.vec(v), ctx.vec(hist)
    return sy.unfold(vin, dh, 7).to_host().tobytes() + sy.exec(vin, dh, 7, s=Scale.SN).to_host().tobytes()


def _child(outdir):
    ctx = ap.Context(0)
    for nt in ("0", "1"):
        os.environ["AETH_NT"] = nt
        for i, shape in enumerate(REPRO):
            with open(os.path.join(outdir, f"nt{nt}_{i}.bin"), "wb") as f:
                f.write(_repro_bytes(ctx, shape))
    synth_of.cache_clear()
    ctx.close()
    print("synth child ok")


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
        ap.Synthesizer(ctx, w, 5)
    with _refused(_lib.E_ARG, "0 channels"):
        ap.Synthesizer(ctx, w, 0)
    with _refused(_lib.E_ARG, "hop 0"):
        ap.Synthesizer(ctx, w, 16, 0)
    with _refused(_lib.E_ARG, "hop 17", "16"):
        ap.Synthesizer(ctx, w, 16, 17)
    with _refused(_lib.E_ARG, "phase mode 2"):
        ap.Synthesizer(ctx, w, 16, 16, 2)
    with _refused(_lib.E_UNSUPPORTED, "65 taps per channel", "64"):
        ap.Synthesizer(ctx, np.ones(130, np.float32), 2)
    with _refused(_lib.E_UNSUPPORTED, "512 taps", "hop 1", "512 frames", "256"):
        ap.Synthesizer(ctx, np.ones(512, np.float32), 512, 1)
    assert ap.Synthesizer(ctx, np.ones(512, np.float32), 512, 2).history == 255      # K = 256 is served
    lib, h = _lib.load(), C.c_void_p(0x55)
    assert lib.aeth_synth_create(ctx.h, None, 64, 16, 16, 0, 0, C.byref(h)) == _lib.E_ARG and not h.value
    assert lib.aeth_synth_create(ctx.h, w.ctypes.data_as(C.c_void_p), 0, 16, 16, 0, 0, C.byref(h)) == _lib.E_ARG
    assert b"0 taps" in lib.aeth_last_error()
    assert lib.aeth_synth_create(ctx.h, w.ctypes.data_as(C.c_void_p), 64, 16, 16, 0, 0, None) == _lib.E_ARG


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
            ap.Synthesizer(ctx, w, M)
        assert _lib.load().aeth_last_error().decode() == fft_msg
    assert fft_code == _lib.E_UNSUPPORTED
    ctx.sync()
    assert _free_bytes() == free0
    sy = ap.Synthesizer(ctx, w[:64], 16)           # the context plans on as before
    assert sy.unfold(ctx.vec(np.ones(16, np.complex64))).to_host().tolist() == [1.0] * 16     # zero history: +0 is added


def test_unfold_and_exec_refusals_launch_nothing(ctx):
    M, P, D = 16, 2, 4
    sy = synth_of(ctx, M, P, D, ST)
    lib = _lib.load()
    n = 5 * M
    v, hist = ctx.vec(rand_c64(1, n + 2)), ctx.vec(rand_c64(2, sy.history * M))
    sentinel = np.full(5 * D + 2, 1.5 - 2.5j, np.complex64)
    out = ctx.vec(sentinel)
    V, H, O = v.ptr, hist.ptr, out.ptr
    p = C.c_void_p

    def unfold(c=sy.h, h=H, i=V, nn=n, o=O, no=5 * D):
        return lib.aeth_synth_unfold(c, p(h), p(i), nn, 0, p(o), no)

    def ex(c=sy.h, h=H, i=V, nn=n, o=O, no=5 * D, sign=1, kind=0):
        return lib.aeth_synth_exec(c, p(h), p(i), nn, 0, sign, kind, 0.0, p(o), no)

    def err(rc, code, *words):
        msg = lib.aeth_last_error().decode()
        assert rc == code, (rc, msg)
        assert all(w in msg for w in words), msg

    for f in (unfold, ex):
        err(f(c=None), _lib.E_ARG, "synth", "null")
        err(f(i=None), _lib.E_ARG, "null")
        err(f(o=None), _lib.E_ARG, "null")
        err(f(nn=0, no=0), _lib.E_LEN, "0 input samples")
        err(f(nn=n + 1), _lib.E_LEN, f"{n + 1} input samples", "16 channels")
        err(f(no=5 * D - 1), _lib.E_LEN, f"{5 * D - 1} elements", "5 frames", "hop 4")
        err(f(no=5 * D + 1), _lib.E_LEN, f"{5 * D + 1} elements")
        err(f(i=V + 4), _lib.E_ALIGN, "8-byte aligned")
        err(f(h=H + 4), _lib.E_ALIGN, "8-byte aligned")
        err(f(o=O + 4), _lib.E_ALIGN, "8-byte aligned")
        # the output range must be clear of the input and of the history
        err(f(o=V), _lib.E_ARG, "overlaps")
        err(f(o=V + 8 * (n - 1)), _lib.E_ARG, "overlaps")
        err(f(i=O + 8 * (5 * D - 1), o=O), _lib.E_ARG, "overlaps")
        err(f(h=O + 8 * (5 * D - 1), o=O), _lib.E_ARG, "overlaps")
        err(f(o=H + 8 * (sy.history * M - 1)), _lib.E_ARG, "overlaps")
    err(ex(sign=0), _lib.E_ARG, "sign")
    err(ex(kind=4), _lib.E_ARG, "scale kind 4")
    err(ex(kind=-1), _lib.E_ARG, "scale kind -1")
    ctx.sync()
    assert bits_equal(out.to_host(), sentinel)                       # nothing was launched
    # and the same arguments, made right, run
    assert unfold() == 0 and ex() == 0
    ctx.sync()
    assert lib.aeth_synth_tile(None) == 0 and lib.aeth_synth_history(None) == 0 and lib.aeth_synth_route(None) == b""
    with pytest.raises(ap.LengthMismatch):
        sy.unfold(v.slice(0, n), ctx.vec(rand_c64(3, 5)))             # the Python mirror checks the history's length


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--child":
    _child(sys.argv[2])
