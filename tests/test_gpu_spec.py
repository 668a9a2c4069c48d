"""GPU: averaged spectra (include/aether_hip.h, "averaged spectra").  aeth_vec_frame_sums byte for byte against the numpy
restatement of its definition (tests/spec_truth.py); aeth_chan_exec_sums, on both routes, byte for byte against
aeth_chan_exec followed by aeth_vec_frame_sums; slices, streams cut at a row, both cache policies, special values,
aeth_vec_sum_levels and every refusal.

Run as a script with --child DIR it writes the bytes of the reproducibility cases under both AETH_NT settings and a small
slice of the general route (the library reads those only in a process started with AETH_TUNING=1)."""
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

import spec_truth                                                          # noqa: E402
from helpers import rand_c64                                               # noqa: E402

import aether_primitives_amd as ap                                         # noqa: E402
from aether_primitives_amd import _lib, Scale                              # noqa: E402
from aether_primitives_amd.chan import PHASE_FRAME as FR, PHASE_STREAM as ST   # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 6                                         # doubles on either side of a plane
SENT = -12345.678
FAR = 2 ** 40 + 3
BURSTS = (0, 9, 10, 17, 18)                       # frames 9, 10 (17, 18) share a chunk of 4 (16) that frame 0 is not in
same = spec_truth.same_plane
P = C.c_void_p


class Plane:
    """n doubles between sentinels"""

    def __init__(self, ctx, n):
        self.n = n
        self.big = ap.DeviceF64(ctx, n + 2 * GUARD)
        ctx.upload(self.big.ptr, np.full(n + 2 * GUARD, SENT))
        self.dev = self.big.slice(GUARD, GUARD + n)

    def host(self):
        h = self.big.to_host()
        assert (h[:GUARD] == SENT).all() and (h[GUARD + self.n:] == SENT).all(), "a guard cell was written"
        return h[GUARD:GUARD + self.n]

    def untouched(self):
        return bool((self.big.to_host() == SENT).all())


def at_offset(ctx, x, off):
    big = ctx.vec(np.concatenate([np.zeros(off, np.complex64), x]))
    return big.slice(off, off + x.size)


def rows(F, block):
    return len(spec_truth.rows_of(F, block))


def frame_sums(ctx, vec, length, block, chunk, want=("sum", "max")):
    """aeth_vec_frame_sums into guarded planes -> host arrays (None for a plane not asked for)"""
    n_out = rows(vec.n // length, block) * length
    s = Plane(ctx, n_out) if "sum" in want else None
    m = Plane(ctx, n_out) if "max" in want else None
    _lib.check(_lib.load().aeth_vec_frame_sums(ctx.h, vec._p(), vec.n, length, block, chunk, s.dev._p() if s else None,
                                               m.dev._p() if m else None, n_out))
    return (s.host() if s else None), (m.host() if m else None)


# ---- the reduction alone ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", (1, 4, 16))
@pytest.mark.parametrize("length", (1, 5, 64, 257, 513, 1024))
def test_frame_sums_are_the_definition_byte_for_byte(ctx, length, chunk):
    Cc = chunk
    for F in sorted({1, Cc - 1, Cc, Cc + 1, 3 * Cc + 1} - {0}):
        x = spec_truth.burst_then_noise(1000 * length + 10 * Cc + F, F, length, BURSTS)
        for off in (0, 1):                                        # base on a 16- and on an 8-byte boundary
            v = at_offset(ctx, x, 2 * off + off)                  # 0 or 3 samples in
            assert v.ptr % 16 == (8 if off else 0)
            for block in (0, 1, Cc, Cc + 3):
                ws, wm = spec_truth.frame_sums(x, length, block, Cc)
                gs, gm = frame_sums(ctx, v, length, block, Cc)
                assert same(gs, ws), (F, off, block, "sum")
                assert same(gm, wm), (F, off, block, "max")
            # each plane alone: the same bytes
            ws, wm = spec_truth.frame_sums(x, length, Cc + 3, Cc)
            assert same(frame_sums(ctx, v, length, Cc + 3, Cc, ("sum",))[0], ws), (F, off, "sum alone")
            assert same(frame_sums(ctx, v, length, Cc + 3, Cc, ("max",))[1], wm), (F, off, "max alone")


def test_the_order_shows_on_the_device_too(ctx):
    x = spec_truth.burst_then_noise(3, 64, 32, BURSTS)
    a, _ = frame_sums(ctx, ctx.vec(x), 32, 0, 64)
    b, _ = frame_sums(ctx, ctx.vec(x), 32, 0, 4)
    assert (a.view(np.uint64) != b.view(np.uint64)).any()


def test_special_values(ctx):
    F, L, Cc = 13, 10, 4
    x = rand_c64(5, F * L).reshape(F, L)
    x[:, 0] = complex(np.nan, 1.0)                                # a column of NaNs
    x[3, 1] = complex(1.0, np.nan)                                # one NaN
    x[5, 2] = complex(np.inf, 0.0)
    x[6, 3], x[7, 3] = complex(-np.inf, 1.0), complex(np.nan, np.nan)
    x[:, 4] = complex(0.0, -0.0)
    x[:, 5] = complex(1e-45, -1e-45)                              # denormals: q = 2e-90 in f64
    x[2, 6], x[9, 6] = complex(3e19, -3e19), complex(-3e19, 1.0)  # q near 1e39: fine in f64
    x[:, 7] = complex(-0.0, 0.0)
    x[0, 7] = complex(np.nan, 0.0)                                # NaN in the first frame of a chunk
    x[12, 8] = complex(0.0, np.nan)                               # ... and in the last, short chunk
    x = x.reshape(-1)
    for block in (0, 5):
        ws, wm = spec_truth.frame_sums(x, L, block, Cc)
        gs, gm = frame_sums(ctx, ctx.vec(x), L, block, Cc)
        assert same(gs, ws) and same(gm, wm), block
    gs, gm = frame_sums(ctx, ctx.vec(x), L, 0, Cc)
    assert np.isnan(gs[0]) and gm[0] == -np.inf
    assert np.isnan(gs[1]) and np.isfinite(gm[1])
    assert gs[2] == np.inf and gm[2] == np.inf
    assert np.isnan(gs[3]) and gm[3] == np.inf
    assert gs[4] == 0.0 and gm[4] == 0.0 and gs[5] > 0.0
    assert np.isfinite(gs[6]) and gs[6] > 1e39


# ---- the filter bank: both routes against exec + frame_sums -----------------------------------------------------------
def proto_of(M, Pp, window):
    if window == "rand":
        return np.random.default_rng(1000 * M + Pp).standard_normal(M * Pp).astype(np.float32)
    return ap.chan.prototype(window, M, Pp)


@functools.lru_cache(maxsize=None)
def chan_of(ctx, M, Pp, D, phase, window):
    return ap.Channelizer(ctx, proto_of(M, Pp, window), M, D, phase)


def fused_expected(M, Pp, D, phase):
    return M in (512, 1024, 2048, 4096) and Pp == 1 and (phase == FR or D == M)


# (M, P, D, phase, window)
FUSED_SHAPES = [(M, 1, D, FR, "rect" if D == M else "hann") for M in (512, 1024, 2048, 4096) for D in (M, M // 2, M // 4, 1)]
FUSED_SHAPES += [(512, 1, 384, FR, "hann"), (1024, 1, 512, FR, "rect"), (1024, 1, 1024, FR, "hann"), (2048, 1, 2048, ST, "hann"),
                 (64, 1, 64, FR, "rect"), (64, 1, 32, FR, "hann"), (256, 1, 256, FR, "hann"), (256, 1, 128, FR, "rect")]
GENERAL_SHAPES = [(12, 1, 12, FR, "rand"), (600, 2, 300, FR, "rand"), (1024, 8, 256, ST, "rand"), (1536, 1, 768, FR, "hann"),
                  (1024, 1, 512, ST, "hann")]
SCALES = (Scale.NONE, Scale.SN, Scale.N, Scale.X(0.37))


def ident(s):
    return f"M{s[0]}-P{s[1]}-D{s[2]}-{'S' if s[3] else 'F'}-{s[4]}"


def reference(ctx, ch, x, hist, first, sign, s, mirror, block, want=("sum", "max")):
    """aeth_chan_exec, vec_mirror of every frame if asked, aeth_vec_frame_sums with the bank's chunk"""
    spec = ch.exec(x, hist, first, sign, s)
    if mirror:
        spec.vec_mirror_frames(ch.channels)
    return frame_sums(ctx, spec, ch.channels, block, ch.sums_chunk, want), spec


def sums(ctx, ch, x, hist, first, sign, s, mirror, block, general, want=("sum", "max")):
    F = x.n // ch.hop
    n_out = rows(F, block) * ch.channels
    sp = Plane(ctx, n_out) if "sum" in want else None
    mp = Plane(ctx, n_out) if "max" in want else None
    _lib.check(_lib.load().aeth_chan_exec_sums(ch.h, hist._p() if hist is not None else None, x._p(), x.n, first, sign, s.kind, s.x,
                                               1 if mirror else 0, block, 1 if general else 0, sp.dev._p() if sp else None,
                                               mp.dev._p() if mp else None, n_out))
    return (sp.host() if sp else None), (mp.host() if mp else None)


@pytest.mark.parametrize("shape", FUSED_SHAPES + GENERAL_SHAPES, ids=ident)
def test_chan_sums_are_exec_then_frame_sums_on_both_routes(ctx, shape):
    M, Pp, D, phase, window = shape
    ch = chan_of(ctx, *shape)
    Cc = ch.sums_chunk
    assert Cc >= 1 and ch.sums_fused == fused_expected(M, Pp, D, phase)
    first = FAR if phase == ST else 0
    H = M * Pp - D
    hist_host = rand_c64(M + D + 1, H) if H else None
    i = 0
    for F in ((2 * Cc + 1,) if D == 1 else (Cc - 1, Cc, Cc + 1, 2 * Cc + 3)):
        x_host = rand_c64(7 * M + D + F, F * D)
        for with_hist in (False, True):
            for block in (0, Cc + 3):
                # every sign, Scale kind, mirror setting and pointer parity comes round as i runs
                sign, s, mirror, off = (1, -1)[i % 2], SCALES[(i // 2) % 4], bool((i // 3) % 2), (i // 5) % 2
                i += 1
                x = at_offset(ctx, x_host, off)
                hist = ctx.vec(hist_host) if with_hist and H else None
                (ws, wm), spec = reference(ctx, ch, x, hist, first, sign, s, mirror, block)
                if i % 7 == 1:                                    # the reference itself against the restatement
                    ts, tm = spec_truth.frame_sums(spec.to_host(), M, block, Cc)
                    assert same(ws, ts) and same(wm, tm)
                for general in (True, False):
                    gs, gm = sums(ctx, ch, x, hist, first, sign, s, mirror, block, general)
                    what = (F, with_hist, block, sign, s.kind, mirror, off, "general" if general else "default")
                    assert same(gs, ws), what + ("sum",)
                    assert same(gm, wm), what + ("max",)
    # each plane alone, on both routes
    x, hist = ctx.vec(x_host), (ctx.vec(hist_host) if H else None)
    (ws, wm), _ = reference(ctx, ch, x, hist, first, 1, Scale.SN, True, Cc + 3)
    for general in (True, False):
        assert same(sums(ctx, ch, x, hist, first, 1, Scale.SN, True, Cc + 3, general, ("sum",))[0], ws)
        assert same(sums(ctx, ch, x, hist, first, 1, Scale.SN, True, Cc + 3, general, ("max",))[1], wm)


def test_python_surface(ctx):
    ch = chan_of(ctx, 1024, 1, 512, FR, "hann")
    x = ctx.vec(rand_c64(4, 40 * 512))
    s, m = ch.sums(x, s=Scale.SN, block=16)
    assert isinstance(s, ap.DeviceF64) and s.n == m.n == 3 * 1024
    s2, m2 = ch.sums(x, s=Scale.SN, block=16, general=True, want=("max",))
    assert s2 is None and same(m2.to_host(), m.to_host())
    spec = ch.exec(x, s=Scale.SN)
    fs, fm = ctx.frame_sums(spec, 1024, block=16, chunk=ch.sums_chunk)
    assert same(fs.to_host(), s.to_host()) and same(fm.to_host(), m.to_host())
    lv = ctx.sum_levels(s.slice(0, 1024), 16, ap.LEVEL_POWER_DB)
    assert isinstance(lv, ap.DeviceF32) and lv.n == 1024


# ---- slices of the general route ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((4096, 1, 1024, FR, "hann"), (4096, 64, 1, FR, "rand")), ids=ident)
def test_a_call_of_two_slices_is_the_definition(ctx, shape):
    """64 MiB of spectrum are 2048 frames of 4096 bins: 2059 frames make two slices.  With 64 taps per channel and hop 1 the
    second slice starts inside the call's first ntaps - hop samples: its history is part history, part input."""
    M, Pp, D, phase, window = shape
    ch = chan_of(ctx, *shape)
    Cc, F = ch.sums_chunk, 2059
    assert F * M * 8 > 64 << 20 and Cc == 8
    x, hist = ctx.vec(rand_c64(31, F * D)), ctx.vec(rand_c64(32, M * Pp - D))
    spec = ch.exec(x, hist, 0, -1, Scale.SN).to_host()
    for block in (0, 100):
        ws, wm = spec_truth.frame_sums(spec, M, block, Cc)
        gs, gm = sums(ctx, ch, x, hist, 0, -1, Scale.SN, False, block, True)
        assert same(gs, ws) and same(gm, wm), block
    gs0, _ = sums(ctx, ch, x, None, 0, -1, Scale.SN, False, 0, True)          # zeros in front
    ws0, _ = spec_truth.frame_sums(ch.exec(x, None, 0, -1, Scale.SN).to_host(), M, 0, Cc)
    assert same(gs0, ws0)


# ---- a stream cut at a row -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((1024, 1, 256, FR, "hann"), (600, 2, 300, FR, "rand"), (1024, 8, 256, ST, "rand")), ids=ident)
def test_two_calls_cut_at_a_row_equal_one(ctx, shape):
    M, Pp, D, phase, window = shape
    ch = chan_of(ctx, *shape)
    B = ch.sums_chunk + 3
    F, cut = 5 * B + 2, 2 * B
    H = M * Pp - D
    x = rand_c64(77, F * D)
    hist = rand_c64(78, H)
    for general in (True, False):
        ws, wm = sums(ctx, ch, ctx.vec(x), ctx.vec(hist), 11, 1, Scale.N, False, B, general)
        a = sums(ctx, ch, ctx.vec(x[:cut * D]), ctx.vec(hist), 11, 1, Scale.N, False, B, general)
        h2 = np.concatenate([hist, x[:cut * D]])[-H:]             # the ntaps - hop samples in front of the second call
        b = sums(ctx, ch, ctx.vec(x[cut * D:]), ctx.vec(h2), 11 + cut, 1, Scale.N, False, B, general)
        assert same(np.concatenate([a[0], b[0]]), ws) and same(np.concatenate([a[1], b[1]]), wm), general


# ---- reproducible, whatever the cache policy and the slice -------------------------------------------------------------
REPRO = ((1024, 1, 1024, FR, "rect"), (1024, 1, 512, FR, "hann"), (4096, 1, 4096, FR, "rect"), (600, 2, 300, FR, "rand"))


def _repro_bytes(ctx, shape):
    M, Pp, D, phase, window = shape
    ch = chan_of(ctx, *shape)
    F = 3 * ch.sums_chunk + 5
    x, hist = ctx.vec(rand_c64(M + 1, F * D)), (ctx.vec(rand_c64(M + 2, M * Pp - D)) if M * Pp > D else None)
    out = b""
    for general in (False, True):
        s, m = ch.sums(x, hist, s=Scale.SN, mirror=True, block=ch.sums_chunk + 3, general=general)
        out += s.to_host().tobytes() + m.to_host().tobytes()
    fs, fm = ctx.frame_sums(x, D, block=7, chunk=4)
    return out + fs.to_host().tobytes() + fm.to_host().tobytes()


def _child(outdir):
    ctx = ap.Context(0)
    for tag, env in (("nt0", {"AETH_NT": "0"}), ("nt1", {"AETH_NT": "1"}), ("slice", {"AETH_SPEC_SLICE_KIB": "64"})):
        for k in ("AETH_NT", "AETH_SPEC_SLICE_KIB"):
            os.environ.pop(k, None)
        os.environ.update(env)
        for i, shape in enumerate(REPRO):
            with open(os.path.join(outdir, f"{tag}_{i}.bin"), "wb") as f:
                f.write(_repro_bytes(ctx, shape))
    chan_of.cache_clear()
    ctx.close()
    print("spec child ok")


def test_results_are_reproducible_under_both_cache_policies_and_any_slice(ctx, tmp_path):
    env = dict(os.environ, AETH_TUNING="1")
    env.pop("AETH_NT", None)
    env.pop("AETH_SPEC_SLICE_KIB", None)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child", str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    for i, shape in enumerate(REPRO):
        want = _repro_bytes(ctx, shape)
        assert _repro_bytes(ctx, shape) == want, "two runs differ"
        for tag in ("nt0", "nt1", "slice"):
            assert open(tmp_path / f"{tag}_{i}.bin", "rb").read() == want, f"{tag} changed the result of {shape}"


# ---- accuracy -------------------------------------------------------------------------------------------------------------
def test_sums_against_complex128(ctx):
    """white noise, M = 1024 Hann, D = 512, F = 64.  The project's bound for fold + transform is -120 dB: ||X - T|| <=
    1e-6 ||T|| over the call.  | |X|^2 - |T|^2 | <= |X - T| (|X| + |T|), so by Cauchy-Schwarz the summed error of the
    powers is at most 1e-6 (2 + 1e-6) sum |T|^2; the f64 additions (64 * 2^-53) and q's own rounding do not show:
    2.1e-6 in all."""
    M, D, F = 1024, 512, 64
    ch = chan_of(ctx, M, 1, D, FR, "hann")
    x = rand_c64(2024, F * D)
    w = ap.chan.prototype("hann", M, 1).astype(np.float64)
    s = np.concatenate([np.zeros(M - D, np.complex128), x.astype(np.complex128)])
    frames = np.stack([s[m * D:m * D + M] * w for m in range(F)])
    truth = (np.abs(np.fft.ifft(frames, axis=1) * M) ** 2).sum(axis=0)       # sign +1, Scale.NONE
    for general in (False, True):
        got, _ = sums(ctx, ch, ctx.vec(x), None, 0, 1, Scale.NONE, False, 0, general)
        figure = np.abs(got - truth).sum() / truth.sum()
        print(f"sum plane against complex128 ({'general' if general else 'fused'}): {figure:.3e} of the total power")
        assert figure <= 2.1e-6


# ---- plane -> levels ------------------------------------------------------------------------------------------------------
def ulps_apart(a, b):
    ia, ib = (v.view(np.int32).astype(np.int64) for v in (a, b))
    ia, ib = (np.where(i < 0, -(i & 0x7fffffff), i) for i in (ia, ib))
    return np.abs(ia - ib)


def test_sum_levels(ctx):
    n = 1 << 16
    rng = np.random.default_rng(9)
    q = np.exp(rng.uniform(-80, 80, n))
    q[:6] = (0.0, np.inf, np.nan, 1.0, 5e-324, 1.7e308)
    plane = ap.DeviceF64(ctx, n)
    ctx.upload(plane.ptr, q)
    for count in (1.0, 2048.0, 3.0):
        with np.errstate(divide="ignore", invalid="ignore"):
            qbar = q / count
            norm = np.sqrt(qbar).astype(np.float32)
            db = (10.0 * np.log10(norm.astype(np.float64))).astype(np.float32)
            pdb = (10.0 * np.log10(qbar)).astype(np.float32)
        got = ctx.sum_levels(plane, count, ap.LEVEL_NORM).to_host()
        assert (got.view(np.uint32)[~np.isnan(norm)] == norm.view(np.uint32)[~np.isnan(norm)]).all() and np.isnan(got[2])
        for kind, want in ((ap.LEVEL_DB, db), (ap.LEVEL_POWER_DB, pdb)):
            got = ctx.sum_levels(plane, count, kind).to_host()
            fin = np.isfinite(want)
            assert (np.isfinite(got) == fin).all()
            assert (got[~fin & ~np.isnan(want)] == want[~fin & ~np.isnan(want)]).all()      # 0 -> -inf, +inf -> +inf
            assert np.isnan(got[2]) and got[0] == -np.inf and got[1] == np.inf
            assert ulps_apart(got[fin], want[fin]).max() <= 1, kind
    for bad in (0.0, -2.0, float("inf"), float("nan")):
        with pytest.raises(ap.AetherError) as e:
            ctx.sum_levels(plane, bad)
        assert e.value.code == _lib.E_ARG and "count" in str(e.value)


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def _free_bytes():
    hip = _lib.load()
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_refusals_launch_nothing(ctx):
    lib = _lib.load()
    M, D = 1024, 512
    ch = chan_of(ctx, M, 1, D, FR, "hann")
    gen = chan_of(ctx, 600, 2, 300, FR, "rand")
    F = 10
    x, hist = ctx.vec(rand_c64(1, F * D + 2)), ctx.vec(rand_c64(2, 2 * 600 - 300))      # the longer history of the two banks
    sp, mp = Plane(ctx, M + 2), Plane(ctx, M + 2)
    X, Hh, S, Mx = x.ptr, hist.ptr, sp.dev.ptr, mp.dev.ptr
    spec = ctx.vec(rand_c64(3, F * M + 2))
    calls = []

    def err(rc, code, *words):
        msg = lib.aeth_last_error().decode()
        assert rc == code, (rc, msg)
        assert all(w in msg for w in words), msg
        calls.append(msg)

    def fs(c=ctx.h, f=spec.ptr, n=F * M, ln=M, block=0, chunk=4, s=S, m=Mx, no=M):
        return lib.aeth_vec_frame_sums(c, P(f), n, ln, block, chunk, P(s), P(m), no)

    def cs(c=ch.h, h=Hh, i=X, n=F * D, sign=1, kind=0, block=0, flags=0, s=S, m=Mx, no=M):
        return lib.aeth_chan_exec_sums(c, P(h), P(i), n, 0, sign, kind, 0.0, 0, block, flags, P(s), P(m), no)

    def refuse_all():
        err(fs(c=None), _lib.E_ARG, "ctx", "null")
        err(fs(f=None), _lib.E_ARG, "null")
        err(fs(s=None, m=None), _lib.E_ARG, "both output planes")
        err(fs(n=0), _lib.E_LEN, "0 samples")
        err(fs(ln=0), _lib.E_LEN, "frames of 0")
        err(fs(n=F * M + 1), _lib.E_LEN, str(F * M + 1), str(M))
        err(fs(chunk=0), _lib.E_LEN, "chunk of 0")
        err(fs(no=M + 1), _lib.E_LEN, str(M + 1))
        err(fs(block=4, no=M), _lib.E_LEN, "3 rows")
        err(fs(f=spec.ptr + 4), _lib.E_ALIGN, hex(spec.ptr + 4))
        err(fs(s=S + 4), _lib.E_ALIGN, hex(S + 4))
        err(fs(m=Mx + 2), _lib.E_ALIGN, hex(Mx + 2))
        err(fs(s=spec.ptr + 8), _lib.E_ARG, "overlaps")
        err(fs(m=S + 8), _lib.E_ARG, "overlaps")
        for c in (ch, gen):
            d, mm = c.hop, c.channels
            err(cs(c=None), _lib.E_ARG, "chan", "null")
            err(cs(c=c.h, flags=2, n=F * d, no=mm), _lib.E_ARG, "flags 0x2")
            err(cs(c=c.h, s=None, m=None, n=F * d, no=mm), _lib.E_ARG, "both output planes")
            err(cs(c=c.h, n=0, no=mm), _lib.E_LEN, "0 input samples")
            err(cs(c=c.h, n=F * d + 1, no=mm), _lib.E_LEN, str(F * d + 1), str(d))
            err(cs(c=c.h, n=F * d, no=mm + 1), _lib.E_LEN, str(mm + 1))
            err(cs(c=c.h, n=F * d, block=3, no=mm), _lib.E_LEN, "4 rows")
            err(cs(c=c.h, n=F * d, no=mm, sign=0), _lib.E_ARG, "sign")
            err(cs(c=c.h, n=F * d, no=mm, kind=4), _lib.E_ARG, "scale kind 4")
            err(cs(c=c.h, n=F * d, no=mm, i=None), _lib.E_ARG, "null")
            err(cs(c=c.h, n=F * d, no=mm, i=X + 4), _lib.E_ALIGN, "aligned")
            err(cs(c=c.h, n=F * d, no=mm, h=Hh + 4), _lib.E_ALIGN, "aligned")
            err(cs(c=c.h, n=F * d, no=mm, s=S + 4), _lib.E_ALIGN, "aligned")
            err(cs(c=c.h, n=F * d, no=mm, m=Mx + 4), _lib.E_ALIGN, hex(Mx + 4))
            err(cs(c=c.h, n=F * d, no=mm, s=X + 8), _lib.E_ARG, "overlaps")
            err(cs(c=c.h, n=F * d, no=mm, m=Hh), _lib.E_ARG, "overlaps")
            err(cs(c=c.h, n=F * d, no=mm, m=S + 8), _lib.E_ARG, "overlaps")

    refuse_all()
    assert len(calls) > 40
    ctx.sync()
    assert sp.untouched() and mp.untouched()
    free0 = _free_bytes()
    for _ in range(3):
        refuse_all()                                              # > 100 refused calls
    ctx.sync()
    assert _free_bytes() == free0
    assert sp.untouched() and mp.untouched()
    # ... and the same arguments without the faults go through
    assert fs() == _lib.OK and cs() == _lib.OK
    ctx.sync()
    assert not sp.untouched() and not mp.untouched()
    sp.host(), mp.host()                                          # the guards are intact


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--child":
    _child(sys.argv[2])
