"""GPU: aeth_vec_stats, aeth_vec_levels and aeth_fft_exec_levels against numpy, from the same bytes the device sees.

Definitions (csrc/aeth_levels.h), with re, im as f64:  q = re*re + im*im (one rounding of |c|^2),  norm = f32(sqrt(q)),
DB = f32(10 * log10(f64(norm))) (the reference's DB::from(c.norm()).db()),  POWER_DB = f32(10 * log10(q)).

Exact (bitwise): NORM levels; n, n_nan, min / max index and norm of the statistics; the whole record across calls,
alignments, cache policy and host / device flavour; aeth_fft_exec_levels against the separate calls.

Derived tolerances (none measured on the code under test):
  * power: relative error against the long-double sum at most n * 2^-52.  The q_i are the same bits on both sides; any
    summation order of n non-negative f64 terms has relative error at most (n - 1) * 2^-53 to first order; the factor
    two covers the second-order term and the final division.  mean_re / mean_im: absolute error at most
    2^-52 * sum(|re_i|) (the same bound for signed terms, divided by n).  An f32 accumulator (1e-7 at best) fails this,
    no legitimate f64 tree does.
  * dB kinds: at most ONE f32 ulp from numpy's f32(10 * log10(v)), -inf / NaN where numpy has them: both f64 logarithms
    are accurate to a few f64 ulps and an f32 ulp is 2^29 of those, so the two roundings can differ only where the true
    value lies within a few f64 ulps of an f32 rounding boundary, and then by one ulp.  For the same reason at most 1
    element in 10^4 may differ at all (numpy's own three f64 routes to log10 differ in none of 2^22).
  * NORM levels of a transform against f64 truth: the suite's TOL_DB = -120 aggregate EVM, as for the transform itself."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import aether_primitives_amd as ap                                        # noqa: E402
from aether_primitives_amd import HipFft, Scale                            # noqa: E402
from helpers import bits_equal, rand_c64                                   # noqa: E402

pytestmark = pytest.mark.gpu
TOL_DB = -120.0
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 4096, 100003, (1 << 20) + 1)
KINDS = (ap.LEVEL_NORM, ap.LEVEL_DB, ap.LEVEL_POWER_DB)
GUARD_F = np.float32(-7.25)


# ---- numpy expectations ----------------------------------------------------------------------------------------
def q_of(x):
    re, im = x.real.astype(np.float64), x.imag.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        return re * re + im * im


def norm_of(x):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.sqrt(q_of(x)).astype(np.float32)


def level_of(x, kind):
    """numpy's value of a level kind (for the dB kinds: the value the device may miss by one ulp)"""
    if kind == ap.LEVEL_NORM:
        return norm_of(x)
    v = norm_of(x).astype(np.float64) if kind == ap.LEVEL_DB else q_of(x)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        return (10.0 * np.log10(v)).astype(np.float32)


def ulps_apart(a, b):
    """per element: 0 where both are NaN or the same value, the distance in f32 ulps where both are finite, a huge
    number where one is NaN / infinite and the other is not the same"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    def ordered(v):
        i = v.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    d = np.abs(ordered(a) - ordered(b))
    special = ~(np.isfinite(a) & np.isfinite(b))
    same = (np.isnan(a) & np.isnan(b)) | (a == b)
    return np.where(special, np.where(same, 0, 1 << 40), d)


def check_levels(got, x, kind, what):
    want = level_of(x, kind)
    if kind == ap.LEVEL_NORM:
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        nan_both = np.isnan(got[bad]) & np.isnan(want[bad])
        assert not bad[~nan_both].size, (what, "NORM not bit-equal", bad[:5], got[bad[:5]], want[bad[:5]])
        return
    d = ulps_apart(got, want)
    differ = int((d != 0).sum())
    print(f"{what} kind {kind}: {differ} of {got.size} differ from numpy, max {int(d.max()) if d.size else 0} ulp")
    assert d.max() <= 1, (what, kind, int(d.argmax()), got[d.argmax()], want[d.argmax()])
    assert differ * 10000 <= got.size, (what, kind, differ, got.size, "more than 1 element in 10^4 differs from numpy")


def specials():
    """every pairing of 0, -0, denormals, 1, 3e38, +-inf and NaN as the two components"""
    vals = np.array([0.0, -0.0, 1e-45, -1e-40, 1.0, 3e38, -3e38, np.inf, -np.inf, np.nan], np.float32)
    re, im = np.meshgrid(vals, vals)
    x = np.empty(vals.size ** 2, np.complex64)
    x.real, x.imag = re.reshape(-1), im.reshape(-1)
    return x


def at_offset(ctx, x, off):
    """x on the device, `off` samples into its allocation (off = 1: an odd 8-byte slot)"""
    return ctx.vec(np.concatenate([np.zeros(off, np.complex64), x])).slice(off, off + x.size)


def guarded_f32(ctx, n, front, back):
    """a float buffer of n levels with guard values around it: (whole buffer, view of the n levels)"""
    buf = ap.DeviceF32(ctx, front + n + back)
    ctx.upload(buf.ptr, np.full(front + n + back, GUARD_F, np.float32))
    return buf, buf.slice(front, front + n)


def guards_intact(buf, n, front):
    h = buf.to_host()
    return bool((h[:front] == GUARD_F).all() and (h[front + n:] == GUARD_F).all())


# ---- 1 / 7: aeth_vec_levels ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_vec_levels_every_size_and_alignment(ctx, n):
    """NORM bit-equal, the dB kinds within one ulp, at a 16-byte-aligned base and at base + 1 sample, the output at a
    16-byte-aligned and at an odd 4-byte slot; guards untouched, input unchanged"""
    x = rand_c64(n + 5, n)
    for off, front in ((0, 4), (1, 1), (0, 3), (1, 4)):
        d = at_offset(ctx, x, off)
        for kind in KINDS:
            buf, lv = guarded_f32(ctx, n, front, 9)
            assert d.levels(kind, out=lv) is lv
            check_levels(lv.to_host(), x, kind, f"n={n} off={off} front={front}")
            assert guards_intact(buf, n, front), (n, off, front, kind, "wrote outside the levels")
        assert bits_equal(d.to_host(), x)


def test_vec_levels_special_values(ctx):
    """0, -0, denormals, 3e38 (norm overflows to +inf, the power level stays finite), +-inf and NaN in either component"""
    x = specials()
    for off in (0, 1):
        d = at_offset(ctx, x, off)
        for kind in KINDS:
            buf, lv = guarded_f32(ctx, x.size, 2, 5)
            d.levels(kind, out=lv)
            got, want = lv.to_host(), level_of(x, kind)
            assert (np.isnan(got) == np.isnan(want)).all(), kind
            assert (np.isneginf(got) == np.isneginf(want)).all() and (np.isposinf(got) == np.isposinf(want)).all(), kind
            check_levels(got, x, kind, f"specials off={off}")
            assert guards_intact(buf, x.size, 2)
    assert np.isneginf(level_of(x[:1], ap.LEVEL_DB)).all()              # norm = 0 -> -inf, as Rust's f64::log10


# ---- 2 / 6: aeth_vec_stats -------------------------------------------------------------------------------------
def check_stats(st, x, what):
    """exact fields against numpy, sums against the long-double truth within the derived bounds"""
    n = x.size
    q = q_of(x)
    nan = np.isnan(q)
    cand = np.flatnonzero(~nan)
    assert st.n == n and st.n_nan == int(nan.sum()), (what, st)
    if cand.size:
        imin, imax = cand[np.argmin(q[cand])], cand[np.argmax(q[cand])]       # argmin / argmax: the lowest index of equals
        assert (st.min_index, st.max_index) == (imin, imax), (what, st, imin, imax)
        nrm = norm_of(x[[imin, imax]])
        assert np.float32(st.min_norm).view(np.uint32) == nrm[0].view(np.uint32), (what, st, nrm)
        assert np.float32(st.max_norm).view(np.uint32) == nrm[1].view(np.uint32), (what, st, nrm)
    else:
        assert (st.min_index, st.max_index) == (n, n) and np.isnan(st.min_norm) and np.isnan(st.max_norm), (what, st)
    if nan.any() or not np.isfinite(q).all():
        sq, sre, sim = q.sum(), x.real.astype(np.float64).sum(), x.imag.astype(np.float64).sum()
        for got, want in ((st.power, sq), (st.mean.real, sre), (st.mean.imag, sim)):
            assert np.isnan(got) == np.isnan(want) and np.isinf(got) == np.isinf(want), (what, got, want)
        return
    ld = np.longdouble
    truth = np.sum(q, dtype=ld) / ld(n)
    rel = abs(ld(st.power) - truth) / truth if truth else abs(ld(st.power))
    print(f"{what}: power rel err {float(rel):.3e} (bound {n * 2.0 ** -52:.3e})")
    assert rel <= n * 2.0 ** -52, (what, st.power, float(truth), float(rel))
    for got, comp in ((st.mean.real, x.real), (st.mean.imag, x.imag)):
        c = comp.astype(np.float64)
        err = abs(ld(got) - np.sum(c, dtype=ld) / ld(n))
        bound = ld(2.0 ** -52) * np.sum(np.abs(c), dtype=ld)
        assert err <= bound, (what, got, float(err), float(bound))


@pytest.mark.parametrize("n", SIZES)
def test_vec_stats_every_size_and_alignment(ctx, n):
    x = rand_c64(n + 9, n)
    for off in (0, 1):
        check_stats(at_offset(ctx, x, off).stats(), x, f"n={n} off={off}")


@pytest.mark.parametrize("n", [257, 100003, (1 << 20) + 1])
def test_vec_stats_ties_go_to_the_lowest_index(ctx, n):
    x = rand_c64(n + 1, n)
    hi, lo = n - 2, n // 3
    x[[lo, hi]] = 9 - 9j                                            # the maximum, twice
    x[[lo + 1, hi - 1]] = 0                                         # the minimum, twice
    # the same q from a different sample: (9, -9) and (-9, 9) tie, the lower index still wins
    x[lo // 2] = -9 + 9j
    x[lo // 2 + 1] = -0.0
    for off in (0, 1):
        st = at_offset(ctx, x, off).stats()
        assert (st.max_index, st.min_index) == (lo // 2, lo // 2 + 1), st
        check_stats(st, x, f"ties n={n} off={off}")


@pytest.mark.parametrize("n", [3, 257, 100003])
def test_vec_stats_counts_and_skips_nan(ctx, n):
    for where in ([0], [n - 1], [n // 2], [0, n // 2, n - 1]):
        x = rand_c64(n + 2, n)
        x[where] = [complex(np.nan, 1.0), complex(2.0, np.nan), complex(np.nan, np.nan)][:len(where)]
        big = (where[-1] + 1) % n                                   # the extremes right beside a NaN sample
        if big not in where:
            x[big] = 50
        for off in (0, 1):
            st = at_offset(ctx, x, off).stats()
            assert st.n_nan == len(where) and np.isnan(st.power) and np.isnan(st.mean.real + st.mean.imag), st
            check_stats(st, x, f"nan at {where} n={n} off={off}")
    x = np.full(n, complex(np.nan, 0), np.complex64)
    st = ctx.vec(x).stats()
    assert st.n_nan == n and (st.min_index, st.max_index) == (n, n) and np.isnan(st.min_norm) and np.isnan(st.max_norm), st
    # infinities are candidates, not NaN
    x = rand_c64(n + 3, n); x[n // 2] = complex(-np.inf, 1)
    st = ctx.vec(x).stats()
    assert st.n_nan == 0 and st.max_index == n // 2 and np.isposinf(st.max_norm) and np.isposinf(st.power), st
    x[:] = complex(np.inf, 0)
    st = ctx.vec(x).stats()
    assert (st.min_index, st.max_index) == (0, 0) and np.isposinf(st.min_norm), st


def test_vec_stats_empty_is_a_length_error(ctx):
    with pytest.raises(ap.LengthMismatch):
        ctx.empty(0).stats()


# ---- 3: reproducibility ------------------------------------------------------------------------------------------
REPRO_SIZES = (1, 257, 4096, 8191, 8192, 8193, 100003, (1 << 20) + 1)


def _repro_input(n):
    return rand_c64(3 * n + 1, n, scale=3.0)


@pytest.mark.parametrize("n", REPRO_SIZES)
def test_vec_stats_record_is_reproducible(ctx, n):
    """(a) two calls, (b) aligned base and base + 1 sample, (d) device and host flavour: the same 64 bytes"""
    x = _repro_input(n)
    d = ctx.vec(x)
    first = d.stats().raw
    assert len(first) == 64
    assert d.stats().raw == first, "two calls differ"
    assert at_offset(ctx, x, 1).stats().raw == first, "the pointer's alignment changed the record"
    assert at_offset(ctx, x, 3).stats().raw == first
    assert ap.HostVec(ctx, x.copy()).stats().raw == first, "host and device flavour differ"
    ctx.trim()                                                      # the slab is released and grown again
    assert d.stats().raw == first


def _child(outdir):
    """the records of REPRO_SIZES under the AETH_NT forced by the parent; one file per size"""
    ctx = ap.Context(0)
    for nt in ("0", "1"):
        os.environ["AETH_NT"] = nt
        for n in REPRO_SIZES:
            x = _repro_input(n)
            with open(os.path.join(outdir, f"nt{nt}_{n}.bin"), "wb") as f:
                f.write(ctx.vec(x).stats().raw)
                for kind in KINDS:
                    f.write(ctx.vec(x).levels(kind).to_host().tobytes())
    ctx.close()
    print("stats child ok")


def test_vec_stats_and_levels_do_not_depend_on_the_cache_policy(ctx, tmp_path):
    """(c) AETH_TUNING=1 with AETH_NT=0 and AETH_NT=1 in a child process: the records (and the levels) of this process"""
    env = dict(os.environ, AETH_TUNING="1")
    env.pop("AETH_NT", None)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child", str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    for n in REPRO_SIZES:
        x = _repro_input(n)
        d = ctx.vec(x)
        want = d.stats().raw + b"".join(d.levels(kind).to_host().tobytes() for kind in KINDS)
        for nt in ("0", "1"):
            got = open(tmp_path / f"nt{nt}_{n}.bin", "rb").read()
            assert got[:64] == want[:64], f"AETH_NT={nt} changed the record at n={n}"
            assert got == want, f"AETH_NT={nt} changed the levels at n={n}"


# ---- 4 / 8: aeth_fft_exec_levels ---------------------------------------------------------------------------------
# frames per workgroup of the power-of-two transform (aeth_fft_core.h: CfgFor -> Cfg::F = WG / T)
FRAMES_PER_WG = {2: 64, 4: 64, 8: 64, 16: 64, 32: 16, 64: 8, 128: 8, 256: 4, 512: 1, 1024: 1, 2048: 1, 4096: 1, 8192: 1}
SCALES = (Scale.NONE, Scale.SN, Scale.X(0.37))
SIGNS = (ap.SIGN_REF_FWD, ap.SIGN_REF_BWD)
NT_SAMPLES = (128 << 20) // 12 + 4096          # the fused call moves 12 B per sample: beyond the 128 MiB threshold


def _batches(n):
    f = FRAMES_PER_WG[n]
    return sorted({1, max(f - 1, 2), f + 1, 301})


def _levels_both_ways(ctx, f, x, n, batch, what):
    """every sign, scale, mirror and kind: the fused call against exec / exec_mirrored + vec_levels, bit for bit"""
    xin = ctx.vec(x)
    spec = ctx.empty(x.size)
    back = FRAMES_PER_WG.get(n, 1) * n + 5                           # a whole workgroup's frames past the end
    for sign in SIGNS:
        for s in SCALES:
            for mirror in (False, True):
                if mirror:
                    check = f._lib.aeth_fft_exec_mirrored(f.h, xin._p(), xin.n, spec._p(), batch, sign, s.kind, s.x)
                else:
                    check = f._lib.aeth_fft_exec(f.h, xin._p(), xin.n, spec._p(), batch, sign, s.kind, s.x)
                assert check == 0
                for kind in KINDS:
                    want = spec.levels(kind).to_host()
                    buf, lv = guarded_f32(ctx, x.size, 3, back)
                    f.levels(xin, s, mirror=mirror, kind=kind, out=lv, sign=sign)
                    h = buf.to_host()
                    got = h[3:3 + x.size]
                    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
                    assert not bad.size, (what, sign, s, mirror, kind, bad.size, bad[:4], got[bad[:4]], want[bad[:4]])
                    assert (h[:3] == GUARD_F).all() and (h[3 + x.size:] == GUARD_F).all(), (what, sign, s, mirror, kind, "wrote outside")
    assert bits_equal(xin.to_host(), x), (what, "the input changed")


@pytest.mark.parametrize("n,batch", [(n, b) for n in FRAMES_PER_WG for b in _batches(n)])
def test_fft_levels_equal_the_separate_calls(ctx, n, batch):
    f = HipFft(ctx, n, max_batch=batch)
    _levels_both_ways(ctx, f, rand_c64(n * 5 + batch, n * batch), n, batch, f"n={n} batch={batch}")


@pytest.mark.parametrize("n", list(FRAMES_PER_WG))
def test_fft_levels_equal_the_separate_calls_beyond_the_cache(ctx, n):
    """a batch whose traffic exceeds the cache threshold: the non-temporal builds of the same kernels"""
    batch = (NT_SAMPLES + n - 1) // n
    pat = rand_c64(n + 77, 1 << 20)
    x = np.tile(pat, (n * batch + pat.size - 1) // pat.size)[:n * batch]
    x[::4099] *= 3                                                  # the repeats of the pattern are not all alike
    f = HipFft(ctx, n, max_batch=batch)
    _levels_both_ways(ctx, f, x, n, batch, f"n={n} batch={batch} (NT)")


OTHER_LENGTHS = (100, 1000, 1331, 2176, 4099, 8192, 32768, 40960, 65536)


def test_fft_levels_other_algorithms(ctx):
    """one length or more of every other algorithm: the transform goes through the plan's temp, the same bits"""
    seen = set()
    for n in OTHER_LENGTHS:
        batch = 3 if n <= 8192 else 2
        f = HipFft(ctx, n, max_batch=batch)
        assert f.algorithm != "stockham_pow2", n
        seen.add(f.algorithm)
        _levels_both_ways(ctx, f, rand_c64(n, n * batch), n, batch, f"n={n} ({f.algorithm})")
    assert seen >= {"stockham_mixed_ragged", "stockham_mixed", "fourstep_pow2", "fourstep_mixed", "bluestein"}, seen


def test_fft_levels_arguments(ctx):
    f = HipFft(ctx, 64)
    x = ctx.vec(rand_c64(1, 128))
    lv = ap.DeviceF32(ctx, 128)
    with pytest.raises(ap.LengthMismatch):
        f.levels(x, out=ap.DeviceF32(ctx, 127))
    with pytest.raises(ap.LengthMismatch):
        f.levels(ctx.vec(rand_c64(1, 100)), out=ap.DeviceF32(ctx, 100))
    with pytest.raises(ap.AetherError, match="level kind"):
        f.levels(x, kind=3, out=lv)
    with pytest.raises(ap.AetherError, match="overlap"):
        f.levels(x, out=ap.DeviceF32(ctx, 128, ptr=x.ptr, offset=64))
    with pytest.raises(ap.AetherError, match="overlap"):
        x.levels(out=ap.DeviceF32(ctx, 128, ptr=x.ptr))
    assert f.levels(ctx.empty(0), out=ap.DeviceF32(ctx, 0)).n == 0


@pytest.mark.parametrize("mirror", [False, True])
def test_fft_levels_2048_against_f64_truth(ctx, oracle, mirror):
    n, batch = 2048, 37
    x = rand_c64(2048, n * batch)
    f = HipFft(ctx, n, max_batch=batch)
    truth = (oracle.fft_f64_frames(x.astype(np.complex128), n, ap.SIGN_REF_FWD) / np.sqrt(n)).reshape(batch, n)
    if mirror:
        truth = np.roll(truth, n // 2, axis=1)
    got = f.levels(ctx.vec(x), Scale.SN, mirror=mirror, kind=ap.LEVEL_NORM).to_host()
    e = oracle.evm_db(got.astype(np.complex64), np.abs(truth).reshape(-1).astype(np.complex128))
    print(f"FFT-2048 NORM levels, mirror={mirror}: EVM {e:.1f} dB")
    assert e <= TOL_DB, e


# ---- 5: byte offsets beyond 4 GiB ---------------------------------------------------------------------------------
def test_stats_and_levels_beyond_4gib(ctx):
    """a pattern of period 2^22 tiled on the device, the maximum planted in the LAST sample: index and norms exact, power
    and mean within their bounds (the truth from one period and the tail); the levels on windows at the head, the 4 GiB
    crossing and the ragged tail.  Element indices beyond 2^32 are not reached (32 GiB of samples); the code is size_t
    throughout."""
    P, CROSS = 1 << 22, 1 << 29
    n = CROSS + (1 << 20) + 3
    pat = rand_c64(61, P)
    pd = ctx.vec(pat)
    x = ctx.empty(n)
    for o in range(0, n, P):
        m = min(P, n - o)
        x.slice(o, o + m).vec_clone(pd.slice(0, m))
    top = np.array([-40 + 9j], np.complex64)
    ctx.upload(x.slice(n - 1, n).ptr, top)
    st = x.stats()
    full, rem = divmod(n, P)
    q = q_of(pat)
    assert st.n == n and st.n_nan == 0
    assert st.max_index == n - 1 and np.float32(st.max_norm).view(np.uint32) == norm_of(top)[0].view(np.uint32), st
    assert st.min_index == int(np.argmin(q)) and np.float32(st.min_norm).view(np.uint32) == norm_of(pat[[np.argmin(q)]])[0].view(np.uint32), st
    ld = np.longdouble
    def total(v):
        v = v.astype(np.float64)
        return ld(full) * np.sum(v, dtype=ld) + np.sum(v[:rem], dtype=ld)
    last = (rem - 1) % P
    truth = (total(q) - ld(q[last]) + ld(q_of(top)[0])) / ld(n)
    rel = abs(ld(st.power) - truth) / truth
    print(f"n = {n}: power rel err {float(rel):.3e} (bound {n * 2.0 ** -52:.3e})")
    assert rel <= n * 2.0 ** -52, (st.power, float(truth))
    for got, comp, t in ((st.mean.real, pat.real, top.real[0]), (st.mean.imag, pat.imag, top.imag[0])):
        want = (total(comp) - ld(comp[last]) + ld(t)) / ld(n)
        bound = ld(2.0 ** -52) * (total(np.abs(comp)) + abs(ld(t)))
        assert abs(ld(got) - want) <= bound, (got, float(want))
    assert x.stats().raw == st.raw
    lv = x.levels(ap.LEVEL_NORM)
    for lo, hi in ((0, 4096), (CROSS - 4096, CROSS + 4096), (n - 4099, n)):
        xs = pat[np.arange(lo, hi) % P]
        if hi == n:
            xs[-1] = top[0]
        check_levels(lv.slice(lo, hi).to_host(), xs, ap.LEVEL_NORM, f"levels [{lo}, {hi})")


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--child":
    _child(sys.argv[2])
