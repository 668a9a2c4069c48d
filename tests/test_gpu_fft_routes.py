"""GPU parity per ROUTE of the large-FFT planner, not per hand-picked length.

Above the single-workgroup kernels `aeth_fft_create` chooses among a small first factor in registers (R = 3 ... 16, rows up
to 8192 points or up to 20480), a square-root split into two register-resident factors, a fallback split into any two
single-launch factors (one-launch chirp-z sub-plans included), the multi-launch chirp-z transform over a ragged-table
convolution length, over `fourstep_pow2` and over its deep form, and `fourstep_pow2` itself.  Every case below names the
route it stands for and asserts it on `HipFft.route` (aeth_fft_route) before anything is computed: the string is the
device library's own account of the plan.

Per length, both signs: batch 1, then 3, then 1 again on one plan (the work buffer grows between the calls; batch 1 only
from 2^21 points), a different Scale in each call, the output between guard bands (3 samples in front, 64 x 64 + 3
behind: a whole transpose tile, and more than a block of `interleave_kernel` owns), the input bit-unchanged by the
out-of-place call, the in-place call with the bits of the out-of-place one.

Bounds (tests/test_gpu_fft.py): aggregate EVM <= -120 dB against f64 truth, and within 8 dB of an f32 reference of the
same algorithm on the CPU (floor -140 dB): the four-step of the same two factors through oracle.Cfft, or the chirp-z
chain in complex64 with its M-point transforms through oracle.Cfft(M).  Both bounds cover every frame of every call.

The same lengths below 2^20 points (batch 3), every row of the ragged table (batch 7) and the power-of-two four-step
lengths whose column and row kernels nothing else streams past the cache run once more in ONE child process under
AETH_TUNING=1 with AETH_NT=0 and AETH_NT=1: the digests of the raw result bytes equal those of the same calls made with
the defaults in this process.
"""
import hashlib
import json
import os
import re
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
from aether_primitives_amd import HipFft, Scale, _lib                      # noqa: E402
from helpers import bits_equal, rand_c64                                   # noqa: E402

pytestmark = pytest.mark.gpu
TOL_DB = -120.0
GUARD = 7 - 7j
FRONT, BACK = 3, 64 * 64 + 3
RAGGED = "stockham_mixed_ragged"

# (length, what its route must contain)
SMALL_FIRST = [(8232, f"[small 3 | {RAGGED} 2744]"), (9604, f"[small 4 | {RAGGED} 2401]"), (8250, f"[small 5 | {RAGGED} 1650]"),
               (8208, f"[small 6 | {RAGGED} 1368]"), (8211, f"[small 7 | {RAGGED} 1173]"), (8704, f"[small 8 | {RAGGED} 1088]"),
               (8721, f"[small 9 | {RAGGED} 969]"), (10450, f"[small 10 | {RAGGED} 1045]"), (15708, f"[small 12 | {RAGGED} 1309]"),
               (10725, f"[small 15 | {RAGGED} 715]"), (17024, f"[small 16 | {RAGGED} 1064]"),
               # rows of more than 8192 points (the second pass over the first factors)
               (61236, f"[small 7 | {RAGGED} 8748]"), (234375, f"[small 15 | {RAGGED} 15625]")]
SQRT_SPLIT = [(8228, f"[fast {RAGGED} 68 x {RAGGED} 121]"), (8303, f"[fast {RAGGED} 23 x {RAGGED} 361]"),   # no multiple of 64
              (9000000, f"[fast {RAGGED} 3000 x {RAGGED} 3000]")]                                         # above 2^23
FALLBACK = [(8200, f"[fallback bluestein 82 (one launch, M=256) x {RAGGED} 100]"),
            (8260, f"[fallback {RAGGED} 70 x bluestein 118 (one launch, M=256)]"),
            (8214, "[fallback bluestein 74 (one launch, M=256) x bluestein 111 (one launch, M=256)]")]
BLU_RAGGED = [(8193, f"bluestein 8193 (multi launch, M=16875)[{RAGGED} 16875]"),
              (10201, f"bluestein 10201 (multi launch, M=20480)[{RAGGED} 20480]")]
BLU_FOURSTEP = [(10242, "(multi launch, M=32768)[fourstep_pow2 128x256]"), (16385, "(multi launch, M=65536)[fourstep_pow2 256x256]"),
                (65537, "(multi launch, M=262144)[fourstep_pow2 256x1024]"), (131073, "(multi launch, M=524288)[fourstep_pow2 256x2048]"),
                (524289, "(multi launch, M=2097152)[fourstep_pow2 1024x2048]"),
                (1048577, "(multi launch, M=4194304)[fourstep_pow2 2048x2048]")]
BLU_DEEP = [(2097153, "(multi launch, M=8388608)[fourstep_pow2 deep 128x[fourstep_pow2 256x256]]"),
            (4194305, "(multi launch, M=16777216)[fourstep_pow2 deep 256x[fourstep_pow2 256x256]]")]
POW2 = [(1 << 19, "fourstep_pow2 256x2048")]
# (length, algorithm, what its route must contain)
CASES = [(n, algo, want) for algo, group in (("fourstep_mixed", SMALL_FIRST + SQRT_SPLIT + FALLBACK),
                                             ("bluestein", BLU_RAGGED + BLU_FOURSTEP + BLU_DEEP), ("fourstep_pow2", POW2))
         for n, want in group]


def _largest_prime_factor(n):
    best, f = 1, 2
    while f * f <= n:
        while n % f == 0:
            best, n = f, n // f
        f += 1
    return n if n > 1 else best


def truth_f64(oracle, x, n, sign):
    """the DFT of every frame in f64: the oracle's recursive mixed radix where it is fast (prime factors up to 61, below
    2^20 points), numpy's complex128 transform elsewhere (tests/test_gpu_large.py does the same)"""
    x = x.astype(np.complex128)
    if n < (1 << 20) and _largest_prime_factor(n) <= 61:
        return oracle.fft_f64_frames(x, n, sign)
    x = x.reshape(-1, n)
    return (np.fft.ifft(x, axis=1) * float(n) if sign > 0 else np.fft.fft(x, axis=1)).reshape(-1)


# ---- the f32 references: the same algorithm on the CPU, one frame ----------------------------------------------------
_CFFT = {}


def _cfft(oracle, n):
    if n not in _CFFT:
        for k in [k for k in _CFFT if k > 65536]:            # one large plan at a time (tables of up to 2^24 points)
            del _CFFT[k]
        _CFFT[n] = oracle.Cfft(n)
    return _CFFT[n]


def _c64_twiddle(num, den, sign):
    """exp(sign 2 pi i num / den) rounded to f32 from an f64 angle of the exact integer num < den (as the device tables)"""
    a = (2.0 * np.pi * sign) * num.astype(np.float64) / float(den)
    return (np.cos(a) + 1j * np.sin(a)).astype(np.complex64)


def fourstep_f32(oracle, x, n1, n2, sign):
    """X[k1 + n1 k2] of one frame x[j1 n2 + j2]: n1-point transforms down the columns, W^(j2 k1), n2-point transforms
    along the rows, all in complex64 through oracle.Cfft of the two factors"""
    n = n1 * n2
    cols = np.ascontiguousarray(x.reshape(n1, n2).T)                                  # [j2][j1]
    a = _cfft(oracle, n1).frames(cols, sign).reshape(n2, n1)                          # [j2][k1]
    tw = _c64_twiddle((np.arange(n2)[:, None] * np.arange(n1)[None, :]) % n, n, sign)
    b = np.ascontiguousarray((a * tw).astype(np.complex64).T)                         # [k1][j2]
    b = _cfft(oracle, n2).frames(b, sign).reshape(n1, n2)                             # [k1][k2]
    return np.ascontiguousarray(b.T).reshape(-1)


_CHIRP = {}


def chirpz_f32(oracle, x, n, m, sign):
    """the chirp-z chain of one frame in complex64 with the m-point transforms through oracle.Cfft(m); the +j transform
    as conj(DFT-(conj x)), the 1/m of the inverse folded into the filter's spectrum (aeth_fft_big.hip)"""
    f = _cfft(oracle, m)
    if (n, m) not in _CHIRP:
        k = np.arange(n, dtype=np.uint64)
        chirp = _c64_twiddle((k * k) % np.uint64(2 * n), 2 * n, -1)                    # exp(-j pi k^2 / n)
        filt = np.zeros(m, np.complex64)
        filt[:n] = chirp.conj()
        filt[m - n + 1:] = chirp[:0:-1].conj()
        _CHIRP.clear()                                                                # one length at a time
        _CHIRP[(n, m)] = chirp, (f.exec_sign(filt, -1) * np.float32(1.0 / m)).astype(np.complex64)
    chirp, spec = _CHIRP[(n, m)]
    a = np.zeros(m, np.complex64)
    a[:n] = (x.conj() if sign > 0 else x) * chirp
    a = (f.exec_sign(a, -1) * spec).astype(np.complex64)
    y = (f.exec_sign(a, +1)[:n] * chirp).astype(np.complex64)
    return y.conj() if sign > 0 else y


def reference_f32(oracle, route, x, n, sign):
    """one frame through the f32 restatement of the plan's top level"""
    m = re.match(r"fourstep_mixed\[small (\d+) ", route)
    if m:
        return fourstep_f32(oracle, x, int(m.group(1)), n // int(m.group(1)), sign)
    if route.startswith("fourstep_mixed["):
        n1 = int(re.match(r"fourstep_mixed\[\w+ \w+ (\d+)", route).group(1))
        return fourstep_f32(oracle, x, n1, n // n1, sign)
    m = re.match(r"fourstep_pow2 (\d+)x(\d+)$", route)
    if m:
        return fourstep_f32(oracle, x, int(m.group(1)), int(m.group(2)), sign)
    m = re.match(r"bluestein \d+ \(multi launch, M=(\d+)\)", route)
    assert m, route
    return chirpz_f32(oracle, x, n, int(m.group(1)), sign)


def _evm_db(oracle, got, truth):
    return oracle.evm_db(np.ascontiguousarray(got, np.complex64), truth)


# ---- the routes against truth --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,algo,want", CASES, ids=[str(c[0]) for c in CASES])
def test_route_meets_truth(ctx, oracle, n, algo, want):
    f = HipFft(ctx, n)
    route = f.route
    assert route.startswith(algo) and want in route, route
    assert f.algorithm == algo and f.len() == n
    calls = ((1, Scale.NONE), (3, Scale.X(0.37)), (1, Scale.SN)) if n < (1 << 21) else ((1, Scale.X(0.37)),)
    # the chirp-z lengths from 2^21 points up: the +j call gets the conjugate of the -j call's input, so that its truth
    # and its f32 reference are the conjugates of that call's (DFT+(x) = conj(DFT-(conj x)), which is also how
    # chirpz_f32 forms it) and the CPU transforms of up to 2^24 points are done once, not twice.  The device
    # conjugates on the way in as well, so at these lengths the +j call sends the -j call's data through the same
    # transforms: what it adds is blu_pre<true> / blu_post<true> at that size, nothing else.  The chirp-z lengths below
    # 2^21 use independent inputs for the two signs.
    share = algo == "bluestein" and n >= (1 << 21)
    for call, (batch, s) in enumerate(calls):
        shared = None
        for sign in (-1, +1):
            x = rand_c64(3 * n + 7 * call + (0 if share else sign), n * batch)
            if share and sign > 0:
                x = x.conj()
            factor = float(s.factor(n))
            inp = ctx.vec(x)
            buf = ctx.vec(np.full(FRONT + x.size + BACK, GUARD, np.complex64))
            f.exec(inp, buf.slice(FRONT, FRONT + x.size), sign, s)
            h = buf.to_host()
            got = h[FRONT:FRONT + x.size]
            assert (h[:FRONT] == GUARD).all() and (h[FRONT + x.size:] == GUARD).all(), (call, sign, "wrote outside the output")
            assert bits_equal(inp.to_host(), x), (call, sign, "the out-of-place call changed its input")
            f.exec(inp, inp, sign, s)
            assert bits_equal(inp.to_host(), got), (call, sign, "in place differs from out of place")
            if shared is None:
                truth = truth_f64(oracle, x, n, sign) * factor
                ref = np.concatenate([reference_f32(oracle, route, x[k * n:(k + 1) * n], n, sign) for k in range(batch)])
                ref = (ref.astype(np.complex128) * factor).astype(np.complex64)
                if share:
                    shared = truth, ref
            else:
                truth, ref = shared[0].conj(), shared[1].conj()
            e_gpu = _evm_db(oracle, got, truth)
            e_ref = _evm_db(oracle, ref, truth)
            print(f"N={n} batch={batch} sign={sign:+d} {s!r}: GPU {e_gpu:.1f} dB, f32 reference {e_ref:.1f} dB")
            assert e_gpu <= TOL_DB, f"N={n} batch={batch} sign={sign:+d}: GPU vs f64 truth {e_gpu:.1f} dB"
            assert e_gpu <= max(e_ref, -140.0) + 8.0, \
                f"N={n} batch={batch} sign={sign:+d}: GPU {e_gpu:.1f} dB vs f32 reference {e_ref:.1f} dB"


def test_every_small_first_factor_has_a_case():
    """R = 3 ... 16 each in an asserted route; R = 2 cannot be planned (fft_run_fourstep_mixed, tools/variant_coverage.py)"""
    seen = {int(re.search(r"small (\d+) ", w).group(1)) for _, w in SMALL_FIRST}
    assert seen == {3, 4, 5, 6, 7, 8, 9, 10, 12, 15, 16}


# ---- lengths without a route ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8388609, 16777213])
def test_lengths_without_a_route_are_refused(ctx, oracle, n):
    """(2^23, 2^24]: no power of two, no split into two single-launch factors -> the chirp-z convolution would need
    2^25 points.  AETH_E_UNSUPPORTED with the requested length and the reason, and the context plans on as before."""
    with pytest.raises(ap.AetherError) as e:
        HipFft(ctx, n)
    msg = str(e.value)
    assert e.value.code == _lib.E_UNSUPPORTED, msg
    assert f"FFT length {n}:" in msg and "33554432 > 2^24" in msg and "products of two single-launch lengths" in msg, msg
    if n == 8388609:                                   # the one-shot calls plan through the same door
        with pytest.raises(ap.AetherError, match=f"FFT length {n}:"):
            ctx.vec(np.zeros(n, np.complex64)).vec_fft(Scale.NONE)
    x = rand_c64(n % 1000, 3 * 128)
    d = ctx.vec(x)
    HipFft(ctx, 128).ifwd(d, Scale.NONE)
    assert _evm_db(oracle, d.to_host(), oracle.fft_f64_frames(x.astype(np.complex128), 128, +1)) <= TOL_DB
    assert HipFft(ctx, 1 << 24).route == "fourstep_pow2 deep 256x[fourstep_pow2 256x256]"     # truth: tests/test_gpu_large.py


# ---- forced cache policy ------------------------------------------------------------------------------------------------
def ragged_rows():
    """the lengths of aeth_fft_ragged_table.inc, in the table's order"""
    txt = open(os.path.join(ROOT, "aether_primitives_amd", "csrc", "aeth_fft_ragged_table.inc")).read()
    return [int(v) for v in re.findall(r"^AETH_RAGGED_P[0-3]\((\d+),", txt, re.M)]


RAGGED_SLICES = 4
# fourstep_pow2 with 512-point rows (2^17), 512- / 1024- / 2048-point columns (2^20 ... 2^22): their non-temporal builds
# serve batches past the cache only, which no test of this size has
POW2_EXTRA = (1 << 17, 1 << 20, 1 << 21, 1 << 22)


def battery_slices():
    """{slice: [(length, batch)]}"""
    rows = ragged_rows()
    per = (len(rows) + RAGGED_SLICES - 1) // RAGGED_SLICES
    out = {"routes": [(c[0], 3) for c in CASES if c[0] < (1 << 20)] + [(n, 1) for n in POW2_EXTRA]}
    for k in range(RAGGED_SLICES):
        out[f"ragged{k}"] = [(n, 7) for n in rows[k * per:(k + 1) * per]]
    return out


def run_slice(ctx, items):
    """{key: digest of the result's bytes} of both signs of every (length, batch)"""
    out = {}
    for n, batch in items:
        f = HipFft(ctx, n)
        x = ctx.vec(rand_c64(n, n * batch))
        y = ctx.empty(n * batch)
        for sign, s in ((+1, Scale.SN), (-1, Scale.X(0.5))):
            f.exec(x, y, sign, s)
            out[f"{n}x{batch}{'f' if sign > 0 else 'b'}"] = hashlib.blake2b(y.to_host().tobytes(), digest_size=16).hexdigest()
    return out


def _child(outdir):
    """every slice under AETH_NT=0 and AETH_NT=1 -> outdir/nt<v>__<slice>.json.  Stops at the first error."""
    ctx = ap.Context(0)
    for nt in ("0", "1"):
        os.environ["AETH_NT"] = nt
        for name, items in battery_slices().items():
            with open(os.path.join(outdir, f"nt{nt}__{name}.json"), "w") as fh:
                json.dump(run_slice(ctx, items), fh)
    del os.environ["AETH_NT"]
    ctx.close()
    print("battery ok")


@pytest.fixture(scope="module")
def forced(tmp_path_factory):
    """run the child once; {(nt, slice): {key: digest}}"""
    d = tmp_path_factory.mktemp("fft_routes")
    env = dict(os.environ, AETH_TUNING="1")
    env.pop("AETH_NT", None)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--battery", str(d)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    if r.returncode != 0:
        pytest.fail(f"battery child exited {r.returncode}:\n{r.stderr[-4000:]}")
    out = {}
    for f in sorted(os.listdir(d)):
        nt, name = f[:-5].split("__")
        out[(nt, name)] = json.load(open(d / f))
    return out


@pytest.mark.parametrize("name", list(battery_slices()))
def test_forced_cache_policy_gives_the_default_bits(ctx, forced, name):
    items = battery_slices()[name]
    if name.startswith("ragged"):
        for n, _ in items:
            assert HipFft(ctx, n).route == f"{RAGGED} {n}"
    else:
        assert {n for n, _ in items} >= {c[0] for c in CASES if c[0] < (1 << 20)}
    base = run_slice(ctx, items)
    assert len(base) == 2 * len(items)
    for nt in ("nt0", "nt1"):
        got = forced[(nt, name)]
        assert list(got) == list(base)
        bad = [k for k in base if got[k] != base[k]]
        assert not bad, f"AETH_NT={nt[-1]} changed {bad}"


def test_the_ragged_sweep_is_the_whole_table():
    rows = ragged_rows()
    assert len(rows) == len(set(rows)) == 674 and min(rows) == 3 and max(rows) == 20480
    assert sorted(n for k, v in battery_slices().items() if k.startswith("ragged") for n, _ in v) == sorted(rows)


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--battery":
    _child(sys.argv[2])
