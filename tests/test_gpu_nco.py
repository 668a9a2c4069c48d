"""GPU: the oscillator (csrc/aeth_nco.hip, aeth_nco_mix / aeth_nco_tone) bit for bit against the numpy restatement of its
definition (tests/nco_truth.py), and its refusals.  Where the restatement gives NaN the device must give NaN; the
payload is not compared.

Launch geometry: a 256-lane workgroup covers 512 samples on the 16-byte route (both pointers on the same 8-byte parity,
one sample peeled in front when that parity is odd and one behind when a sample is left over) and 256 samples on the
8-byte route (parities differ).  The lengths below sit on both sides of every one of those edges; every case is a few
thousand samples at most."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):                             # also run as a script: the AETH_NT child
    if _p not in sys.path:
        sys.path.insert(0, _p)

import nco_truth                                                           # noqa: E402
from helpers import bits_equal, rand_c64                                   # noqa: E402

import aether_primitives_amd as ap                                         # noqa: E402
from aether_primitives_amd import _lib                                     # noqa: E402

pytestmark = pytest.mark.gpu

TOL_DB = -120.0                                   # tests/test_gpu_fft.py:20
GUARD = 16                                        # samples: keeps a 16-byte aligned buffer 16-byte aligned
SENT = np.complex64(-7.5 + 3.25j)
LENGTHS = (1, 2, 3, 255, 256, 257, 511, 512, 513, 4099)

_rng = np.random.default_rng(2024)
_r64 = lambda: int(_rng.integers(0, 2 ** 64, dtype=np.uint64))            # noqa: E731
SHIFT = (_r64(), _r64(), 0)                       # random phase and step, no chirp
CHIRP = (_r64(), _r64(), _r64())                  # all three random: T(n) * rate wraps at almost every sample
WORD_SETS = {
    "zero": (0, 0, 0),
    "shift": SHIFT,
    "chirp": CHIRP,
    "alternate": (0, 1 << 63, 0),                 # +1, -1, +1, ...
    "quarter": (0, 1 << 62, 0),
    "fast-chirp": (12345, 0xfedcba9876543211, (1 << 63) + (1 << 40) + 1),
}
AMP = 0.8125


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


def osc(ctx, words, n0=0):
    return ap.Nco.from_words(ctx, *words, position=n0)


# ---- 1. lengths and pointer parities, both operations ----------------------------------------------------------------------
@pytest.mark.parametrize("n", LENGTHS)
def test_lengths_and_parities_bit_for_bit(ctx, n):
    x = rand_c64(100 + n, n)
    n0 = 2 ** 40 + 7
    for words in (SHIFT, CHIRP):
        want = nco_truth.mix(words, n0, x)
        twant = nco_truth.tone(words, n0, AMP, n)
        for in_off, out_off in ((0, 0), (1, 1), (0, 1), (1, 0)):
            what = (words is CHIRP, in_off, out_off)
            big, out = guarded(ctx, n, out_off)
            o = osc(ctx, words, n0)
            o.mix(at_offset(ctx, x, in_off), out)
            assert o.position == n0 + n
            assert bits_equal(out.to_host(), want), what
            assert guards_intact(big, n, out_off), what
        for out_off in (0, 1):
            big, out = guarded(ctx, n, out_off)
            osc(ctx, words, n0).tone(n, AMP, out)
            assert bits_equal(out.to_host(), twant), (words is CHIRP, out_off)
            assert guards_intact(big, n, out_off), (words is CHIRP, out_off)


# ---- 2. stream positions ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n0", (0, 1, 2 ** 32 - 100, 2 ** 63 - 3, 2 ** 64 - 1 - 513), ids=("0", "1", "2^32-100", "2^63-3", "2^64-1-n"))
def test_stream_positions(ctx, n0):
    n = 513
    x = rand_c64(77, n)
    for words in (SHIFT, CHIRP):
        for off in (0, 1):
            xin = at_offset(ctx, x, off)
            assert bits_equal(osc(ctx, words, n0).mix(xin).to_host(), nco_truth.mix(words, n0, x)), (words is CHIRP, off)
        assert bits_equal(osc(ctx, words, n0).tone(n, AMP).to_host(), nco_truth.tone(words, n0, AMP, n))


# ---- 3. word sets -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(WORD_SETS))
def test_word_sets(ctx, name):
    words = WORD_SETS[name]
    n = 1027
    x = rand_c64(31, n)
    for n0 in (0, 2 ** 33 + 1):
        got = osc(ctx, words, n0).mix(ctx.vec(x)).to_host()
        assert bits_equal(got, nco_truth.mix(words, n0, x)), (name, n0)
        assert bits_equal(osc(ctx, words, n0).tone(n, AMP).to_host(), nco_truth.tone(words, n0, AMP, n)), (name, n0)
    if name == "zero":
        assert bits_equal(osc(ctx, words).tone(n, 1.0).to_host(), np.ones(n, np.complex64))
    if name == "alternate":
        assert bits_equal(osc(ctx, words).tone(4, 1.0).to_host(), np.array([1, complex(-1, -0.0), 1, complex(-1, -0.0)], np.complex64))


# ---- 4. chunks of a stream concatenate ---------------------------------------------------------------------------------------
def test_chunks_concatenate_and_in_place_equals_out_of_place(ctx):
    n, n0 = 1500, 2 ** 32 - 100
    x = rand_c64(5, n)
    xin = ctx.vec(x)
    for words in (SHIFT, CHIRP):
        whole = osc(ctx, words, n0).mix(xin).to_host()
        assert bits_equal(whole, nco_truth.mix(words, n0, x))
        twhole = osc(ctx, words, n0).tone(n, AMP).to_host()
        for cut in (1, 2, 255, 256, 257, 733):
            out = ctx.empty(n)
            o = osc(ctx, words, n0)
            o.mix(xin.slice(0, cut), out.slice(0, cut))                   # Nco.mix twice: the position carries over
            o.mix(xin.slice(cut, n), out.slice(cut, n))
            assert o.position == n0 + n
            assert bits_equal(out.to_host(), whole), (words is CHIRP, cut)
            o.seek(n0)
            o.tone(cut, AMP, out.slice(0, cut))
            o.tone(n - cut, AMP, out.slice(cut, n))
            assert bits_equal(out.to_host(), twhole), (words is CHIRP, cut)
        for off in (0, 1):                                                # in place, on both parities
            buf = at_offset(ctx, x, off)
            got = osc(ctx, words, n0).mix(buf, out=buf)
            assert got is buf and bits_equal(buf.to_host(), whole), (words is CHIRP, off)


# ---- 5. special data -----------------------------------------------------------------------------------------------------
def test_zeros_infinities_and_denormals(ctx):
    tiny = np.float32(1e-45)                                                # the smallest denormal
    vals = np.array([0.0, -0.0, np.inf, -np.inf, tiny, -tiny, np.float32(1.1e-38), 1.0, np.float32(3e38)], np.float32)
    re, im = np.meshgrid(vals, vals)
    x = np.empty(re.size, np.complex64)
    x.real, x.imag = re.reshape(-1), im.reshape(-1)                         # every pair of values, the signs of zero kept
    x = np.tile(x, 7)                                                       # 567 samples: every value meets several phasors
    for words in ((0, 1 << 62, 0), SHIFT, CHIRP):
        want = nco_truth.mix(words, 3, x)
        got = osc(ctx, words, 3).mix(ctx.vec(x)).to_host()
        assert np.isnan(want.view(np.float32)).any() or words[1] == 1 << 62
        assert nco_truth.same_bits(got, want), words
    for amp in (0.0, -0.0, np.inf, float(tiny)):
        want = nco_truth.tone((0, 1 << 62, 0), 0, amp, 8)                  # inf * 0 = NaN at the cardinal words
        assert nco_truth.same_bits(osc(ctx, (0, 1 << 62, 0)).tone(8, amp).to_host(), want), amp


# ---- 6. accuracy ------------------------------------------------------------------------------------------------------------
def test_accuracy_against_complex128(ctx):
    n, n0 = 4096, 2 ** 40 + 7
    x = rand_c64(9, n)
    for words in (SHIFT, CHIRP):
        truth = nco_truth.phasor_f64([nco_truth.word_int(words, n0 + i) for i in range(n)])
        got = osc(ctx, words, n0).mix(ctx.vec(x)).to_host().astype(np.complex128)
        want = x.astype(np.complex128) * truth
        e_mix = 20 * np.log10(np.linalg.norm(got - want) / np.linalg.norm(want))
        t = osc(ctx, words, n0).tone(n, 1.0).to_host().astype(np.complex128)
        e_tone = 20 * np.log10(np.linalg.norm(t - truth) / np.linalg.norm(truth))
        print(f"rate {'!=' if words[2] else '=='} 0: mix {e_mix:.1f} dB, tone {e_tone:.1f} dB")
        assert e_mix <= TOL_DB and e_tone <= TOL_DB, (e_mix, e_tone)


# ---- 7. reproducible, whatever the cache policy ---------------------------------------------------------------------------
REPRO = [(words, n, off) for words in (SHIFT, CHIRP) for n, off in ((1027, 0), (1028, 1))]


def _repro_bytes(ctx, case):
    words, n, off = case
    x = rand_c64(n, n)
    a = osc(ctx, words, 2 ** 33 + 5).mix(at_offset(ctx, x, off)).to_host().tobytes()           # 16-byte out, in at `off`: both routes
    big, out = guarded(ctx, n, off)
    osc(ctx, words, 2 ** 33 + 5).tone(n, AMP, out)
    return a + out.to_host().tobytes()


def _child(outdir):
    ctx = ap.Context(0)
    for nt in ("0", "1"):
        os.environ["AETH_NT"] = nt
        for i, case in enumerate(REPRO):
            with open(os.path.join(outdir, f"nt{nt}_{i}.bin"), "wb") as f:
                f.write(_repro_bytes(ctx, case))
    ctx.close()
    print("nco child ok")


def test_results_are_the_same_under_both_cache_policies(ctx, tmp_path):
    env = dict(os.environ, AETH_TUNING="1")
    env.pop("AETH_NT", None)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child", str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    for i, case in enumerate(REPRO):
        want = _repro_bytes(ctx, case)
        for nt in ("0", "1"):
            assert open(tmp_path / f"nt{nt}_{i}.bin", "rb").read() == want, f"AETH_NT={nt} changed the result of {case}"


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx):
    lib = _lib.load()
    n = 64
    sentinel = np.full(2 * n, 1.5 - 2.5j, np.complex64)
    x, out = ctx.vec(rand_c64(1, 2 * n)), ctx.vec(sentinel)
    X, O = x.ptr, out.ptr
    w = ap.nco._Words(*CHIRP)
    p = C.c_void_p

    def mix(c=ctx.h, ww=C.byref(w), n0=0, i=X, o=O, nn=n):
        return lib.aeth_nco_mix(c, ww, n0, p(i), p(o), nn)

    def tone(c=ctx.h, ww=C.byref(w), n0=0, o=O, nn=n):
        return lib.aeth_nco_tone(c, ww, n0, 1.0, p(o), nn)

    def err(rc, code, *words):
        msg = lib.aeth_last_error().decode()
        assert rc == code, (rc, msg)
        assert all(wd in msg for wd in words), msg

    err(mix(c=None), _lib.E_ARG, "ctx", "null")
    err(mix(ww=None), _lib.E_ARG, "words", "null")
    err(mix(i=None), _lib.E_ARG, "null")
    err(mix(o=None), _lib.E_ARG, "null")
    err(tone(o=None), _lib.E_ARG, "null")
    err(mix(i=X + 4), _lib.E_ALIGN, "8-byte aligned")
    err(mix(o=O + 4), _lib.E_ALIGN, "8-byte aligned")
    err(tone(o=O + 4), _lib.E_ALIGN, "8-byte aligned")
    # out == in runs in place; any other overlap is refused
    err(mix(i=O + 8, o=O), _lib.E_ARG, "overlaps")
    err(mix(i=O, o=O + 8 * (n - 1)), _lib.E_ARG, "overlaps")
    err(mix(i=O + 8 * (n - 1), o=O), _lib.E_ARG, "overlaps")
    # n0 <= 2^64 - 1 - n
    err(mix(n0=2 ** 64 - n + 1), _lib.E_UNSUPPORTED, str(2 ** 64 - n + 1), f"{n} samples")
    err(mix(n0=2 ** 64 - n), _lib.E_UNSUPPORTED, str(2 ** 64 - n), f"{n} samples")
    err(tone(n0=2 ** 64 - 1, nn=2), _lib.E_UNSUPPORTED, str(2 ** 64 - 1), "2 samples")
    # 2^31 workgroups: refused before any pointer is followed (16-byte route: 512 samples per workgroup, 8-byte: 256)
    err(lib.aeth_nco_mix(ctx.h, C.byref(w), 0, p(0x1000), p(2 ** 62), 2 ** 40), _lib.E_UNSUPPORTED, f"{2 ** 40} samples", "2^31 workgroups")
    err(lib.aeth_nco_mix(ctx.h, C.byref(w), 0, p(0x1008), p(2 ** 62), 2 ** 39), _lib.E_UNSUPPORTED, "2^31 workgroups")
    err(lib.aeth_nco_tone(ctx.h, C.byref(w), 0, 1.0, p(2 ** 62), 2 ** 40), _lib.E_UNSUPPORTED, "2^31 workgroups")
    assert mix(nn=0) == _lib.OK and tone(nn=0) == _lib.OK
    assert mix(i=None, o=None, nn=0) == _lib.OK and tone(o=None, nn=0) == _lib.OK
    ctx.sync()
    assert bits_equal(out.to_host(), sentinel)                       # nothing was launched
    # and the same arguments, made right, run: the last position that is served
    assert mix(n0=2 ** 64 - 1 - n) == _lib.OK
    ctx.sync()
    got = out.to_host()
    assert bits_equal(got[:n], nco_truth.mix(CHIRP, 2 ** 64 - 1 - n, x.to_host()[:n])) and bits_equal(got[n:], sentinel[n:])
    with pytest.raises(ap.LengthMismatch):
        osc(ctx, SHIFT).mix(x, out=ctx.empty(3))


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--child":
    _child(sys.argv[2])
