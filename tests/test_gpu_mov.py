"""GPU: the moving-window detectors (include/aether_hip.h, aeth_mov_*) against the numpy restatement of their order
(tests/mov_truth.py, itself checked against math.fsum in tests/test_mov_truth.py).

  1. planes, bit for bit (a NaN matches any NaN): the shapes of the CPU test and every size around the kernel's chunk of
     1024 outputs, with and without history, both kinds; the terms at W = 1 for every pair of special values.
  2. every subset of the planes gives the bytes of all three together.
  3. both 8-byte parities of x, odd elements of r and m, sentinels around every output.
  4. reproducibility: twice, after aeth_ctx_trim, under both cache policies (a child process).
  5. a stream cut at the grid continues bit for bit, the first cut shorter than the history.
  6. search against exec: the host's argmax and first crossing over the m plane under the candidate rule, the f64 sums at
     the index, the fold of the records, blocks of zeros, NaN samples, an all-equal metric."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if __name__ == "__main__":
    sys.path[:0] = [ROOT, HERE]

import aether_primitives_amd as ap                    # noqa: E402
from aether_primitives_amd import mov                 # noqa: E402
from aether_primitives_amd.context import DeviceF32   # noqa: E402
import mov_truth as mt                                # noqa: E402

pytestmark = pytest.mark.gpu

LAG, POWER = mov.LAG, mov.POWER
SHAPES = ((1, 1, 50), (2, 1, 65), (16, 16, 400), (63, 5, 300), (64, 64, 700), (65, 1, 500), (144, 2048, 3000), (1000, 16, 4200),
          (4096, 64, 9000))
PLANES = ("p", "r", "m")


def burst_input(n, seed):
    """the first third scaled by 3e9, the rest by 1e-3 (the input of tests/test_mov_truth.py)"""
    r = np.random.default_rng(seed)
    x = r.standard_normal(n) + 1j * r.standard_normal(n)
    x[: n // 3] *= 3e9
    x[n // 3:] *= 1e-3
    return x.astype(np.complex64)


def signal(n, seed):
    r = np.random.default_rng(seed)
    return ((r.standard_normal(n) + 1j * r.standard_normal(n)) * 0.7).astype(np.complex64)


def at_offset(ctx, x, off):
    """x on the device, `off` samples behind a 16-byte boundary -> (DeviceVec view, owner)"""
    buf = np.zeros(x.size + off, np.complex64)
    buf[off:] = x
    d = ctx.vec(buf)
    return d.slice(off, off + x.size), d


def run(ctx, x, kind, W, L=0, hist=None, want=PLANES):
    """the planes on the host, in the order p, r, m (None where not asked for or where the kind has none)"""
    if kind == POWER:
        want = tuple(w for w in want if w != "p")
    out = mov.exec(ctx, x, kind, W, L, hist, want)
    return tuple(out[k].to_host() if k in out else None for k in PLANES)


def same_planes(got, want, what):
    for name, g, w in zip(PLANES, got, want):
        assert (g is None) == (w is None), (what, name)
        assert g is None or mt.same_bits(g, w), (what, name, int((g.view(np.uint32) != w.view(np.uint32)).sum()))


# ---- 1: planes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,L,n", SHAPES)
def test_planes_of_the_truth_shapes(ctx, W, L, n):
    x = burst_input(n, 1000 + W)
    hist = burst_input(mt.history(LAG, W, L), 7)[::-1].copy()
    for h in (None, hist):
        same_planes(run(ctx, x, LAG, W, L, h), mt.planes(x, LAG, W, L, h)[:3], (W, L, n, h is not None, PLANES))


@pytest.mark.parametrize("W,L", ((16, 64), (144, 2048)))
def test_planes_at_every_size_around_the_chunk(ctx, W, L):
    big = signal(100003, 3 + W)
    hist = signal(mt.history(LAG, W, L), 4 + W)
    for n in (1, W - 1, W, W + 1, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097, 3 * 4096 + 17, 100003):
        x = big[:n]
        for h in (None, hist):
            same_planes(run(ctx, x, LAG, W, L, h), mt.planes(x, LAG, W, L, h)[:3], (W, L, n, h is not None, PLANES))


@pytest.mark.parametrize("W", (1, 64, 1000))
def test_planes_of_the_power_kind(ctx, W):
    for n in (1, 50, 1025, 3 * 4096 + 17):
        x = burst_input(n, 20 + W)
        hist = signal(W - 1, 21)
        for h in (None, hist):
            same_planes(run(ctx, x, POWER, W, 0, h), mt.planes(x, POWER, W, 0, h)[:3], (W, n, h is not None, ("r", "m")))


def test_terms_of_every_pair_of_special_values(ctx):
    v = np.array([0.0, -0.0, 1e-40, -1e-42, 1.0, 3e9, np.inf, -np.inf, np.nan], np.float32)
    x = np.empty(v.size ** 2, np.complex64)
    x.real, x.imag = np.repeat(v, v.size), np.tile(v, v.size)
    for hist in (np.array([-0.0 - 1j], np.complex64), np.array([3e9 + 1e-40j], np.complex64), None):
        got, want = run(ctx, x, LAG, 1, 1, hist), mt.planes(x, LAG, 1, 1, hist)
        same_planes(got, want[:3], ("specials", hist, PLANES))
    same_planes(run(ctx, x, LAG, 1, 7, None), mt.planes(x, LAG, 1, 7, None)[:3], ("specials among themselves", PLANES))
    same_planes(run(ctx, x, POWER, 1), mt.planes(x, POWER, 1)[:3], ("specials, power", ("r", "m")))


# ---- 2: subsets ----------------------------------------------------------------------------------------------------
def test_every_subset_of_the_planes_gives_the_same_bytes(ctx):
    n = 3 * 4096 + 17
    x = ctx.vec(burst_input(n, 5))
    for kind, W, L, names in ((LAG, 144, 2048, PLANES), (LAG, 16, 16, PLANES), (POWER, 1000, 0, ("r", "m"))):
        full = run(ctx, x, kind, W, L)
        for mask in range(1, 2 ** len(names)):
            want = tuple(nm for j, nm in enumerate(names) if mask >> j & 1)
            got = run(ctx, x, kind, W, L, None, want)
            for nm, g, f in zip(PLANES, got, full):
                assert (g is None) == (nm not in want), (kind, want, nm)
                assert g is None or g.tobytes() == f.tobytes(), (kind, want, nm)


# ---- 3: alignment and sentinels ------------------------------------------------------------------------------------
def test_alignment_and_sentinels(ctx):
    n, W, L, pad = 4096 + 333, 63, 5, 3
    x = burst_input(n, 9)
    hist = signal(mt.history(LAG, W, L), 10)
    want = mt.planes(x, LAG, W, L, hist)
    views = [at_offset(ctx, x, off) for off in (0, 1)]
    hviews = [at_offset(ctx, hist, off) for off in (0, 1)]
    for off in (0, 1):
        for shift in (0, 1):                                        # r and m at even and odd elements, p at both parities
            pb = ctx.vec(np.full(n + 2 * pad + shift, np.complex64(7 - 7j)))
            rb, mb = DeviceF32(ctx, n + 2 * pad + shift), DeviceF32(ctx, n + 2 * pad + shift)
            fill = np.full(n + 2 * pad + shift, np.float32(-123.5))
            ctx.upload(rb.ptr, fill)
            ctx.upload(mb.ptr, fill)
            lo = pad + shift
            mov.exec_into(ctx, views[off][0], LAG, W, L, hviews[1 - off][0], pb.slice(lo, lo + n), rb.slice(lo, lo + n), mb.slice(lo, lo + n))
            for name, buf, w, sent in (("p", pb.to_host(), want[0], np.complex64(7 - 7j)), ("r", rb.to_host(), want[1], np.float32(-123.5)),
                                       ("m", mb.to_host(), want[2], np.float32(-123.5))):
                assert mt.same_bits(buf[lo:lo + n], w), (off, shift, name)
                assert (buf[:lo] == sent).all() and (buf[lo + n:] == sent).all(), (off, shift, name, "sentinel")


# ---- 4: reproducibility --------------------------------------------------------------------------------------------
def repro_calls(ctx):
    """the planes and records of a fixed set of calls as bytes"""
    n = 3 * 4096 + 17
    x = ctx.vec(burst_input(n, 77))
    b = b""
    for kind, W, L in ((LAG, 16, 64), (LAG, 144, 2048), (LAG, 4096, 1), (POWER, 1000, 0)):
        hist = ctx.vec(signal(mt.history(kind, W, L), 78))
        b += b"".join(p.tobytes() for p in run(ctx, x, kind, W, L, hist) if p is not None)
        rec, best = mov.search(ctx, x, kind, W, L, 1e-9, 0.5, hist, 1000)
        b += rec.tobytes() + bytes(best)
    return b


def test_same_bytes_twice_and_after_trim(ctx):
    a = repro_calls(ctx)
    assert repro_calls(ctx) == a, "the same calls gave other bytes"
    ctx.trim()                                                       # the slab is released and grown again
    assert repro_calls(ctx) == a


def _child(outdir):
    ctx = ap.Context(0)
    for nt in ("0", "1"):
        os.environ["AETH_NT"] = nt
        with open(os.path.join(outdir, f"nt{nt}.bin"), "wb") as f:
            f.write(repro_calls(ctx))
    ctx.close()
    print("mov child ok")


def test_bytes_do_not_depend_on_the_cache_policy(ctx, tmp_path):
    """AETH_TUNING=1 with AETH_NT=0 and AETH_NT=1 in a child process: the bytes of this process"""
    env = dict(os.environ, AETH_TUNING="1")
    env.pop("AETH_NT", None)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child", str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    want = repro_calls(ctx)
    for nt in ("0", "1"):
        assert open(tmp_path / f"nt{nt}.bin", "rb").read() == want, f"AETH_NT={nt} changed the bytes"


# ---- 5: cuts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,W,L", ((LAG, 16, 64), (LAG, 144, 2048), (LAG, 1000, 16), (POWER, 33, 0), (POWER, 1000, 0)))
def test_a_stream_cut_at_the_grid_continues_bit_for_bit(ctx, kind, W, L):
    n = 3 * 4096 + 17
    x = burst_input(n, 31 + W)
    xd = ctx.vec(x)
    G, H = mov.grid(kind, W), mov.history(kind, W, L)
    assert 1 <= G <= 4096
    whole = run(ctx, xd, kind, W, L)
    for cut in sorted({G, 2 * G, (n - 1) // G * G}):                # the first one is shorter than the lag kinds' history
        if cut >= H:
            hist = xd.slice(cut - H, cut)
        else:
            hist = ctx.vec(np.concatenate([np.zeros(H - cut, np.complex64), x[:cut]]))
        a, b = run(ctx, xd.slice(0, cut), kind, W, L), run(ctx, xd.slice(cut, n), kind, W, L, hist if H else None)
        for name, pa, pb, pw in zip(PLANES, a, b, whole):
            assert pw is None or np.concatenate([pa, pb]).tobytes() == pw.tobytes(), (cut, name)


# ---- 6: search -----------------------------------------------------------------------------------------------------
BLOCKS = (0, 1, 7, 64, 4096, 4097)


def check_search(ctx, x, kind, W, L, hist, r_min, threshold, what):
    n = len(x)
    xd = ctx.vec(x)
    hd = ctx.vec(hist) if hist is not None else None
    p, r, m = run(ctx, xd, kind, W, L, hd)
    s = mt.sums(x, kind, W, L, hist)                                 # the f64 sums (the planes above are their roundings: test 1)
    for block in BLOCKS:
        peaks = mov.DevicePeaks(ctx, mov.n_blocks(n, block))
        best = mov.search_into(ctx, xd, kind, W, L, r_min, threshold, peaks, hd, block, best=True)
        rec = peaks.to_host()
        want = mt.records(m, s, kind, n, block, r_min, threshold)     # argmax and first crossing over the DEVICE's m plane
        for f in ("index", "first", "n_nan", "reserved"):
            assert (rec[f] == want[f]).all(), (what, block, f, np.flatnonzero(rec[f] != want[f])[:5])
        for f in ("p_re", "p_im", "r", "r_lag", "metric"):
            assert mt.same_bits(rec[f], want[f]), (what, block, f)
        has = rec["index"] < n
        at = rec["index"][has].astype(np.int64)
        assert mt.same_bits(rec["r"][has].astype(np.float32), r[at]) and mt.same_bits(rec["metric"][has], m[at]), (what, block)
        if kind == LAG:
            assert mt.same_bits(rec["p_re"][has].astype(np.float32), p.real[at]) and mt.same_bits(rec["p_im"][has].astype(np.float32), p.imag[at])
        fold = mt.fold_records(rec, n)
        got = np.frombuffer(bytes(best), mt.PEAK_DTYPE)[0]
        for f in ("index", "first", "n_nan", "reserved"):
            assert got[f] == fold[f], (what, block, f, got[f], fold[f])
        for f in ("p_re", "p_im", "r", "r_lag", "metric"):
            assert mt.same_bits(got[f], fold[f]), (what, block, f)
        only = mov.search_into(ctx, xd, kind, W, L, r_min, threshold, None, hd, block, best=True)      # no records kept
        assert bytes(only) == bytes(best), (what, block)
    return rec, best


def burst_in_zeros(n, start, half, reps, seed):
    x = np.zeros(n, np.complex64)
    h = signal(half, seed)
    x[start:start + reps * half] = np.tile(h, reps)
    return x


@pytest.mark.parametrize("W,L", ((64, 64), (16, 100), (1000, 16)))
def test_search_finds_what_a_host_finds_in_the_planes(ctx, W, L):
    n, start = 3 * 4096 + 17, 5000
    x = burst_in_zeros(n, start, L, 2 + 2 * W // L + 1500 // L, 60 + W)
    s = mt.sums(x, LAG, W, L)
    inside = np.arange(n)
    full = (inside >= start + W - 1 + L) & (inside < start + L * (2 + 2 * W // L + 1500 // L))
    r_min = 0.5 * min(s["r"][full].min(), s["r_lag"][full].min())     # exact zeros around the burst: the gate is unambiguous
    rec, best = check_search(ctx, x, LAG, W, L, None, r_min, 0.75, (W, L))
    assert start <= best.first <= best.index < n and best.metric > 0.99 and best.n_nan == 0
    # a block of zeros has no candidate
    peaks, _ = mov.search(ctx, x, LAG, W, L, r_min, 0.75, None, 64)
    assert peaks[0]["index"] == n and peaks[0]["first"] == n and np.isnan(peaks[0]["metric"]) and peaks[0]["r"] == 0.0
    assert not np.signbit(peaks[0]["p_re"]) and not np.signbit(peaks[0]["r_lag"])


def test_search_of_the_power_kind(ctx):
    n = 3 * 4096 + 17
    x = burst_in_zeros(n, 3000, 700, 3, 5)
    check_search(ctx, x, POWER, 64, 0, None, 1e-3, 0.4, "power")
    check_search(ctx, burst_input(n, 6), POWER, 1000, 0, signal(999, 7), 0.0, 1.0, "power with history")


def test_nan_samples_are_counted_and_never_win(ctx):
    n, W, L = 3 * 4096 + 17, 32, 32
    x = signal(n, 8)
    x[4000:4064] = x[4000 - 32:4032]                                  # a repeated stretch: a peak
    x[[100, 7000, 7001]] = np.nan
    x[9000] = np.complex64(complex(np.inf, 1))
    rec, best = check_search(ctx, x, LAG, W, L, signal(63, 9), 0.0, 0.9, "nan")
    m = mt.planes(x, LAG, W, L, signal(63, 9))[2]
    assert best.n_nan == int(np.isnan(m).sum()) > 3 * W and best.index < n and not np.isnan(best.metric)


def test_an_all_equal_metric_returns_index_zero(ctx):
    n, W, L = 4096 + 100, 16, 16
    ones = np.ones(n, np.complex64)
    rec, best = mov.search(ctx, ones, LAG, W, L, 1.0, 0.5, np.ones(mov.history(LAG, W, L), np.complex64), 1000)
    assert best.index == 0 and best.first == 0 and best.metric == 1.0 and best.p_re == 16.0 and best.r == 16.0 and best.r_lag == 16.0
    assert list(rec["index"]) == [0, 1000, 2000, 3000, 4000] and list(rec["first"]) == [0, 1000, 2000, 3000, 4000]


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        _child(sys.argv[2])
