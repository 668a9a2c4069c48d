"""GPU: the synchronisation estimators (include/aether_hip.h, aeth_sync_*) against the numpy restatement of their terms
(tests/sync_truth.py).

  1. terms, bit for bit: with block = 1 every record is one term; random samples and the specials (+-0, denormals, 1,
     3e9 -- which overflows under POW8 --, +-inf, NaN in either component), every kind with and without words, every
     power with lags 1 and 5 with and without history.
  2. sums: each component within n_b * 2^-52 * sum|t_i| of math.fsum over the restated terms of the block, mass within
     n_b * 2^-52 relative, n exact.  That is the bound tests/test_gpu_stats_levels.py derives for ANY order of f64
     additions (n_b - 1 additions, each within 2^-53 relative of a partial sum that never exceeds sum|t_i|, plus fsum's own
     rounding); an f32 accumulator misses it by eight orders of magnitude.
  3. closed forms in integer arithmetic: bitwise, whatever the order.
  4. reproducibility: twice, both alignments, both cache policies (a child process), a stream cut at a block boundary.
  5. guards: sentinels around rec_dev, total-only and records-only calls, records visible behind aeth_ctx_sync."""
import ctypes as C
import os
import subprocess
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if __name__ == "__main__":
    sys.path[:0] = [ROOT, HERE]

import aether_primitives_amd as ap                    # noqa: E402
from aether_primitives_amd import nco, sync           # noqa: E402
import sync_truth as st                               # noqa: E402

pytestmark = pytest.mark.gpu

C_ = sync.chunk()
WORDS = (0x0123_4567_89ab_cdef, nco.word(0.0371), nco.word(-2.5e-7))
N0 = 2 ** 41 + 12345
SIZES = (1, 2, 63, 64, 65, C_ - 1, C_, C_ + 1, 3 * C_ + 17, 100003)
BLOCKS = (0, 7, 64, C_, C_ + 1, 2 * C_ + 5)
LAGS = (1, 4, 1000, C_ + 3)
EPS = 2.0 ** -52


def signal(n, seed):
    r = np.random.default_rng(seed)
    return ((r.standard_normal(n) + 1j * r.standard_normal(n)) * r.uniform(0.5, 1.5, n) * 0.7).astype(np.complex64)


def at_offset(ctx, x, off):
    """x on the device, `off` samples behind a 16-byte boundary -> (DeviceVec view, owner)"""
    buf = np.zeros(x.size + off, np.complex64)
    buf[off:] = x
    d = ctx.vec(buf)
    return d.slice(off, off + x.size), d


def run_line(ctx, xd, kind, words, n0, block):
    rec = sync.DeviceRecords(ctx, sync.n_blocks(xd.n, block))
    tot = sync.line_into(ctx, xd, kind, rec, words, n0, block, total=True)
    return rec.to_host(), tot


def run_lag(ctx, xd, power, lag, hd, block):
    rec = sync.DeviceRecords(ctx, sync.n_blocks(xd.n, block))
    tot = sync.lag_into(ctx, xd, power, lag, rec, hd, block, total=True)
    return rec.to_host(), tot


# ---- 1: terms ------------------------------------------------------------------------------------------------------
def special_input():
    v = np.array([0.0, -0.0, 1e-40, -1e-42, 1.0, 3e9, np.inf, -np.inf, np.nan], np.float32)
    sp = np.empty(v.size ** 2, np.complex64)                              # every pair of components
    sp.real, sp.imag = np.repeat(v, v.size), np.tile(v, v.size)
    return np.concatenate([signal(257, 11), sp])


def check_terms(rec, t_re, t_im, wt, exists, what):
    e = exists
    assert (rec["n"] == e.astype(np.uint64)).all(), what
    assert (rec["reserved"] == 0).all(), what
    zero = np.zeros(int((~e).sum()))
    for name, t in (("re", t_re), ("im", t_im), ("mass", wt)):
        assert st.same_f64_bits(rec[name][e], t[e]), (what, name)
        assert st.same_f64_bits(rec[name][~e], zero), (what, name, "a record without terms is +0.0")
    assert (rec["n_nonfinite"][e] == st.nonfinite(t_re, t_im)[e]).all(), what
    assert (rec["n_nonfinite"][~e] == 0).all(), what


@pytest.mark.parametrize("kind", st.KINDS)
def test_line_terms_bit_for_bit(ctx, kind):
    x = special_input()
    xd = ctx.vec(x)
    for words, n0 in ((None, 0), (WORDS, N0), ((0, 0, 0), 7)):
        rec, _ = run_line(ctx, xd, kind, words, n0, 1)
        t_re, t_im, wt = st.line_terms(x, kind, words, n0)
        check_terms(rec, t_re, t_im, wt, np.ones(x.size, bool), (kind, words))


@pytest.mark.parametrize("lag", (1, 5))
@pytest.mark.parametrize("power", st.POWERS)
def test_lag_terms_bit_for_bit(ctx, power, lag):
    x = special_input()
    hist = x[40:40 + lag][::-1].copy()
    xd, hd = ctx.vec(x), ctx.vec(hist)
    for h, hdev in ((None, None), (hist, hd)):
        rec, _ = run_lag(ctx, xd, power, lag, hdev, 1)
        t_re, t_im, wt, exists = st.lag_terms(x, power, lag, h)
        check_terms(rec, t_re, t_im, wt, exists, (power, lag, h is not None))


# ---- 2: sums -------------------------------------------------------------------------------------------------------
def check_sums(rec, tot, want, mag, what):
    assert (rec["n"] == want["n"]).all(), what
    assert (rec["n_nonfinite"] == 0).all() and (rec["reserved"] == 0).all(), what
    nb = want["n"].astype(np.float64)
    for j, name in enumerate(("re", "im")):
        err, bound = np.abs(rec[name] - want[name]), nb * EPS * mag[:, j]
        assert (err <= bound).all(), (what, name, float((err / np.maximum(bound, 1e-300)).max()))
    assert (np.abs(rec["mass"] - want["mass"]) <= nb * EPS * want["mass"]).all(), (what, "mass")
    # the total: the sum of the block records under the same bound over all terms
    # (n_all terms in some order, against the fsum of the nb block references)
    n_all = float(want["n"].sum()) + want.size
    assert tot.n == int(want["n"].sum()) and tot.n_nonfinite == 0 and tot.reserved == 0, what
    for j, (name, got) in enumerate((("re", tot.re), ("im", tot.im))):
        assert abs(got - st.fsum(want[name])) <= n_all * EPS * mag[:, j].sum(), (what, name, "total")
    assert abs(tot.mass - st.fsum(want["mass"])) <= n_all * EPS * want["mass"].sum(), (what, "total mass")


@pytest.mark.parametrize("n", SIZES)
def test_line_sums(ctx, n):
    x = signal(n, 100 + n % 97)
    views = [at_offset(ctx, x, off) for off in (0, 1)]
    for i, block in enumerate(BLOCKS):
        kind = st.KINDS[(i + n) % len(st.KINDS)]
        words, n0 = ((WORDS, N0) if (i + n // 2) % 2 == 0 else (None, 0))
        want, mag = st.records(*st.line_terms(x, kind, words, n0), block)
        for off, (xd, _) in enumerate(views):
            rec, tot = run_line(ctx, xd, kind, words, n0, block)
            check_sums(rec, tot, want, mag, ("line", n, block, off, kind, words is not None))


@pytest.mark.parametrize("n", SIZES)
def test_lag_sums(ctx, n):
    x = signal(n, 200 + n % 89)
    views = [at_offset(ctx, x, off) for off in (0, 1)]
    j = n
    for lag in LAGS:
        hist = signal(lag, 300 + lag % 83)
        hviews = [at_offset(ctx, hist, off) for off in (0, 1)]
        for with_hist in (False, True):
            j += 1
            block, power, off = BLOCKS[j % len(BLOCKS)], st.POWERS[(j // 2) % 4], j % 2
            t_re, t_im, wt, exists = st.lag_terms(x, power, lag, hist if with_hist else None)
            want, mag = st.records(t_re, t_im, wt, block, exists)
            rec, tot = run_lag(ctx, views[off][0], power, lag, hviews[1 - off][0] if with_hist else None, block)
            check_sums(rec, tot, want, mag, ("lag", n, block, off, power, lag, with_hist))


def test_every_block_size_meets_every_lag(ctx):
    """the shapes the rotation of test_lag_sums leaves out at the size with several chunks per block"""
    n = 3 * C_ + 17
    x = signal(n, 5)
    xd = ctx.vec(x)
    for lag in LAGS:
        hist = signal(lag, 6)
        hd = ctx.vec(hist)
        for block in BLOCKS:
            for with_hist in (False, True):
                t_re, t_im, wt, exists = st.lag_terms(x, 2, lag, hist if with_hist else None)
                want, mag = st.records(t_re, t_im, wt, block, exists)
                rec, tot = run_lag(ctx, xd, 2, lag, hd if with_hist else None, block)
                check_sums(rec, tot, want, mag, ("lag", n, block, lag, with_hist))


# ---- 3: closed forms -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 65, C_ + 1, 3 * C_ + 17, 100003))
def test_exact_closed_forms(ctx, n):
    ones = ctx.vec(np.ones(n, np.complex64))
    for kind in st.KINDS:
        for block in (0, 7, C_ + 1):
            rec, tot = run_line(ctx, ones, kind, None, 0, block)
            assert (tot.re, tot.im, tot.mass, tot.n, tot.n_nonfinite) == (float(n), 0.0, float(n), n, 0), (kind, block)
            assert (rec["re"] == rec["n"]).all() and (rec["im"] == 0).all() and (rec["mass"] == rec["n"]).all() and rec["n"].sum() == n
    diag = ctx.vec(np.full(n, 1 + 1j, np.complex64))
    _, tot = run_line(ctx, diag, st.POW4, None, 0, 0)                     # (1 + j)^4 = -4
    assert (tot.re, tot.im, tot.mass, tot.n) == (-4.0 * n, 0.0, 16.0 * n, n)
    _, tot = run_line(ctx, diag, st.POW8, None, 0, 64)                    # (1 + j)^8 = 16
    assert (tot.re, tot.im, tot.mass, tot.n) == (16.0 * n, 0.0, 256.0 * n, n)
    for lag in (1, 4, 1000, C_ + 3):
        _, tot = run_lag(ctx, ones, 4, lag, None, 0)
        m = max(n - lag, 0)
        assert (tot.re, tot.im, tot.mass, tot.n) == (float(m), 0.0, float(m), m), lag
        if lag <= n:
            _, tot = run_lag(ctx, ones, 2, lag, ones.slice(0, lag), C_)
            assert (tot.re, tot.im, tot.mass, tot.n) == (float(n), 0.0, float(n), n), lag


@pytest.mark.parametrize("n", (4, 64, C_ + 4, 3 * C_ + 16, 100004))
def test_a_quarter_turn_step_cancels_a_constant(ctx, n):
    """step = 2^62: the phasors are exactly 1, j, -1, -j, so every four samples of a constant sum to (0, 0) exactly"""
    x = ctx.vec(np.full(n, 3 - 2j, np.complex64))
    for kind in (st.SQUARE, st.POW1, st.POW2):
        for block in (0, 4, C_):
            rec, tot = run_line(ctx, x, kind, (0, 1 << 62, 0), 0, block)
            assert tot.re == 0.0 and tot.im == 0.0 and tot.n == n, (kind, block, tot.re, tot.im)
            assert (rec["re"] == 0).all() and (rec["im"] == 0).all()


# ---- 4: reproducibility --------------------------------------------------------------------------------------------
REPRO_N = 3 * C_ + 17
REPRO_BLOCK = C_ + 1


def repro_calls(ctx):
    """the records and totals of a fixed set of calls as bytes"""
    x = signal(REPRO_N, 77)
    hist = signal(1000, 78)
    out = []
    for off in (0, 1):
        xd, _keep = at_offset(ctx, x, off)
        hd, _keep2 = at_offset(ctx, hist, 1 - off)
        b = b""
        for kind in st.KINDS:
            rec, tot = run_line(ctx, xd, kind, WORDS, N0, REPRO_BLOCK)
            b += rec.tobytes() + bytes(tot)
        rec, tot = run_line(ctx, xd, st.POW2, None, 0, 0)
        b += rec.tobytes() + bytes(tot)
        for power in st.POWERS:
            rec, tot = run_lag(ctx, xd, power, 1000, hd, REPRO_BLOCK)
            b += rec.tobytes() + bytes(tot)
        out.append(b)
    return out


def test_same_records_twice_and_at_both_alignments(ctx):
    a, b = repro_calls(ctx), repro_calls(ctx)
    assert a[0] == b[0] and a[1] == b[1], "the same call gave other records"
    assert a[0] == a[1], "the records depend on the pointer's alignment"
    ctx.trim()                                                       # the slab is released and grown again
    assert repro_calls(ctx)[0] == a[0]


def _child(outdir):
    ctx = ap.Context(0)
    for nt in ("0", "1"):
        os.environ["AETH_NT"] = nt
        with open(os.path.join(outdir, f"nt{nt}.bin"), "wb") as f:
            f.write(repro_calls(ctx)[0])
    ctx.close()
    print("sync child ok")


def test_records_do_not_depend_on_the_cache_policy(ctx, tmp_path):
    """AETH_TUNING=1 with AETH_NT=0 and AETH_NT=1 in a child process: the records of this process"""
    env = dict(os.environ, AETH_TUNING="1")
    env.pop("AETH_NT", None)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child", str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    want = repro_calls(ctx)[0]
    for nt in ("0", "1"):
        assert open(tmp_path / f"nt{nt}.bin", "rb").read() == want, f"AETH_NT={nt} changed the records"


@pytest.mark.parametrize("block", (64, C_, C_ + 1, 2 * C_ + 5))
def test_a_stream_cut_at_a_block_boundary_continues_bit_for_bit(ctx, block):
    n, cut = 4 * block + block // 3 + 1, 2 * block                   # five blocks, the last one short
    x = signal(n, 31)
    xd = ctx.vec(x)
    for kind in st.KINDS:
        whole, _ = run_line(ctx, xd, kind, WORDS, N0, block)
        a, _ = run_line(ctx, xd.slice(0, cut), kind, WORDS, N0, block)
        b, _ = run_line(ctx, xd.slice(cut, n), kind, WORDS, N0 + cut, block)
        assert whole.size == 5 and np.concatenate([a, b]).tobytes() == whole.tobytes(), ("line", kind)
    for power, lag in ((1, 1), (2, 4), (4, 1000), (8, C_ + 3), (4, 1)):
        if lag > cut:
            continue
        whole, _ = run_lag(ctx, xd, power, lag, None, block)
        a, _ = run_lag(ctx, xd.slice(0, cut), power, lag, None, block)
        b, _ = run_lag(ctx, xd.slice(cut, n), power, lag, xd.slice(cut - lag, cut), block)
        assert np.concatenate([a, b]).tobytes() == whole.tobytes(), ("lag", power, lag)


# ---- 5: guards -----------------------------------------------------------------------------------------------------
def test_sentinels_and_output_flavours(ctx):
    n, block = 3 * C_ + 17, 64
    nb = sync.n_blocks(n, block)
    x = signal(n, 41)
    xd = ctx.vec(x)
    size = sync.RECORD_DTYPE.itemsize
    for call in ("line", "lag"):
        buf = np.frombuffer(b"\x5a" * (size * (nb + 4)), sync.RECORD_DTYPE).copy()
        dev = ctx.alloc(buf.nbytes)
        try:
            ctx.upload(dev, buf)
            inner = types.SimpleNamespace(_p=lambda: C.c_void_p(dev + 2 * size))          # the records, two sentinels on either side
            # records only: no wait, the records are there behind aeth_ctx_sync
            if call == "line":
                assert sync.line_into(ctx, xd, st.POW4, inner, WORDS, N0, block) is None
                want, tot_want = run_line(ctx, xd, st.POW4, WORDS, N0, block)
                tot = sync.line_into(ctx, xd, st.POW4, None, WORDS, N0, block, total=True)       # total only
            else:
                assert sync.lag_into(ctx, xd, 4, 5, inner, None, block) is None
                want, tot_want = run_lag(ctx, xd, 4, 5, None, block)
                tot = sync.lag_into(ctx, xd, 4, 5, None, None, block, total=True)
            ctx.sync()
            ctx.download(dev, buf)
        finally:
            ctx.free(dev)
        assert buf[:2].tobytes() == b"\x5a" * (2 * size) == buf[-2:].tobytes(), call
        assert buf[2:-2].tobytes() == want.tobytes(), call
        assert bytes(tot) == bytes(tot_want), call


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        _child(sys.argv[2])
