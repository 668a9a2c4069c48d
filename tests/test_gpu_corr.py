"""GPU: the streaming correlator (aeth_corr_exec, aeth_corr_exec_levels, aeth_corr_search) against what it is defined
as, from the same bytes the device sees.

    c[j] = sum_{k<M} conj(s[M-1-k]) * x[j-k]     (include/aether_hip.h)

Exact (bitwise): correlate against Fir(conj(ref[::-1])).filter; levels against correlate + DeviceVec.levels (NaN where
that has NaN, -inf where that has -inf); every peak record against DeviceVec.stats() of the matching slice of
correlate's output (max_index, max_norm, n_nan), the best record against the stats of the whole output; shards against
the unsharded run; one run against the next.

Tolerance (not measured on the code under test): correlate against numpy.correlate in complex128 at the suite's FIR
bound, -120 dB aggregate EVM (tests/test_gpu_fir.py: TOL_DB).

Every output lies between guard bands that are checked after every call."""
import ctypes as C
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
from aether_primitives_amd.corr import PEAK_DTYPE                          # noqa: E402
from helpers import bits_equal, rand_c64                                   # noqa: E402

pytestmark = pytest.mark.gpu
TOL_DB = -120.0
KINDS = (ap.LEVEL_NORM, ap.LEVEL_DB, ap.LEVEL_POWER_DB)
FUSED_LENGTHS = (1024, 2048, 4096)
M = 64
GUARD_F = np.float32(-7.25)
GUARD_C = np.complex64(complex(-7.25, 3.5))
GUARD_B = 0xA5
BIG = (1 << 24) + 3                                 # above 2^24 + 1; 8 and 12 B per sample pass the 128 MiB cache threshold


def template(seed=5, m=M):
    return rand_c64(seed, m)


def hop_of(fft_len, m=M):
    return ((fft_len - m + 1) // 64) * 64           # aeth_fir_create's rounding for fft_len >= 512


def sizes(fft_len):
    """n < hop, one sample, a multiple of the hop, a partial last block"""
    hop = hop_of(fft_len)
    return (hop - 5, 1, 3 * hop, 5 * hop + 37)


def stream(seed, n, hop, zeros=True):
    """random samples; with room for it, two blocks' worth of zeros in front so that a whole window is zero and its
    outputs are exactly 0 (level -inf)"""
    if n > (1 << 22):
        pat = rand_c64(seed, 1 << 20)
        x = np.tile(pat, (n + pat.size - 1) // pat.size)[:n].copy()
        x[::4099] *= 3                              # the repeats of the pattern are not all alike
    else:
        x = rand_c64(seed, n)
    if zeros and n >= 3 * hop:
        x[:2 * hop] = 0
    return x


# ---- guarded outputs -----------------------------------------------------------------------------------------------
def guarded_c64(ctx, n, front=3, back=7):
    buf = ctx.vec(np.full(front + n + back, GUARD_C, np.complex64))
    return buf, buf.slice(front, front + n), front


def guards_intact_c64(buf, n, front):
    h = buf.to_host().view(np.uint32).reshape(-1, 2)
    g = np.array([GUARD_C]).view(np.uint32)
    return bool((h[:front] == g).all() and (h[front + n:] == g).all())


def guarded_f32(ctx, n, front=3, back=9):
    buf = ap.DeviceF32(ctx, front + n + back)
    ctx.upload(buf.ptr, np.full(front + n + back, GUARD_F, np.float32))
    return buf, buf.slice(front, front + n), front


def guards_intact_f32(buf, n, front):
    h = buf.to_host()
    return bool((h[:front] == GUARD_F).all() and (h[front + n:] == GUARD_F).all())


def correlate_guarded(ctx, corr, x, hist=None):
    buf, out, front = guarded_c64(ctx, x.n)
    assert corr.correlate(x, out=out, hist=hist) is out
    assert guards_intact_c64(buf, x.n, front), "correlate wrote outside its output"
    return out


def levels_guarded(ctx, corr, x, kind, hist=None):
    buf, lv, front = guarded_f32(ctx, x.n)
    assert corr.levels(x, kind, out=lv, hist=hist) is lv
    h = buf.to_host()
    assert (h[:front] == GUARD_F).all() and (h[front + x.n:] == GUARD_F).all(), "levels wrote outside its output"
    return h[front:front + x.n]


def search_guarded(ctx, corr, x, hist=None, want_best=True, want_blocks=True):
    """aeth_corr_search with the records between two guard records: (best or None, records or None, raw record bytes)"""
    nb = corr.n_blocks(x.n)
    front, back = 2, 3
    host = np.full((front + nb + back) * 16, GUARD_B, np.uint8)
    dev = ctx.alloc(host.size)
    try:
        ctx.upload(dev, host)
        best = (C.c_char * 16)(*([GUARD_B] * 16))
        ap._lib.check(corr._lib.aeth_corr_search(corr.h, hist._p() if hist is not None else None, x._p(), x.n,
                                                 C.c_void_p(dev + front * 16) if want_blocks else None, nb if want_blocks else 0,
                                                 best if want_best else None))
        ctx.sync()
        ctx.download(dev, host)
    finally:
        ctx.free(dev)
    assert (host[:front * 16] == GUARD_B).all() and (host[(front + nb) * 16:] == GUARD_B).all(), "search wrote outside its records"
    raw = host[front * 16:(front + nb) * 16].copy()
    if not want_blocks:
        assert (raw == GUARD_B).all()
    if not want_best:
        assert bytes(best) == bytes([GUARD_B] * 16)
    b = np.frombuffer(bytes(best), PEAK_DTYPE)[0] if want_best else None
    return b, (raw.view(PEAK_DTYPE) if want_blocks else None), (raw.tobytes() if want_blocks else b"") + (bytes(best) if want_best else b"")


def f32_bits_equal(got, want):
    """bit-equal, NaN where the other has NaN"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    bad = got.view(np.uint32) != want.view(np.uint32)
    return got.shape == want.shape and not (bad & ~(np.isnan(got) & np.isnan(want))).any()


def same_record(rec, st, base, n_total):
    """a peak record against VecStats of the slice that starts at output `base`"""
    if st.max_index == st.n:                                        # no candidate in the slice
        return int(rec["index"]) == n_total and np.isnan(rec["norm"]) and int(rec["n_nan"]) == st.n_nan
    return (int(rec["index"]) == st.max_index + base and int(rec["n_nan"]) == st.n_nan
            and np.float32(rec["norm"]).view(np.uint32) == np.float32(st.max_norm).view(np.uint32))


def numpy_records(c, hop):
    """the records numpy derives from correlate's output (q in f64, argmax = lowest index of equals, NaN no candidate)"""
    n = c.size
    nb = -(-n // hop)
    re, im = c.real.astype(np.float64), c.imag.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        q = re * re + im * im
    pad = np.full(nb * hop, -1.0)
    nan = np.zeros(nb * hop, bool)
    nan[:n] = np.isnan(q)
    pad[:n] = np.where(nan[:n], -1.0, q)
    pad, nan = pad.reshape(nb, hop), nan.reshape(nb, hop)
    arg = pad.argmax(axis=1)
    top = pad[np.arange(nb), arg]
    out = np.empty(nb, PEAK_DTYPE)
    out["index"] = np.where(top < 0, n, arg + np.arange(nb) * hop)
    with np.errstate(invalid="ignore", over="ignore"):
        out["norm"] = np.where(top < 0, np.nan, np.sqrt(np.maximum(top, 0))).astype(np.float32)
    out["n_nan"] = nan.sum(axis=1)
    return out


def records_equal(a, b):
    return (a.size == b.size and (a["index"] == b["index"]).all() and (a["n_nan"] == b["n_nan"]).all()
            and f32_bits_equal(a["norm"], b["norm"]))


# ---- correlate ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fft_len,m", [(64, 16), (512, 64), (1024, 64), (2048, 64), (4096, 64), (2048, 1000)])
def test_correlate_is_the_fir_with_the_conj_reversed_template(ctx, fft_len, m):
    ref = template(fft_len, m)
    corr = ap.Corr(ctx, ref, fft_len)
    fir = ap.Fir(ctx, np.conj(ref[::-1]), fft_len)
    assert (corr.nref, corr.fft_len, corr.hop) == (m, fft_len, fir.hop)
    for n in (1, corr.hop - 1, 4 * corr.hop, 7 * corr.hop + 11):
        x = rand_c64(n + m, n + m - 1)
        d = ctx.vec(x)
        body, hist = d.slice(m - 1, d.n), d.slice(0, m - 1)
        assert bits_equal(correlate_guarded(ctx, corr, body).to_host(), fir.filter(body).to_host()), (fft_len, n)
        assert bits_equal(correlate_guarded(ctx, corr, body, hist).to_host(), fir.filter(body, hist=hist).to_host()), (fft_len, n, "hist")
        assert bits_equal(d.to_host(), x)


@pytest.mark.parametrize("fft_len", FUSED_LENGTHS)
def test_correlate_against_numpy(ctx, oracle, fft_len):
    ref = template(11)
    corr = ap.Corr(ctx, ref, fft_len)
    n = 6 * corr.hop + 101
    x = rand_c64(12, n + M - 1)
    d = ctx.vec(x)
    ref128 = ref.astype(np.complex128)
    # numpy: c_k = sum_i a[i + k] conj(v[i]), k from -(M-1): entry j of "full" is the causal c[j]
    truth0 = np.correlate(x[M - 1:].astype(np.complex128), ref128, "full")[:n]
    e0 = oracle.evm_db(correlate_guarded(ctx, corr, d.slice(M - 1, d.n)).to_host(), truth0)
    truth1 = np.correlate(x.astype(np.complex128), ref128, "full")[M - 1:M - 1 + n]
    e1 = oracle.evm_db(correlate_guarded(ctx, corr, d.slice(M - 1, d.n), d.slice(0, M - 1)).to_host(), truth1)
    print(f"fft_len {fft_len}: EVM {e0:.1f} dB without history, {e1:.1f} dB with")
    assert e0 <= TOL_DB and e1 <= TOL_DB, (e0, e1)


@pytest.mark.parametrize("fft_len", FUSED_LENGTHS)
def test_a_planted_template_peaks_at_its_offset_plus_m_minus_1(ctx, fft_len):
    ref = template(21)
    corr = ap.Corr(ctx, ref, fft_len)
    hop = corr.hop
    n = 9 * hop
    # inside a block, across a block boundary, at the very start, ending with the stream
    offsets = (0, 2 * hop - 30, 4 * hop + 500, 6 * hop - M + 1, n - M)
    x = rand_c64(22, n, scale=0.05)
    for p in offsets:
        x[p:p + M] += ref
    d = ctx.vec(x)
    mag = np.abs(correlate_guarded(ctx, corr, d).to_host())
    energy = float(np.sum(np.abs(ref.astype(np.complex128)) ** 2))
    for p in offsets:
        j = p + M - 1
        lo, hi = max(0, j - 200), min(n, j + 200)
        assert lo + int(mag[lo:hi].argmax()) == j and abs(mag[j] / energy - 1) < 0.1, (p, mag[j], energy)
    best, rec, _ = search_guarded(ctx, corr, d)
    hits = sorted(int(r["index"]) - (M - 1) for r in rec if r["norm"] > 0.6 * energy)
    assert hits == sorted(offsets), hits
    assert int(best["index"]) - (M - 1) in offsets
    # with history the lag can be negative: the template starts 10 samples before the body
    body, hist = d.slice(2 * hop - 30 + 10, n), d.slice(2 * hop - 30 + 10 - (M - 1), 2 * hop - 30 + 10)
    b = corr.search(body, hist=hist, blocks=False)
    first = corr.search(body.slice(0, hop), hist=hist)
    assert first.lag == -10 and first.index == M - 1 - 10, first
    assert b.lag + (2 * hop - 30 + 10) in offsets


# ---- levels -----------------------------------------------------------------------------------------------------------
def _levels_case(ctx, corr, x, what):
    """every kind, without and with history: the fused call against correlate + vec_levels"""
    m = corr.nref
    d = ctx.vec(x)
    body, hist = d.slice(m - 1, d.n), d.slice(0, m - 1)
    seen_inf = seen_nan = False
    for h in (None, hist):
        c = correlate_guarded(ctx, corr, body, h)
        for kind in KINDS:
            want = c.levels(kind).to_host()
            got = levels_guarded(ctx, corr, body, kind, h)
            assert f32_bits_equal(got, want), (what, kind, h is not None, np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))[:5])
            seen_inf |= bool(np.isneginf(got).any())
            seen_nan |= bool(np.isnan(got).any())
    assert bits_equal(d.to_host(), x), (what, "the input changed")
    return seen_inf, seen_nan


@pytest.mark.parametrize("fft_len", FUSED_LENGTHS)
def test_levels_equal_correlate_then_vec_levels(ctx, fft_len):
    corr = ap.Corr(ctx, template(31), fft_len)
    hop = corr.hop
    for n in sizes(fft_len):
        x = stream(32 + n, n + M - 1, hop)
        inf, _ = _levels_case(ctx, corr, x, f"fft_len={fft_len} n={n}")
        if n >= 3 * hop:
            assert inf, "a window of zeros gives outputs that are exactly 0: level -inf in the dB kinds"
    # a NaN component in one sample: every block whose window holds it is NaN, the others are not
    n = 5 * hop + 37
    x = stream(33, n + M - 1, hop)
    x[M - 1 + 3 * hop + 17] = complex(1.0, np.nan)
    _, nan = _levels_case(ctx, corr, x, f"fft_len={fft_len} NaN")
    assert nan


@pytest.mark.parametrize("fft_len", FUSED_LENGTHS)
def test_levels_equal_correlate_then_vec_levels_beyond_the_cache(ctx, fft_len):
    """more than 2^24 + 1 samples: the non-temporal builds, and block indices that need more than 13 bits"""
    corr = ap.Corr(ctx, template(41), fft_len)
    x = stream(42, BIG + M - 1, corr.hop)
    x[M - 1 + BIG // 2] = complex(np.nan, 0.0)
    inf, nan = _levels_case(ctx, corr, x, f"fft_len={fft_len} n={BIG}")
    assert inf and nan


# ---- search -----------------------------------------------------------------------------------------------------------
def _search_case(ctx, corr, d, hist, what, every_block=True):
    n, hop = d.n, corr.hop
    c = correlate_guarded(ctx, corr, d, hist)
    best, rec, raw = search_guarded(ctx, corr, d, hist)
    nb = corr.n_blocks(n)
    assert rec.size == nb
    # all blocks against numpy on the downloaded output, the listed ones against DeviceVec.stats() of the slice
    assert records_equal(rec, numpy_records(c.to_host(), hop)), what
    blocks = range(nb) if every_block else sorted({0, 1, nb // 3, nb // 2, nb - 2, nb - 1})
    for b in blocks:
        lo, hi = b * hop, min((b + 1) * hop, n)
        assert same_record(rec[b], c.slice(lo, hi).stats(), lo, n), (what, b, rec[b], c.slice(lo, hi).stats())
    assert same_record(best, c.stats(), 0, n), (what, best, c.stats())
    # either output alone gives the same bytes
    assert search_guarded(ctx, corr, d, hist, want_best=False)[2] == raw[:nb * 16], what
    assert search_guarded(ctx, corr, d, hist, want_blocks=False)[2] == raw[nb * 16:], what
    return best, rec, raw


@pytest.mark.parametrize("fft_len", FUSED_LENGTHS)
def test_search_records_equal_the_stats_of_correlates_output(ctx, fft_len):
    corr = ap.Corr(ctx, template(51), fft_len)
    for n in sizes(fft_len):
        x = stream(52 + n, n + M - 1, corr.hop, zeros=False)
        d = ctx.vec(x)
        for hist in (None, d.slice(0, M - 1)):
            _search_case(ctx, corr, d.slice(M - 1, d.n), hist, f"fft_len={fft_len} n={n} hist={hist is not None}")
        assert bits_equal(d.to_host(), x)


@pytest.mark.parametrize("fft_len", FUSED_LENGTHS)
def test_search_beyond_the_cache(ctx, fft_len):
    corr = ap.Corr(ctx, template(61), fft_len)
    x = stream(62, BIG, corr.hop)
    x[BIG - 5] = 4000 - 900j                                            # the strongest sample sits in the ragged last block
    d = ctx.vec(x)
    best, rec, raw = _search_case(ctx, corr, d, None, f"fft_len={fft_len} n={BIG}", every_block=False)
    assert int(best["index"]) >= BIG - 5
    # the zeros in front: every sample of block 0 ties at q = 0, the first one is reported
    assert int(rec[0]["index"]) == 0 and rec[0]["norm"] == 0
    assert search_guarded(ctx, corr, d, None)[2] == raw, "two runs differ"
    ctx.trim()                                                      # the slab is released and grown again
    assert search_guarded(ctx, corr, d, None)[2] == raw


@pytest.mark.parametrize("fft_len", FUSED_LENGTHS)
def test_search_ties_go_to_the_lowest_index(ctx, fft_len):
    corr = ap.Corr(ctx, template(71), fft_len)
    hop = corr.hop
    n = 6 * hop + 100
    d = ctx.vec(np.zeros(n, np.complex64))
    best, rec, _ = search_guarded(ctx, corr, d)
    assert (rec["index"] == np.arange(rec.size) * hop).all() and (rec["norm"] == 0).all() and (rec["n_nan"] == 0).all(), rec
    assert (int(best["index"]), float(best["norm"]), int(best["n_nan"])) == (0, 0.0, 0)
    _search_case(ctx, corr, d, None, f"zeros fft_len={fft_len}")


@pytest.mark.parametrize("fft_len", FUSED_LENGTHS)
def test_search_counts_and_skips_nan(ctx, fft_len):
    corr = ap.Corr(ctx, template(81), fft_len)
    hop = corr.hop
    n = 7 * hop + 300
    x = rand_c64(82, n)
    d = ctx.vec(x)
    _, clean, _ = search_guarded(ctx, corr, d)
    x[3 * hop + 40] = complex(np.nan, 2.0)
    d = ctx.vec(x)
    c = correlate_guarded(ctx, corr, d).to_host()
    best, rec, raw = _search_case(ctx, corr, d, None, f"NaN fft_len={fft_len}")
    all_nan = [bool(np.isnan(c[b * hop:min((b + 1) * hop, n)].real + c[b * hop:min((b + 1) * hop, n)].imag).all()) for b in range(rec.size)]
    assert any(all_nan) and not all(all_nan)
    for b, gone in enumerate(all_nan):
        if gone:                                                    # the sentinel, exactly where correlate's output is all NaN
            assert int(rec[b]["index"]) == n and np.isnan(rec[b]["norm"]) and int(rec[b]["n_nan"]) == min(hop, n - b * hop), rec[b]
        else:                                                       # a block the NaN does not reach is untouched
            assert rec[b].tobytes() == clean[b].tobytes(), (b, rec[b], clean[b])
    assert int(best["n_nan"]) == int(rec["n_nan"].sum()) and int(best["index"]) < n
    assert search_guarded(ctx, corr, d)[2] == raw, "two runs differ"
    # nothing but NaN: the best record is the sentinel too
    d = ctx.vec(np.full(2 * hop + 5, complex(np.nan, np.nan), np.complex64))
    best, rec, _ = search_guarded(ctx, corr, d)
    assert int(best["index"]) == d.n and np.isnan(best["norm"]) and int(best["n_nan"]) == d.n
    assert (rec["index"] == d.n).all() and np.isnan(rec["norm"]).all()


# ---- sharding ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fft_len", FUSED_LENGTHS)
def test_shards_cut_at_a_hop_concatenate_to_the_unsharded_result(ctx, fft_len):
    corr = ap.Corr(ctx, template(91), fft_len)
    hop = corr.hop
    n = 9 * hop + 77
    x = rand_c64(92, n)
    x[5 * hop - 3] = 30                                             # a peak whose response straddles the cut below
    d = ctx.vec(x)
    _, whole, _ = search_guarded(ctx, corr, d)
    for cut in (hop, 5 * hop):
        a, b = d.slice(0, cut), d.slice(cut, n)
        hist = d.slice(cut - (M - 1), cut)
        for kind in KINDS:
            parts = np.concatenate([levels_guarded(ctx, corr, a, kind), levels_guarded(ctx, corr, b, kind, hist)])
            assert f32_bits_equal(parts, levels_guarded(ctx, corr, d, kind)) and not np.isnan(parts).any(), (cut, kind)
        _, ra, _ = search_guarded(ctx, corr, a)
        _, rb, _ = search_guarded(ctx, corr, b, hist)
        rb = rb.copy()
        rb["index"] += cut                                          # a shard reports indices of its own stream
        assert records_equal(np.concatenate([ra, rb]), whole), cut


# ---- arguments on a real correlator ---------------------------------------------------------------------------------
def test_lengths_without_a_fused_build_are_refused(ctx):
    corr = ap.Corr(ctx, template(95, 16), 512)
    d = ctx.vec(rand_c64(96, 3000))
    assert corr.correlate(d).n == 3000
    with pytest.raises(ap.AetherError, match="fft_len 512") as e:
        corr.levels(d)
    assert e.value.code == ap._lib.E_UNSUPPORTED
    with pytest.raises(ap.AetherError, match="fft_len 512"):
        corr.search(d)
    good = ap.Corr(ctx, template(97), 2048)
    with pytest.raises(ap.LengthMismatch):
        good.levels(d, out=ap.DeviceF32(ctx, 2999))
    with pytest.raises(ap.AetherError, match="overlaps"):
        good.levels(d, out=ap.DeviceF32(ctx, 3000, ptr=d.ptr, offset=8))
    with pytest.raises(ap.AetherError, match="in place"):
        good.correlate(d, out=d)
    with pytest.raises(ap.AetherError, match="2\\*nref"):
        ap.Corr(ctx, template(98, 600), 1024)


# ---- the example ------------------------------------------------------------------------------------------------------
def test_sync_example_reports_every_planted_offset(ctx):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "examples", "sync.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    m = re.search(r"^hits:(.*)$", r.stdout, re.M)
    assert m, r.stdout
    assert [int(v) for v in m.group(1).split()] == [1000, 300000, 777777, 1040000], r.stdout
