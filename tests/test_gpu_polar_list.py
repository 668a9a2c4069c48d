"""GPU: aeth_polar_list_decode / aeth_polar_list_pick (include/aether_hip.h) against the restatement
tests/polar_list_truth.py, byte for byte and record for record; outputs lie between guard bytes that are checked unchanged.

  1. decode, per (code, L) -- (3, 4) at 1, 2, 4, 8; (3, 3) and (3, 8) at 8; (4, 8) at 1, 2, 4; (5, 16) at 1, 2, 4, 8; (6, 1)
     at 2; a 5-bit random mask with position 31 frozen at 4; (7, 64) random at 8; (9, 171) at 8; (10, 512) at 4 and 8;
     (10, 1023) at 2: between them they reach every (lanes, paths) the build contains -- the six kinds of input of
     tests/test_gpu_polar.py x flags 0, CODEWORD, ALL, ALL | CODEWORD at 3 G + 1 codewords; records NULL; F = 1, G - 1, G,
     G + 1 on the uniform input.
  2. soft pointer at byte offsets 0 .. 3 x output at 0 and 1.
  3. the same call twice; a call cut at a codeword equals two calls.
  4. L = 1 equals aeth_polar_decode on the device.
  5. on the device's ALL | CODEWORD output: the metric identity, ascending metrics, L distinct rows.
  6. pick: planted diff words (none, first, last, several zero), row_bytes 1, 7, 240, 1024, F around a workgroup's share of
     4096 output bytes, odd pointers, which NULL.
  7. refusals launch nothing."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import aether_primitives_amd as ap                    # noqa: E402
from aether_primitives_amd import _lib                # noqa: E402
import polar_truth as T                               # noqa: E402
import polar_list_truth as LT                         # noqa: E402
from test_gpu_polar import GUARD, KINDS, SENTINEL, Mem, group_counts     # noqa: E402

pytestmark = pytest.mark.gpu

BUILT = {(4, 1), (4, 2), (4, 4), (4, 8), (8, 1), (8, 2), (8, 4), (8, 8), (16, 1), (16, 2), (16, 4)}
PICK_BYTES = 4096                                      # output bytes a workgroup of the pick takes


def codes():
    c = dict(T.test_codes())
    c["3x3"] = (3, T.mask(3, 3))
    c["4x8"] = (4, T.mask(4, 8))
    m = T.random_mask(5, 14, 531)
    m[31] = 0
    c["5f31"] = (5, m)
    return c


CODES = codes()
CASES = (("3x4", 1), ("3x4", 2), ("3x4", 4), ("3x4", 8), ("3x3", 8), ("3x8", 8), ("4x8", 1), ("4x8", 2), ("4x8", 4), ("5x16", 1), ("5x16", 2),
         ("5x16", 4), ("5x16", 8), ("6x1", 2), ("5f31", 4), ("7x64r", 8), ("9x171", 8), ("10x512", 4), ("10x512", 8), ("10x1023", 2))
IDS = [f"{name}-L{L}" for name, L in CASES]
FLAGS = (0, LT.CODEWORD, LT.ALL, LT.ALL | LT.CODEWORD)
_TRUTH = {}


def soft_of(name, kind, F):
    """the first F codewords of the kind's input for this code (the six kinds of tests/test_gpu_polar.py)"""
    n, msk = CODES[name]
    N, K = 1 << n, int(msk.sum())
    key = ("soft", name, kind)
    if key not in _TRUTH or _TRUTH[key].size < F * N:
        rng = np.random.default_rng(len(name) * 1000 + N + KINDS.index(kind))
        if kind == "ties":
            s = rng.integers(-1, 2, F * N).astype(np.int8)
        elif kind == "zero":
            s = np.zeros(F * N, np.int8)
        elif kind == "uniform":
            s = rng.integers(-128, 128, F * N).astype(np.int8)
            s[::97] = -128
        elif kind == "max":
            s = np.full(F * N, 127, np.int8)
        elif kind == "min":
            s = np.full(F * N, -128, np.int8)
        else:
            s = T.noisy_soft(rng, T.encode(msk, rng.integers(0, 2, F * K, dtype=np.uint8)), 0.8, 24.0)
        _TRUTH[key] = s
    return _TRUTH[key][:F * N]


def truth_of(name, L, kind, F):
    """{flags: rows [F][per]} and records [F] of the restatement, computed once per (code, L, kind, F)"""
    n, msk = CODES[name]
    key = ("dec", name, L, kind, F)
    if key not in _TRUTH:
        soft = soft_of(name, kind, F)
        out = {}
        for flags in FLAGS:
            bits, rec = LT.decode(msk, soft, L, flags)
            out[flags] = bits.reshape(F, -1)
        _TRUTH[key] = (out, rec)
    return _TRUTH[key]


@pytest.fixture
def mem(ctx):
    m = Mem(ctx)
    yield m
    m.free()


@pytest.fixture(scope="module")
def objects(ctx):
    made = {}

    def get(name, L):
        if (name, L) not in made:
            made[name, L] = ap.PolarList(ctx, *CODES[name], L)
        return made[name, L]
    yield get
    for o in made.values():
        o.close()


def per_of(c, flags):
    return (c.paths if flags & LT.ALL else 1) * (c.n if flags & LT.CODEWORD else c.k)


def d_decode(mem, c, soft, flags=0, records=True, in_off=0, out_off=0):
    """-> (rows [F][per], records [F] or None) of one device call"""
    F = soft.size // c.n
    per = per_of(c, flags)
    o = mem.out(F * per, out_off)
    r = mem.out(F * 32, 4) if records else None
    _lib.check(c._lib.aeth_polar_list_decode(c.h, mem.inp(soft, in_off), soft.size, flags, mem.ptr(o), F * per, mem.ptr(r)))
    return mem.get(o).reshape(F, per), (mem.get(r).view(LT.LIST_RECORD) if records else None)


# ---- 1 -----------------------------------------------------------------------------------------------------------------
def test_getters_and_every_built_instance(objects):
    seen = set()
    for name, L in CASES:
        n, msk = CODES[name]
        c = objects(name, L)
        assert (c.n, c.k, c.paths) == (1 << n, int(msk.sum()), L)
        assert c.lanes in (4, 8, 16) and 2 * c.lanes <= c.n and c.group * c.lanes * L == 64
        assert c.lanes == max(t for t in (4, 8, 16) if t == 4 or (t * L <= 64 and 2 * t <= c.n))
        state = 2 * (c.n - 2 * c.lanes) + 4 * max(c.n // 32, 1) + 4
        slots = 64 // c.lanes
        assert c.lds_bytes % slots == 0 and state <= c.lds_bytes // slots < state + 128 and c.lds_bytes <= 65536
        seen.add((c.lanes, L))
    assert seen == BUILT, "a built (lanes, paths) that no case of this file reaches, or the reverse"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,L", CASES, ids=IDS)
def test_decode_against_the_restatement(objects, mem, name, L, kind):
    c = objects(name, L)
    F = 3 * c.group + 1
    soft = soft_of(name, kind, F)
    want, want_rec = truth_of(name, L, kind, F)
    for flags in FLAGS:
        rows, rec = d_decode(mem, c, soft, flags)
        assert rec.tobytes() == want_rec.tobytes(), (name, L, kind, flags, rec[0], want_rec[0])
        assert rows.tobytes() == want[flags].tobytes(), (name, L, kind, flags)
    mem.free()
    rows, rec = d_decode(mem, c, soft, LT.ALL, records=False)
    assert rec is None and rows.tobytes() == want[LT.ALL].tobytes()
    if kind == "uniform":
        for Fs in group_counts(c.group):
            for flags in (0, LT.ALL | LT.CODEWORD):
                rows, rec = d_decode(mem, c, soft[:Fs * c.n], flags)
                assert rec.tobytes() == want_rec[:Fs].tobytes() and rows.tobytes() == want[flags][:Fs].tobytes(), (name, L, Fs, flags)
            mem.free()


# ---- 2 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_off", (0, 1, 2, 3))
def test_any_byte_alignment(objects, mem, in_off):
    for name, L in (("5x16", 4), ("7x64r", 8)):
        c = objects(name, L)
        Fm = 3 * c.group + 1
        F = c.group + 1
        soft = soft_of(name, "uniform", Fm)[:F * c.n]
        want, want_rec = truth_of(name, L, "uniform", Fm)
        for out_off in (0, 1):
            for flags in (0, LT.ALL | LT.CODEWORD):
                rows, rec = d_decode(mem, c, soft, flags, True, in_off, out_off)
                assert rec.tobytes() == want_rec[:F].tobytes()
                assert rows.tobytes() == want[flags][:F].tobytes(), (name, in_off, out_off, flags)


# ---- 3 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,L", (("3x4", 2), ("5x16", 4), ("10x1023", 2)))
def test_same_bytes_twice_and_two_calls_equal_one(objects, mem, name, L):
    c = objects(name, L)
    G = c.group
    F = 3 * G + 1
    soft = soft_of(name, "noisy", F)
    one = d_decode(mem, c, soft, LT.ALL)
    again = d_decode(mem, c, soft, LT.ALL)
    assert one[0].tobytes() == again[0].tobytes() and one[1].tobytes() == again[1].tobytes()
    for cut in sorted({1, max(G - 1, 1), G, G + 1, F - 1}):
        a = d_decode(mem, c, soft[:cut * c.n], LT.ALL)
        b = d_decode(mem, c, soft[cut * c.n:], LT.ALL)
        assert a[0].tobytes() + b[0].tobytes() == one[0].tobytes() and a[1].tobytes() + b[1].tobytes() == one[1].tobytes(), cut
        mem.free()


# ---- 4 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("3x4", "4x8", "5x16", "9x171"))
def test_a_list_of_one_is_the_sc_decoder_on_the_device(ctx, objects, mem, name):
    c = objects(name, 1)
    sc = ap.Polar(ctx, *CODES[name])
    F = 3 * c.group + 1
    for kind in ("ties", "uniform", "noisy"):
        soft = soft_of(name, kind, F)
        for flags in (0, LT.CODEWORD):
            nb = c.n if flags else c.k
            o = mem.out(F * nb)
            _lib.check(sc._lib.aeth_polar_decode(sc.h, mem.inp(soft), soft.size, None, flags, mem.ptr(o), F * nb, None))
            for f in (flags, flags | LT.ALL):
                rows, rec = d_decode(mem, c, soft, f)
                assert rows.tobytes() == mem.get(o).tobytes(), (name, kind, f)
                assert (rec["metric"][:, 1:] == LT.NONE).all()
        mem.free()
    sc.close()


# ---- 5 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,L", (("3x3", 8), ("5f31", 4), ("7x64r", 8), ("10x512", 8), ("10x1023", 2)))
def test_metrics_of_the_devices_own_rows(objects, mem, name, L):
    c = objects(name, L)
    F = 3 * c.group + 1
    for kind in ("uniform", "noisy", "ties"):
        soft = soft_of(name, kind, F)
        rows, rec = d_decode(mem, c, soft, LT.ALL | LT.CODEWORD)
        rows = rows.reshape(F, L, c.n)
        metric = rec["metric"].astype(np.int64)
        assert (metric[:, L:] == LT.NONE).all() and (np.diff(metric[:, :L], axis=1) >= 0).all()
        for f in range(F):
            assert (LT.metric_of(soft[f * c.n:(f + 1) * c.n], rows[f]) == metric[f, :L]).all(), (name, kind, f)
            assert len({r.tobytes() for r in rows[f]}) == L, (name, kind, f)
        mem.free()


# ---- 6 -----------------------------------------------------------------------------------------------------------------
def planted(rng, F, L):
    """diff words per codeword in turn: none zero, the first, the last, several, all"""
    d = rng.integers(1, 1 << 63, (F, L), dtype=np.uint64)
    for f in range(F):
        how = f % 5
        if how == 1:
            d[f, 0] = 0
        elif how == 2:
            d[f, L - 1] = 0
        elif how == 3:
            d[f, rng.integers(0, L, 2)] = 0
        elif how == 4:
            d[f] = 0
    return d


@pytest.mark.parametrize("row_bytes", (1, 7, 240, 1024))
def test_pick(ctx, mem, row_bytes):
    lib = _lib.load()
    rng = np.random.default_rng(row_bytes)
    share = max(PICK_BYTES // row_bytes, 1)
    for L in (1, 2, 4, 8, 3):
        for F in sorted({1, 5, share - 1, share, share + 1, 2 * share + 3} - {0}):
            rows = rng.integers(0, 256, F * L * row_bytes, dtype=np.uint8)
            diff = planted(rng, F, L)
            want, want_which = LT.pick(rows, row_bytes, L, diff)
            for in_off, out_off, with_which in ((0, 0, True), (1, 3, True), (3, 1, False)):
                o = mem.out(F * row_bytes, out_off)
                w = mem.out(F * 4, 4) if with_which else None
                _lib.check(lib.aeth_polar_list_pick(ctx.h, mem.inp(rows, in_off), row_bytes, F, L, mem.inp(diff.ravel()), mem.ptr(o), mem.ptr(w)))
                assert mem.get(o).tobytes() == want.tobytes(), (row_bytes, L, F, in_off, out_off)
                if with_which:
                    assert mem.get(w, np.uint32).tolist() == want_which.tolist(), (row_bytes, L, F)
            mem.free()


def test_pick_through_python(ctx):
    rng = np.random.default_rng(5)
    rows = rng.integers(0, 2, 9 * 4 * 24, dtype=np.uint8)
    diff = planted(rng, 9, 4)
    out, which = ap.polar.pick(ctx, rows, 24, 4, diff.ravel())
    want, want_which = LT.pick(rows, 24, 4, diff)
    assert out.to_host().tobytes() == want.tobytes() and which.to_host().tolist() == want_which.tolist()
    assert ap.polar.NONE in want_which and 0 in want_which and 3 in want_which


def test_decode_through_python(ctx, objects):
    c = objects("5x16", 4)
    F = 3 * c.group + 1
    soft = soft_of("5x16", "noisy", F)
    want, want_rec = truth_of("5x16", 4, "noisy", F)
    for all_, cw in ((False, False), (True, False), (False, True), (True, True)):
        bits, rec = c.decode(soft, all=all_, codeword=cw)
        flags = (LT.ALL if all_ else 0) | (LT.CODEWORD if cw else 0)
        assert bits.to_host().tobytes() == want[flags].tobytes() and rec.to_host().tobytes() == want_rec.tobytes()
    bits, rec = c.decode(soft, records=False)
    assert rec is None and bits.to_host().tobytes() == want[0].tobytes()
    assert ap.polar.LIST_RECORD == LT.LIST_RECORD and ap.polar.ALL == LT.ALL


# ---- 7 -----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx, objects, mem):
    c = objects("5x16", 4)
    N, K, L = c.n, c.k, 4
    soft = mem.inp(np.zeros(2 * N, np.int8))
    diff = mem.inp(np.zeros(2 * L, np.uint64))
    o, r = mem.out(2 * L * N), mem.out(64, 4)
    lib = c._lib
    assert lib.aeth_polar_list_decode(c.h, soft, 2 * N - 1, 0, mem.ptr(o), 2 * K, mem.ptr(r)) == _lib.E_LEN
    assert lib.aeth_polar_list_decode(c.h, soft, 2 * N, 0, mem.ptr(o), 2 * L * K, mem.ptr(r)) == _lib.E_LEN
    assert lib.aeth_polar_list_decode(c.h, soft, 2 * N, LT.ALL, mem.ptr(o), 2 * K, mem.ptr(r)) == _lib.E_LEN
    assert lib.aeth_polar_list_decode(c.h, soft, 2 * N, LT.ALL | LT.CODEWORD, mem.ptr(o), 2 * L * K, mem.ptr(r)) == _lib.E_LEN
    assert lib.aeth_polar_list_decode(c.h, soft, 2 * N, 4, mem.ptr(o), 2 * K, mem.ptr(r)) == _lib.E_ARG
    assert lib.aeth_polar_list_decode(c.h, soft, 2 * N, 0, mem.ptr(o), 2 * K, C.c_void_p(mem.ptr(r).value + 1)) == _lib.E_ALIGN
    assert lib.aeth_polar_list_decode(c.h, soft, 2 * N, 1, mem.ptr(o), 2 * N, C.c_void_p(mem.ptr(o).value + 2 * N - 4)) == _lib.E_ARG
    assert lib.aeth_polar_list_decode(c.h, mem.ptr(o), 2 * N, 0, mem.ptr(o), 2 * K, mem.ptr(r)) == _lib.E_ARG
    assert lib.aeth_polar_list_pick(ctx.h, soft, N, 2, 0, diff, mem.ptr(o), mem.ptr(r)) == _lib.E_ARG
    assert lib.aeth_polar_list_pick(ctx.h, soft, N, 2, 9, diff, mem.ptr(o), mem.ptr(r)) == _lib.E_ARG
    assert lib.aeth_polar_list_pick(ctx.h, soft, 0, 2, 1, diff, mem.ptr(o), mem.ptr(r)) == _lib.E_LEN
    assert lib.aeth_polar_list_pick(ctx.h, soft, N, 2, 1, C.c_void_p(diff.value + 4), mem.ptr(o), mem.ptr(r)) == _lib.E_ALIGN
    assert lib.aeth_polar_list_pick(ctx.h, soft, N, 2, 1, diff, mem.ptr(o), C.c_void_p(mem.ptr(r).value + 2)) == _lib.E_ALIGN
    assert lib.aeth_polar_list_pick(ctx.h, mem.ptr(o), N, 2, 1, diff, mem.ptr(o), mem.ptr(r)) == _lib.E_ARG
    assert lib.aeth_polar_list_pick(ctx.h, soft, N, 2, 1, diff, mem.ptr(o), C.c_void_p(mem.ptr(o).value + 2 * N - 4)) == _lib.E_ARG
    assert lib.aeth_polar_list_decode(c.h, soft, 0, LT.ALL, mem.ptr(o), 0, mem.ptr(r)) == _lib.OK         # F = 0: nothing is launched
    assert lib.aeth_polar_list_pick(ctx.h, soft, N, 0, 4, diff, mem.ptr(o), mem.ptr(r)) == _lib.OK
    ctx.sync()
    assert (mem.get(o) == SENTINEL).all() and (mem.get(r) == SENTINEL).all()
    for L_bad, code in ((0, _lib.E_ARG), (3, _lib.E_ARG), (16, _lib.E_ARG)):
        with pytest.raises(ap.AetherError) as e:
            ap.PolarList(ctx, 5, T.mask(5, 16), L_bad)
        assert e.value.code == code and f"L = {L_bad}" in str(e.value)
    with pytest.raises(ap.AetherError) as e:
        ap.PolarList(ctx, 6, CODES["6x1"][1], 4)
    assert e.value.code == _lib.E_ARG and "K = 1" in str(e.value)
