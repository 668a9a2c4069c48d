"""GPU: aeth_rs_encode / aeth_rs_decode (include/aether_hip.h) against the restatement tests/rs_truth.py, byte for byte,
record for record and summary for summary; outputs lie between guard bytes that are checked unchanged.

Codewords are independent, so the truth is computed once per code on a POOL of words and every device call below is an
arrangement of pool words into frames: RS(7, 3) over GF(8) against the exhaustive search, (15, 11), (15, 8), dvb-204-188,
ccsds-255-223 and (255, 191) against Euclid's algorithm.  The pool holds clean words, the all-zero and the all-N0 word,
errors of weight 0 .. t + 2 at random positions (t = r div 2), errors at the first and last symbol, errors in the parity
only, erasures alone up to r + 1, mixes exactly on and one past 2 e + f = r, erased positions that also carry an error,
and (m < 8) bytes with bits above m set.  The share of pool words beyond the bound is asserted between 20 % and 60 % from
the truth's own verdicts.

  1. every depth 1, 2, 4, 5, 64 x frame counts 1, 2, G - 1, G, G + 1 (G = aeth_rs_group), with and without PAYLOAD.
  2. batches in which only codeword 0, only the last, or every second codeword is damaged.
  3. records and summary NULL in every combination; zero frames write the summary {0, 0}.
  4. every input x output alignment 0 .. 15 on one small shape.
  5. a call cut at a frame equals one call; the same bytes twice give the same output.
  6. encode for the same depths and counts, input bytes 0 .. 255, odd pointers; encode -> decode gives {0, 0} records."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import aether_primitives_amd as ap                    # noqa: E402
from aether_primitives_amd import _lib, rs            # noqa: E402
import rs_truth as T                                  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0xA5
DEPTHS = (1, 2, 4, 5, 64)

CODES = {
    "rs-7-3": (3, 0xb, 1, 1, 4, 7),
    "rs-15-11": (4, 0x13, 1, 1, 4, 15),
    "rs-15-8": (4, 0x13, 0, 2, 7, 15),
    "dvb-204-188": (8, 0x11d, 0, 1, 16, 204),
    "ccsds-255-223": (8, 0x187, 112, 11, 32, 255),
    "rs-255-191": (8, 0x11d, 3, 1, 64, 255),
}
_POOL = {}


def plants(r, n):
    """[(errors, erasures, kind)] of a pool; kind: '', 'ends', 'parity', 'overlap', 'zero', 'ones'"""
    t = r // 2
    weights = range(t + 3) if t <= 6 else sorted({0, 1, 2, t // 2, t - 1, t, t + 1, t + 2})
    out = [(0, 0, "")] * 6 + [(0, 0, "zero"), (0, 0, "ones")]
    for w in weights:
        out += [(w, 0, "")] * (3 if w > t else 2)
    out += [(min(2, n), 0, "ends"), (max(t, 1), 0, "parity"), (t + 1, 0, "parity")]
    for f in (range(1, r + 2) if r <= 8 else sorted({1, 2, r // 2, r - 1, r, r + 1})):
        out += [(0, f, "")] * (2 if f > r else 1)
    for f in sorted({1, 2, r // 2, r - 2, r - 1} - {0, -1}):
        e = (r - f) // 2
        out += [(e, f, ""), (e + 1, f, ""), (e + 1, f, "")]
    out += [(1, min(3, r), "overlap"), (min(3, r), min(3, r), "overlap"), (t + 1, 2, "overlap")]
    out += [(t + 1 + i % 3, i % 2, "") for i in range(len(out) // 5)]     # weight on the far side of the bound
    return out


def pool(name):
    """{words [P][n] as sent to the device, era [P][n], out [P][n], corrected [P], status [P], truth}: once per code"""
    if name not in _POOL:
        code = CODES[name]
        tr = T.Truth(code)
        rng = np.random.default_rng(sum(code))
        spec = plants(tr.r, tr.n)
        rng.shuffle(spec)
        P = len(spec)
        words = tr.encode(rng.integers(0, tr.N0 + 1, P * tr.k).astype(np.uint8)).reshape(P, tr.n)
        era = np.zeros_like(words)
        for w, (ne, nf, kind) in enumerate(spec):
            ne, nf = int(ne), int(nf)
            if kind == "zero":
                words[w] = 0
            elif kind == "ones":
                words[w] = tr.N0
            elif kind == "ends":
                for j in (0, tr.n - 1)[:ne]:
                    words[w, j] ^= rng.integers(1, tr.N0 + 1)
            elif kind == "parity":
                for j in tr.k + rng.permutation(tr.r)[:ne]:
                    words[w, j] ^= rng.integers(1, tr.N0 + 1)
            else:
                words[w:w + 1], era[w:w + 1] = T.damage(rng, tr, words[w:w + 1], [ne], [nf], overlap=kind == "overlap")
        if tr.m < 8:                                                      # bits above m: the library masks them
            words |= ((rng.integers(0, 1 << (8 - tr.m), words.shape) << tr.m) * (rng.random(words.shape) < 0.3)).astype(np.uint8)
        out, corrected, status = tr.decode(words.ravel(), era.ravel(), exhaustive=name == "rs-7-3")
        share = float(status.mean())
        assert 0.2 <= share <= 0.6, f"{name}: {share:.2f} of the pool lies beyond the bound"
        _POOL[name] = dict(words=words, era=era, out=out.reshape(P, tr.n), corrected=corrected, status=status, truth=tr,
                           clean=np.flatnonzero((corrected == 0) & (status == 0) & (era.sum(axis=1) == 0)),
                           hurt=np.flatnonzero((corrected != 0) | (status != 0)))
    return _POOL[name]


def frames(words, depth):
    """words [F depth][n] -> the bytes of F frames: symbol j of codeword i of frame f at f depth n + j depth + i"""
    W, n = words.shape
    return np.ascontiguousarray(words.reshape(W // depth, depth, n).transpose(0, 2, 1)).ravel()


class Mem:
    """device buffers of one test: inputs at an offset behind an allocation's start, outputs between guards"""

    def __init__(self, ctx):
        self.ctx, self.held = ctx, []

    def inp(self, a, off=0):
        a = np.ascontiguousarray(a)
        base = self.ctx.alloc(off + a.nbytes + 16)
        self.held.append(base)
        if a.nbytes:
            self.ctx.upload(base + off, a.view(np.uint8))
        return C.c_void_p(base + off)

    def out(self, n, off=0):
        base = self.ctx.alloc(GUARD + off + n + GUARD)
        self.held.append(base)
        self.ctx.upload(base, np.full(GUARD + off + n + GUARD, SENTINEL, np.uint8))
        return (base, n, off)

    @staticmethod
    def ptr(o):
        return C.c_void_p(o[0] + GUARD + o[2]) if o is not None else None

    def get(self, o, dtype=np.uint8):
        base, n, off = o
        got = np.empty(GUARD + off + n + GUARD, np.uint8)
        self.ctx.download(base, got)
        lo = GUARD + off
        assert (got[:lo] == SENTINEL).all(), "bytes in front of the output were written"
        assert (got[lo + n:] == SENTINEL).all(), "bytes behind the output were written"
        return got[lo:lo + n].copy().view(dtype)

    def free(self):
        for b in self.held:
            self.ctx.free(b)
        self.held = []


@pytest.fixture
def mem(ctx):
    m = Mem(ctx)
    yield m
    m.free()


@pytest.fixture(scope="module")
def objects(ctx):
    made = {}

    def get(name):
        if name not in made:
            made[name] = ap.Rs(ctx, CODES[name])
        return made[name]
    yield get
    for o in made.values():
        o.close()


def d_decode(mem, obj, coded, era, depth, payload=False, records=True, summary=True, in_off=0, out_off=0):
    """-> (bytes, records or None, summary or None) of one device call"""
    W = coded.size // obj.n
    nout = W * (obj.k if payload else obj.n)
    o = mem.out(nout, out_off)
    r = mem.out(W * 8, 4) if records else None
    s = mem.out(16, 8) if summary else None
    _lib.check(obj._lib.aeth_rs_decode(obj.h, mem.inp(coded, in_off), coded.size, mem.inp(era, (in_off * 7 + 3) % 16) if era is not None else None, depth,
                                       rs.PAYLOAD if payload else 0, mem.ptr(o), nout, mem.ptr(r), mem.ptr(s)))
    return mem.get(o), (mem.get(r, np.uint32).reshape(W, 2) if records else None), (mem.get(s, np.uint64) if summary else None)


def check_call(mem, obj, p, idx, depth, payload=False, records=True, summary=True, with_era=True, **kw):
    """one device call over the pool words `idx` (a multiple of depth), held against the truth"""
    idx = np.asarray(idx)
    if not with_era:
        assert not p["era"][idx].any()
    got, rec, summ = d_decode(mem, obj, frames(p["words"][idx], depth), frames(p["era"][idx], depth) if with_era else None, depth, payload, records, summary, **kw)
    nb = obj.k if payload else obj.n
    exp = frames(p["out"][idx][:, :nb], depth)
    assert (got == exp).all(), f"{int((got != exp).sum())} bytes differ, first at {int(np.flatnonzero(got != exp)[0])}"
    if records:
        assert (rec[:, 0] == p["corrected"][idx]).all() and (rec[:, 1] == p["status"][idx]).all()
    if summary:
        assert tuple(int(v) for v in summ) == (int(p["status"][idx].sum()), int(p["corrected"][idx].sum()))
    return got


def group_counts(G):
    return sorted({F for F in (1, 2, G - 1, G, G + 1) if F >= 1})


# ---- 1 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CODES))
def test_getters(objects, name):
    m, poly, fcr, prim, r, n = CODES[name]
    o = objects(name)
    assert (o.n, o.k, o.nroots, o.m) == (n, n - r, r, m)
    R2 = 1 << (r - 1).bit_length()
    assert o.group == 256 // R2 and 0 < o.lds_bytes(1) <= 8192 and o.lds_bytes(0) == 0 and o.lds_bytes(65) == 0


@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("name", sorted(CODES))
def test_decode_every_depth_and_frame_count(mem, objects, name, depth):
    p, o = pool(name), objects(name)
    P = p["words"].shape[0]
    start = 0
    for k, F in enumerate(group_counts(o.group)):
        idx = (start + np.arange(F * depth)) % P
        start += 7 * F + 1
        check_call(mem, o, p, idx, depth, payload=bool((k + depth) & 1))
        mem.free()


@pytest.mark.parametrize("name", sorted(CODES))
def test_decode_whole_pool_both_outputs(mem, objects, name):
    p, o = pool(name), objects(name)
    idx = np.arange(p["words"].shape[0])
    for payload in (False, True):
        check_call(mem, o, p, idx, 1, payload=payload)


# ---- 2 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", (1, 4))
@pytest.mark.parametrize("name", sorted(CODES))
def test_clean_and_damaged_codewords_side_by_side(mem, objects, name, depth):
    p, o = pool(name), objects(name)
    W = (2 * o.group + 3) * depth
    clean = p["clean"][np.arange(W) % p["clean"].size]
    hurt = p["hurt"][np.arange(W) % p["hurt"].size]
    for pattern in ("first", "last", "second"):
        idx = clean.copy()
        if pattern == "first":
            idx[0] = hurt[0]
        elif pattern == "last":
            idx[-1] = hurt[1]
        else:
            idx[::2] = hurt[::2]
        check_call(mem, o, p, idx, depth)
        mem.free()
    check_call(mem, o, p, clean, depth, with_era=False)                   # nothing damaged and no erasure array at all


# ---- 3 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("records", (False, True))
@pytest.mark.parametrize("summary", (False, True))
@pytest.mark.parametrize("payload", (False, True))
def test_optional_outputs(mem, objects, payload, summary, records):
    p, o = pool("rs-15-8"), objects("rs-15-8")
    check_call(mem, o, p, np.arange(3 * (o.group + 1)) % p["words"].shape[0], 3, payload=payload, records=records, summary=summary)


def test_zero_frames_write_the_summary_and_nothing_else(mem, objects):
    o = objects("rs-15-11")
    out, rec, s = mem.out(32), mem.out(32, 4), mem.out(16, 8)
    _lib.check(o._lib.aeth_rs_decode(o.h, mem.inp(np.zeros(4, np.uint8)), 0, None, 5, 0, mem.ptr(out), 0, mem.ptr(rec), mem.ptr(s)))
    assert tuple(mem.get(s, np.uint64)) == (0, 0)
    assert (mem.get(out) == SENTINEL).all() and (mem.get(rec) == SENTINEL).all()
    _lib.check(o._lib.aeth_rs_decode(o.h, None, 0, None, 5, 0, None, 0, None, None))
    _lib.check(o._lib.aeth_rs_encode(o.h, None, 0, 5, None, 0))


# ---- 4 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_off", range(16))
def test_every_alignment(mem, objects, in_off):
    p, o = pool("rs-15-11"), objects("rs-15-11")
    idx = np.arange(6) + in_off
    tr = p["truth"]
    data = p["out"][idx][:, :tr.k]
    for out_off in range(16):
        check_call(mem, o, p, idx, 2, payload=bool(out_off & 1), in_off=in_off, out_off=out_off)
        enc = mem.out(6 * tr.n, out_off)
        _lib.check(o._lib.aeth_rs_encode(o.h, mem.inp(frames(data, 2), in_off), 6 * tr.k, 2, mem.ptr(enc), 6 * tr.n))
        assert (mem.get(enc) == tr.encode(frames(data, 2), 2)).all()
        mem.free()


# ---- 5 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("rs-15-8", "ccsds-255-223"))
def test_a_cut_call_equals_one_call_and_a_repeat_equals_the_first(mem, objects, name):
    p, o = pool(name), objects(name)
    depth, F = 5, o.group + 2
    idx = np.arange(F * depth) % p["words"].shape[0]
    whole = check_call(mem, o, p, idx, depth)
    again = check_call(mem, o, p, idx, depth)
    assert (whole == again).all()
    for cut in (1, F // 2, F - 1):
        a = check_call(mem, o, p, idx[:cut * depth], depth)
        b = check_call(mem, o, p, idx[cut * depth:], depth)
        assert (np.concatenate([a, b]) == whole).all()
        mem.free()


# ---- 6 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("name", sorted(CODES))
def test_encode(mem, objects, name, depth):
    o, tr = objects(name), pool(name)["truth"]
    rng = np.random.default_rng(depth * 100 + len(name))
    for F in group_counts(o.group):
        data = rng.integers(0, 256, F * depth * tr.k).astype(np.uint8)   # every byte value: bits above m are masked
        enc = mem.out(F * depth * tr.n, F & 3)
        _lib.check(o._lib.aeth_rs_encode(o.h, mem.inp(data, depth & 3), data.size, depth, mem.ptr(enc), F * depth * tr.n))
        got = mem.get(enc).reshape(F, depth * tr.n)
        exp = tr.encode(data, depth).reshape(F, depth * tr.n)
        assert (got == exp).all()
        mem.free()


@pytest.mark.parametrize("name", sorted(CODES))
def test_encode_then_decode_reports_nothing(ctx, objects, name):
    o = objects(name)
    rng = np.random.default_rng(9)
    data = rng.integers(0, 1 << o.m, 3 * 4 * o.k).astype(np.uint8)
    coded = o.encode(data, depth=4)
    out, rec, summ = o.decode(coded, depth=4, payload=True)
    rec, summ = rec.to_host(), summ.to_host()
    assert (out.to_host() == data).all()
    assert not rec["corrected"].any() and not rec["status"].any() and (int(summ["n_failed"]), int(summ["n_corrected"])) == (0, 0)
