"""GPU: aeth_polar_encode / aeth_polar_decode (include/aether_hip.h) against the restatement tests/polar_truth.py, byte for
byte and record for record; outputs lie between guard bytes that are checked unchanged.

  1. decode, per code -- (3, 4), (3, 8) rate 1, (5, 16), (6, 1) with the one information leaf last, (7, 64) with a seeded
     random mask, (9, 171), (10, 512), (10, 1023); between them they reach every lane count the build contains -- six kinds
     of input (values in {-1, 0, 1}, all zero, uniform int8 with -128 planted, all +127, all -128, a noisy codeword) x
     flips NULL, all NONE and a per-codeword mix of index[0] of a first pass, a frozen position, N and NONE, each with
     and without AETH_POLAR_CODEWORD, at 3 G + 1 codewords; records NULL; F = 1, G - 1, G, G + 1 on the uniform input.
  2. soft pointer at byte offsets 0 .. 3 x output at 0 and 1.
  3. the same call twice; a call cut at a codeword equals two calls.
  4. encode for the same codes and F, input bytes 0 .. 255, odd pointers.
  5. refusals launch nothing."""
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

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0xA5
KINDS = ("ties", "zero", "uniform", "max", "min", "noisy")
FLIPS = ("null", "none", "mix")
CODES = T.test_codes()
_TRUTH = {}


def soft_of(name, kind, F):
    """the first F codewords of the kind's input for this code: computed once at the largest F asked for first"""
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


def flips_of(name, kind, F, how):
    """None, or F positions: all NONE, or by codeword index[0] of a first pass, a frozen position, N, NONE"""
    if how == "null":
        return None
    n, msk = CODES[name]
    if how == "none":
        return np.full(F, T.NONE, np.uint32)
    first = truth_of(name, kind, F, "null")[2]["index"][:, 0]
    frozen = np.flatnonzero(msk == 0)
    out = np.full(F, T.NONE, np.uint32)
    out[0::4] = first[0::4]
    out[1::4] = frozen[len(frozen) // 2] if frozen.size else T.NONE
    out[2::4] = 1 << n
    return out


def truth_of(name, kind, F, how):
    """(decisions [F][K], re-encoded bits [F][N], records [F]) of the restatement"""
    n, msk = CODES[name]
    key = ("dec", name, kind, F, how)
    if key not in _TRUTH:
        soft, flip = soft_of(name, kind, F), flips_of(name, kind, F, how)
        bits, rec = T.decode(msk, soft, flip)
        word, rec2 = T.decode(msk, soft, flip, T.CODEWORD)
        assert rec.tobytes() == rec2.tobytes()
        _TRUTH[key] = (bits.reshape(F, -1), word.reshape(F, -1), rec)
    return _TRUTH[key]


class Mem:
    """device buffers of one test: inputs at an offset behind an allocation's start, outputs between guards"""

    def __init__(self, ctx):
        self.ctx, self.held = ctx, []

    def inp(self, a, off=0):
        if a is None:
            return None
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
            made[name] = ap.Polar(ctx, *CODES[name])
        return made[name]
    yield get
    for o in made.values():
        o.close()


def d_decode(mem, code, soft, flip=None, flags=0, records=True, in_off=0, out_off=0):
    """-> (bits [F][nb], records [F] or None) of one device call"""
    F = soft.size // code.n
    nb = code.n if flags & T.CODEWORD else code.k
    o = mem.out(F * nb, out_off)
    r = mem.out(F * 32, 4) if records else None
    _lib.check(code._lib.aeth_polar_decode(code.h, mem.inp(soft, in_off), soft.size, mem.inp(flip), flags, mem.ptr(o), F * nb, mem.ptr(r)))
    return mem.get(o).reshape(F, nb), (mem.get(r).view(T.RECORD) if records else None)


def group_counts(G):
    return sorted({F for F in (1, G - 1, G, G + 1) if F >= 1})


# ---- 1 -----------------------------------------------------------------------------------------------------------------
def test_getters_and_every_built_lane_count(objects):
    seen = set()
    for name in sorted(CODES):
        n, msk = CODES[name]
        c = objects(name)
        assert (c.n, c.k) == (1 << n, int(msk.sum()))
        assert c.lanes in (4, 8, 16) and 2 * c.lanes <= c.n and c.group * c.lanes == 64
        words = max(c.n // 32, 1)
        state = 2 * (c.n - 2 * c.lanes) + 8 * words
        assert c.lds_bytes % c.group == 0 and state <= c.lds_bytes // c.group < state + 128 and c.lds_bytes <= 65536
        seen.add(c.lanes)
    assert seen == {4, 8, 16}, "a built lane count that no code of this file reaches"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(CODES))
def test_decode_against_the_restatement(objects, mem, name, kind):
    c = objects(name)
    F = 3 * c.group + 1
    soft = soft_of(name, kind, F)
    for how in FLIPS:
        want_bits, want_word, want_rec = truth_of(name, kind, F, how)
        flip = flips_of(name, kind, F, how)
        for flags in (0, T.CODEWORD):
            bits, rec = d_decode(mem, c, soft, flip, flags)
            want = want_word if flags else want_bits
            assert rec.tobytes() == want_rec.tobytes(), (name, kind, how, flags)
            assert bits.tobytes() == want.tobytes(), (name, kind, how, flags)
        mem.free()
    assert truth_of(name, kind, F, "none")[2].tobytes() == truth_of(name, kind, F, "null")[2].tobytes()
    bits, rec = d_decode(mem, c, soft, flips_of(name, kind, F, "mix"), 0, records=False)
    assert rec is None and bits.tobytes() == truth_of(name, kind, F, "mix")[0].tobytes()
    if kind == "uniform":
        want_bits, want_word, want_rec = truth_of(name, kind, F, "mix")
        flip = flips_of(name, kind, F, "mix")
        for Fs in group_counts(c.group):
            bits, rec = d_decode(mem, c, soft[:Fs * c.n], flip[:Fs], T.CODEWORD)
            assert rec.tobytes() == want_rec[:Fs].tobytes() and bits.tobytes() == want_word[:Fs].tobytes(), (name, Fs)
        mem.free()


def test_the_mixed_flips_change_some_codewords_and_only_those(objects):
    """the restatement's own verdict: a flip at index[0] changes that codeword's decisions, the other three kinds none"""
    name = "9x171"
    F = 3 * objects(name).group + 1
    plain, flipped = truth_of(name, "noisy", F, "null")[0], truth_of(name, "noisy", F, "mix")[0]
    changed = (plain != flipped).any(axis=1)
    assert changed[0::4].all() and not changed[1::4].any() and not changed[2::4].any() and not changed[3::4].any()


# ---- 2 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_off", (0, 1, 2, 3))
def test_any_byte_alignment(objects, mem, in_off):
    for name in ("5x16", "7x64r"):
        c = objects(name)
        Fm = 3 * c.group + 1
        F = c.group + 1
        soft = soft_of(name, "uniform", Fm)[:F * c.n]
        want_bits, want_word, want_rec = truth_of(name, "uniform", Fm, "mix")
        flip = flips_of(name, "uniform", Fm, "mix")[:F]
        for out_off in (0, 1):
            for flags in (0, T.CODEWORD):
                bits, rec = d_decode(mem, c, soft, flip, flags, True, in_off, out_off)
                assert rec.tobytes() == want_rec[:F].tobytes()
                assert bits.tobytes() == (want_word if flags else want_bits)[:F].tobytes(), (name, in_off, out_off, flags)


# ---- 3 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("3x4", "7x64r", "10x512"))
def test_same_bytes_twice_and_two_calls_equal_one(objects, mem, name):
    c = objects(name)
    G = c.group
    F = 3 * G + 1
    soft = soft_of(name, "noisy", F)
    flip = flips_of(name, "noisy", F, "mix")
    one = d_decode(mem, c, soft, flip)
    again = d_decode(mem, c, soft, flip)
    assert one[0].tobytes() == again[0].tobytes() and one[1].tobytes() == again[1].tobytes()
    for cut in sorted({1, max(G - 1, 1), G, G + 1, F - 1}):
        a = d_decode(mem, c, soft[:cut * c.n], flip[:cut])
        b = d_decode(mem, c, soft[cut * c.n:], flip[cut:])
        assert a[0].tobytes() + b[0].tobytes() == one[0].tobytes() and a[1].tobytes() + b[1].tobytes() == one[1].tobytes(), cut
        mem.free()


# ---- 4 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CODES))
def test_encode_against_the_restatement(objects, mem, name):
    n, msk = CODES[name]
    c = objects(name)
    G = c.group
    Fm = max(3 * G + 1, 4096 // c.n * 4 + 1)                     # more than one workgroup of the encoder as well
    rng = np.random.default_rng(c.n + c.k)
    u = rng.integers(0, 256, Fm * c.k, dtype=np.uint8)
    u[:c.k] = 255
    want = T.encode(msk, u).reshape(Fm, c.n)
    for F in sorted({1, 4096 // c.n, 4096 // c.n + 1, 3 * G + 1, Fm} | set(group_counts(G))):
        if F < 1 or F > Fm:
            continue
        for in_off, out_off in ((0, 0), (1, 3)):
            o = mem.out(F * c.n, out_off)
            _lib.check(c._lib.aeth_polar_encode(c.h, mem.inp(u[:F * c.k], in_off), F * c.k, mem.ptr(o), F * c.n))
            assert mem.get(o).tobytes() == want[:F].tobytes(), (name, F, in_off, out_off)
        mem.free()
    # the Python layer, and a decode of what it encoded
    coded = c.encode(u)
    assert coded.to_host().tobytes() == want.tobytes()
    bits, rec = c.decode(T.soft_of_bits(want.ravel(), 64))
    assert bits.to_host().tobytes() == (u & 1).tobytes()
    rec = rec.to_host()
    assert rec.dtype == T.RECORD and (rec["index"][:, min(c.k, 4):] == T.NONE).all() and (rec["abs"][:, :min(c.k, 4)] >= 64).all()
    word, none = c.decode(T.soft_of_bits(want.ravel(), 64), flip=np.full(Fm, ap.polar.NONE, np.uint32), codeword=True, records=False)
    assert none is None and word.to_host().tobytes() == want.tobytes()


# ---- 5 -----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx, objects, mem):
    c = objects("5x16")
    N, K = c.n, c.k
    soft = mem.inp(np.zeros(2 * N, np.int8))
    flip = mem.inp(np.zeros(2, np.uint32))
    o, r = mem.out(2 * N), mem.out(64, 4)
    lib = c._lib
    assert lib.aeth_polar_decode(c.h, soft, 2 * N - 1, flip, 0, mem.ptr(o), 2 * K, mem.ptr(r)) == _lib.E_LEN
    assert lib.aeth_polar_decode(c.h, soft, 2 * N, flip, 0, mem.ptr(o), 2 * N, mem.ptr(r)) == _lib.E_LEN
    assert lib.aeth_polar_decode(c.h, soft, 2 * N, flip, 1, mem.ptr(o), 2 * K, mem.ptr(r)) == _lib.E_LEN
    assert lib.aeth_polar_decode(c.h, soft, 2 * N, flip, 2, mem.ptr(o), 2 * K, mem.ptr(r)) == _lib.E_ARG
    assert lib.aeth_polar_decode(c.h, soft, 2 * N, flip, 1, mem.ptr(o), 2 * N, C.c_void_p(mem.ptr(o).value + 2 * N - 4)) == _lib.E_ARG
    assert lib.aeth_polar_decode(c.h, soft, 2 * N, flip, 0, mem.ptr(o), 2 * K, C.c_void_p(mem.ptr(r).value + 1)) == _lib.E_ALIGN
    assert lib.aeth_polar_decode(c.h, soft, 2 * N, C.c_void_p(flip.value + 2), 0, mem.ptr(o), 2 * K, mem.ptr(r)) == _lib.E_ALIGN
    assert lib.aeth_polar_decode(c.h, soft, 2 * N, mem.ptr(o), 0, mem.ptr(o), 2 * K, mem.ptr(r)) == _lib.E_ARG
    assert lib.aeth_polar_encode(c.h, soft, 2 * K, mem.ptr(o), 2 * N - 1) == _lib.E_LEN
    assert lib.aeth_polar_encode(c.h, soft, 2 * K + 1, mem.ptr(o), 2 * N) == _lib.E_LEN
    assert lib.aeth_polar_encode(c.h, mem.ptr(o), 2 * K, mem.ptr(o), 2 * N) == _lib.E_ARG
    assert lib.aeth_polar_decode(c.h, soft, 0, flip, 0, mem.ptr(o), 0, mem.ptr(r)) == _lib.OK          # F = 0: nothing is launched
    assert lib.aeth_polar_encode(c.h, soft, 0, mem.ptr(o), 0) == _lib.OK
    ctx.sync()
    assert (mem.get(o) == SENTINEL).all() and (mem.get(r) == SENTINEL).all()
    with pytest.raises(ap.AetherError) as e:
        ap.Polar(ctx, 5, np.zeros(32, np.uint8))
    assert e.value.code == _lib.E_ARG and "K = 0" in str(e.value)
