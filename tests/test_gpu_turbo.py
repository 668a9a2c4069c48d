"""GPU: aeth_turbo_encode / aeth_turbo_decode (include/aether_hip.h) against the restatement tests/turbo_truth.py, byte for
byte and record for record; outputs lie between guard bytes that are checked unchanged.

  1. decode, per code -- (k3, K = 8, W = 8, A = 0), (lte, 40, W = 40), (lte, 40, 16, 8) with a ragged last window and
     warm-ups clipped at both ends, (lte, 40, 8, 0), (lte, 37, a seeded random permutation, 5, 3), (ccsds, 64, 16, 16),
     (lte, 512, 32, 16), (lte, 1024, 8, 8) with 128 windows, two waves per codeword, (lte, 6144, 32, 32) through two
     iterations: S = 4, 8 and 16 are all reached -- six kinds of input (zeros, uniform int8 with -128 and 127 planted, all
     -128, all +127, a noisy codeword that converges, one beyond capacity) x max_iter 1, 2, 8 x early stop and none at
     3 G + 1 codewords, records given and NULL; F = 1, G - 1, G, G + 1 on the noisy input, where neighbours in one
     workgroup stop at different iterations.  One run of the restatement per (code, kind) serves all of them.
  2. soft pointer at byte offsets 0 .. 3 x output at 0 and 1.
  3. the same call twice; a call cut at a codeword equals two calls.
  4. encode for the same codes and F, input bytes 0 .. 255, odd pointers.
  5. refusals launch nothing; F = 0."""
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
import turbo_truth as T                               # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0xA5
KINDS = ("zero", "uniform", "min", "max", "noisy", "hopeless")
CODES = T.test_codes()
GROUPS = {"k3_8": 64, "lte40_full": 64, "lte40_16_8": 64, "lte40_8_0": 51, "lte37_rand": 32, "ccsds64": 64, "lte512": 11, "lte1024": 2,
          "lte6144": 1}
_TRUTH = {}


def shape(name):
    cname, pi, W, A = CODES[name]
    code = T.named(cname)
    return code, pi, W, A, pi.size, 3 * pi.size + 4 * code.nu


def iterations_of(name):
    return (1, 2) if name == "lte6144" else (1, 2, 8)


def count_of(name):
    return 3 * GROUPS[name] + 1


def soft_of(name, kind):
    """count_of(name) codewords of the kind's input for this code"""
    code, pi, W, A, K, N = shape(name)
    key = ("soft", name, kind)
    if key not in _TRUTH:
        F = count_of(name)
        rng = np.random.default_rng(len(name) * 1000 + K + KINDS.index(kind))
        if kind == "zero":
            s = np.zeros(F * N, np.int8)
        elif kind == "uniform":
            s = rng.integers(-128, 128, F * N).astype(np.int8)
            s[::97] = -128
            s[5::89] = 127
        elif kind == "min":
            s = np.full(F * N, -128, np.int8)
        elif kind == "max":
            s = np.full(F * N, 127, np.int8)
        else:
            coded = T.encode(code, pi, rng.integers(0, 2, F * K, dtype=np.uint8))
            s = T.noisy_soft(rng, coded, 1.0 if kind == "noisy" else 2.5)
        _TRUTH[key] = s
    return _TRUTH[key]


def truth_of(name, kind, max_iter, flags):
    """(decisions [F][K], records [F]) of the restatement, from one run per (code, kind)"""
    code, pi, W, A, K, N = shape(name)
    key = ("hist", name, kind)
    if key not in _TRUTH:
        history = []
        T.decode(code, pi, W, A, soft_of(name, kind), max(iterations_of(name)), 0, None, history)
        _TRUTH[key] = history
    bits, rec = T.from_history(_TRUTH[key], max_iter, flags)
    return bits.reshape(-1, K), rec


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
            cname, pi, W, A = CODES[name]
            made[name] = ap.Turbo(ctx, cname, pi, W, A)
        return made[name]
    yield get
    for o in made.values():
        o.close()


def d_decode(mem, code, soft, max_iter, flags=0, records=True, in_off=0, out_off=0):
    """-> (bits [F][K], records [F] or None) of one device call"""
    F = soft.size // code.n
    o = mem.out(F * code.k, out_off)
    r = mem.out(F * 8, 4) if records else None
    _lib.check(code._lib.aeth_turbo_decode(code.h, mem.inp(soft, in_off), soft.size, max_iter, flags, mem.ptr(o), F * code.k, mem.ptr(r)))
    return mem.get(o).reshape(F, code.k), (mem.get(r).view(T.RECORD) if records else None)


def group_counts(G):
    return sorted({F for F in (1, G - 1, G, G + 1) if F >= 1})


# ---- 1 -----------------------------------------------------------------------------------------------------------------
def test_getters_and_every_built_state_count(objects):
    seen = set()
    for name in sorted(CODES):
        code, pi, W, A, K, N = shape(name)
        c = objects(name)
        assert (c.k, c.n, c.states, c.window, c.warmup, c.windows) == (K, N, code.S, W, A, (K - 1) // W + 1)
        assert c.group == GROUPS[name] and c.group * c.windows <= 1024
        per = ((N + 3) & ~3) + ((K + 3) & ~3) + 4 * K
        assert c.lds_bytes == c.group * per + 8 * c.group + 8 and c.lds_bytes <= 160 * 1024
        seen.add(c.states)
    assert seen == {4, 8, 16}, "a built state count that no code of this file reaches"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(CODES))
def test_decode_against_the_restatement(objects, mem, name, kind):
    c = objects(name)
    soft = soft_of(name, kind)
    for max_iter in iterations_of(name):
        for flags in (0, T.EARLY):
            want_bits, want_rec = truth_of(name, kind, max_iter, flags)
            bits, rec = d_decode(mem, c, soft, max_iter, flags)
            assert rec.tobytes() == want_rec.tobytes(), (name, kind, max_iter, flags, rec[:8], want_rec[:8])
            assert bits.tobytes() == want_bits.tobytes(), (name, kind, max_iter, flags)
        mem.free()
    last = max(iterations_of(name))
    bits, rec = d_decode(mem, c, soft, last, T.EARLY, records=False)
    assert rec is None and bits.tobytes() == truth_of(name, kind, last, T.EARLY)[0].tobytes()
    if kind == "zero":
        want_bits, want_rec = truth_of(name, kind, last, T.EARLY)
        assert not want_bits.any() and (want_rec["iterations"] == 1).all() and (want_rec["disagreements"] == 0).all()
    if kind == "noisy":
        want_bits, want_rec = truth_of(name, kind, last, T.EARLY)
        for Fs in group_counts(c.group):
            bits, rec = d_decode(mem, c, soft[:Fs * c.n], last, T.EARLY)
            assert rec.tobytes() == want_rec[:Fs].tobytes() and bits.tobytes() == want_bits[:Fs].tobytes(), (name, Fs)
        mem.free()


def test_neighbours_in_a_workgroup_stop_at_different_iterations():
    """the restatement's own verdict on the inputs above: early stop is exercised per codeword, not per workgroup"""
    mixed = 0
    for name in sorted(CODES):
        G = GROUPS[name]
        if G < 2:
            continue
        its = truth_of(name, "noisy", max(iterations_of(name)), T.EARLY)[1]["iterations"]
        first = its[:G]
        mixed += len(set(first.tolist())) > 1
    assert mixed >= 4
    its = truth_of("lte512", "noisy", 8, T.EARLY)[1]["iterations"][:11]
    assert len(set(its.tolist())) > 1 and its.min() < 8
    assert (truth_of("lte512", "hopeless", 8, T.EARLY)[1]["disagreements"] > 0).all()


# ---- 2 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_off", (0, 1, 2, 3))
def test_any_byte_alignment(objects, mem, in_off):
    for name in ("lte40_16_8", "lte37_rand"):
        c = objects(name)
        F = c.group + 1
        soft = soft_of(name, "uniform")[:F * c.n]
        for out_off in (0, 1):
            for flags in (0, T.EARLY):
                want_bits, want_rec = truth_of(name, "uniform", 2, flags)
                bits, rec = d_decode(mem, c, soft, 2, flags, True, in_off, out_off)
                assert rec.tobytes() == want_rec[:F].tobytes()
                assert bits.tobytes() == want_bits[:F].tobytes(), (name, in_off, out_off, flags)


# ---- 3 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("k3_8", "lte37_rand", "lte512", "lte1024"))
def test_same_bytes_twice_and_two_calls_equal_one(objects, mem, name):
    c = objects(name)
    G = c.group
    F = count_of(name)
    soft = soft_of(name, "noisy")
    one = d_decode(mem, c, soft, 8, T.EARLY)
    again = d_decode(mem, c, soft, 8, T.EARLY)
    assert one[0].tobytes() == again[0].tobytes() and one[1].tobytes() == again[1].tobytes()
    for cut in sorted({1, max(G - 1, 1), G, G + 1, F - 1}):
        a = d_decode(mem, c, soft[:cut * c.n], 8, T.EARLY)
        b = d_decode(mem, c, soft[cut * c.n:], 8, T.EARLY)
        assert a[0].tobytes() + b[0].tobytes() == one[0].tobytes() and a[1].tobytes() + b[1].tobytes() == one[1].tobytes(), cut
        mem.free()


# ---- 4 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CODES))
def test_encode_against_the_restatement(objects, mem, name):
    code, pi, W, A, K, N = shape(name)
    c = objects(name)
    G = c.group
    Fm = max(count_of(name), 70 if K <= 64 else 0)                 # more than one workgroup of the encoder as well
    rng = np.random.default_rng(K + N)
    u = rng.integers(0, 256, Fm * K, dtype=np.uint8)
    u[:K] = 255
    want = T.encode(code, pi, u).reshape(Fm, N)
    for F in sorted({1, 32, 33, Fm} | set(group_counts(G))):
        if F < 1 or F > Fm:
            continue
        for in_off, out_off in ((0, 0), (1, 3)):
            o = mem.out(F * N, out_off)
            _lib.check(c._lib.aeth_turbo_encode(c.h, mem.inp(u[:F * K], in_off), F * K, mem.ptr(o), F * N))
            assert mem.get(o).tobytes() == want[:F].tobytes(), (name, F, in_off, out_off)
        mem.free()
    # the Python layer, and a decode of what it encoded: one iteration, the constituents agree
    coded = c.encode(u)
    assert coded.to_host().tobytes() == want.tobytes()
    bits, rec = c.decode(T.soft_of_bits(want.ravel(), 64), max_iter=4, early=True)
    assert bits.to_host().tobytes() == (u & 1).tobytes()
    rec = rec.to_host()
    assert rec.dtype == T.RECORD and (rec["iterations"] == 1).all() and (rec["disagreements"] == 0).all()
    bits, none = c.decode(T.soft_of_bits(want.ravel(), 1), max_iter=1, records=False)
    assert none is None and bits.to_host().tobytes() == (u & 1).tobytes()


def _free_bytes():
    hip = _lib.load()                              # hipMemGetInfo of the runtime the library is bound to
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


# ---- 5 -----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx, objects, mem):
    c = objects("lte40_16_8")
    N, K = c.n, c.k
    soft = mem.inp(np.zeros(2 * N, np.int8))
    o, r = mem.out(2 * N), mem.out(16, 4)
    lib = c._lib
    assert lib.aeth_turbo_decode(c.h, soft, 2 * N - 1, 1, 0, mem.ptr(o), 2 * K, mem.ptr(r)) == _lib.E_LEN
    assert lib.aeth_turbo_decode(c.h, soft, 2 * N, 1, 0, mem.ptr(o), 2 * N, mem.ptr(r)) == _lib.E_LEN
    assert lib.aeth_turbo_decode(c.h, soft, 2 * N, 0, 0, mem.ptr(o), 2 * K, mem.ptr(r)) == _lib.E_ARG
    assert lib.aeth_turbo_decode(c.h, soft, 2 * N, 65, 0, mem.ptr(o), 2 * K, mem.ptr(r)) == _lib.E_ARG
    assert lib.aeth_turbo_decode(c.h, soft, 2 * N, 1, 2, mem.ptr(o), 2 * K, mem.ptr(r)) == _lib.E_ARG
    assert lib.aeth_turbo_decode(c.h, soft, 2 * N, 1, 0, mem.ptr(o), 2 * K, C.c_void_p(mem.ptr(o).value + 2 * K - 4)) == _lib.E_ARG
    assert lib.aeth_turbo_decode(c.h, soft, 2 * N, 1, 0, mem.ptr(o), 2 * K, C.c_void_p(mem.ptr(r).value + 1)) == _lib.E_ALIGN
    assert lib.aeth_turbo_decode(c.h, mem.ptr(o), 2 * N, 1, 0, mem.ptr(o), 2 * K, mem.ptr(r)) == _lib.E_ARG
    assert lib.aeth_turbo_encode(c.h, soft, 2 * K, mem.ptr(o), 2 * N - 1) == _lib.E_LEN
    assert lib.aeth_turbo_encode(c.h, soft, 2 * K + 1, mem.ptr(o), 2 * N) == _lib.E_LEN
    assert lib.aeth_turbo_encode(c.h, mem.ptr(o), 2 * K, mem.ptr(o), 2 * N) == _lib.E_ARG
    assert lib.aeth_turbo_decode(c.h, soft, 0, 1, 0, mem.ptr(o), 0, mem.ptr(r)) == _lib.OK             # F = 0: nothing is launched
    assert lib.aeth_turbo_encode(c.h, soft, 0, mem.ptr(o), 0) == _lib.OK
    ctx.sync()
    assert (mem.get(o) == SENTINEL).all() and (mem.get(r) == SENTINEL).all()
    free = _free_bytes()
    for bad in (dict(code=(9, 0o13, 0o15)), dict(K=7), dict(window=0), dict(dup=True)):
        pi = T.qpp(40, 3, 10)
        if bad.get("dup"):
            pi[1] = pi[0]
        with pytest.raises(ap.AetherError) as e:
            ap.Turbo(ctx, bad.get("code", "lte"), pi[:bad.get("K", 40)], bad.get("window", 16), 8)
        assert e.value.code in (_lib.E_ARG, _lib.E_UNSUPPORTED)
    ctx.sync()
    assert _free_bytes() == free, "a refused create changed the free device memory"
