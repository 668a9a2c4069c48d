"""GPU: aeth_ldpc_encode / aeth_ldpc_decode (include/aether_hip.h) against the restatement tests/ldpc_truth.py, byte for
byte and record for record; outputs lie between guard bytes that are checked unchanged.

  1. decode, per code -- the staircase codes (2, 4, 1), (3, 6, 5), (4, 8, 27), (4, 24, 64), (12, 24, 81), (6, 12, 96), one with
     a single-block row, and two the kernel treats differently: z = 300 (a lone codeword's lanes take several checks) and
     (32, 64, 256) with 128 blocks, whose state is the 64 KiB limit to the byte -- five kinds of input (values in {-1, 0, 1},
     all zero, uniform int8 with -128, all +127, a noisy codeword) x max_iter 0, 1, 7, 50 with and without early stop, at
     3 G + 1 codewords, each with and without the payload flag; F = 1, G - 1, G, G + 1 on the uniform input; records NULL.
  2. soft pointer at byte offsets 0 .. 3 x output at 0 and 1.
  3. the same call twice; a call cut at a codeword equals two calls.
  4. encode for the same codes and F, input bytes 0 .. 255, odd pointers.
  5. refusals launch nothing; 100 refused creates leave the device's free memory unchanged."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import aether_primitives_amd as ap                    # noqa: E402
from aether_primitives_amd import _lib, ldpc          # noqa: E402
import ldpc_truth as T                                # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0xA5
KINDS = ("ties", "zero", "uniform", "max", "noisy")
RUNS = ((0, 0), (0, T.EARLY), (1, 0), (1, T.EARLY), (7, 0), (7, T.EARLY), (50, 0), (50, T.EARLY))


def limit_code():
    """(32, 64, 256) with four blocks in every row: 2 N + E z = 65536"""
    shift = ldpc.staircase(32, 64, 256, col_weight=0)
    rng = np.random.default_rng(256)
    for r in range(32):
        free = np.flatnonzero(shift[r, :32] < 0)
        need = 4 - int((shift[r] >= 0).sum())
        shift[r, rng.choice(free, need, replace=False)] = rng.integers(0, 256, need)
    return shift


CODES = dict(T.test_codes())
CODES["2x4x300"] = (ldpc.staircase(2, 4, 300), 300)
CODES["limit"] = (limit_code(), 256)
_TRUTH = {}


def generator_of(name):
    if ("P", name) not in _TRUTH:
        _TRUTH["P", name] = T.generator(*CODES[name])
    return _TRUTH["P", name]


def soft_of(name, kind, F):
    """the first F codewords of the kind's input for this code: computed once at the largest F asked for first"""
    shift, z = CODES[name]
    rows, cols, N, M, K = T.dims(shift, z)
    key = ("soft", name, kind)
    if key not in _TRUTH or _TRUTH[key].size < F * N:
        rng = np.random.default_rng(len(name) * 1000 + KINDS.index(kind))
        if kind == "ties":
            s = rng.integers(-1, 2, F * N).astype(np.int8)
        elif kind == "zero":
            s = np.zeros(F * N, np.int8)
        elif kind == "uniform":
            s = rng.integers(-128, 128, F * N).astype(np.int8)
            s[::97] = -128
        elif kind == "max":
            s = np.full(F * N, 127, np.int8)
        else:
            s = T.bpsk_soft(rng, T.encode(shift, z, rng.integers(0, 2, F * K, dtype=np.uint8), generator_of(name)), 0.6)
        _TRUTH[key] = s
    return _TRUTH[key][:F * N]


def truth_of(name, kind, F, max_iter, early):
    """(all N bits [F][N], records [F][2]) of the restatement; the payload is its first K columns"""
    shift, z = CODES[name]
    key = ("dec", name, kind, F, max_iter, early)
    if key not in _TRUTH:
        bits, rec = T.decode(shift, z, soft_of(name, kind, F), max_iter, early)
        _TRUTH[key] = (bits.reshape(F, -1), rec)
    return _TRUTH[key]


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
            made[name] = ap.Ldpc(ctx, *CODES[name])
        return made[name]
    yield get
    for o in made.values():
        o.close()


def d_decode(mem, code, soft, max_iter, flags, records=True, in_off=0, out_off=0):
    """-> (bits [F][nb], records [F][2] or None) of one device call"""
    F = soft.size // code.n
    nb = code.k if flags & T.PAYLOAD else code.n
    o = mem.out(F * nb, out_off)
    r = mem.out(F * 8, 4) if records else None
    _lib.check(code._lib.aeth_ldpc_decode(code.h, mem.inp(soft, in_off), soft.size, max_iter, flags, mem.ptr(o), F * nb, mem.ptr(r)))
    return mem.get(o).reshape(F, nb), (mem.get(r, np.uint32).reshape(F, 2) if records else None)


def group_counts(G):
    return sorted({F for F in (1, G - 1, G, G + 1) if F >= 1})


# ---- 1 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CODES))
def test_getters_and_the_group(objects, name):
    shift, z = CODES[name]
    rows, cols, N, M, K = T.dims(shift, z)
    c = objects(name)
    E = int((shift >= 0).sum())
    assert (c.n, c.k, c.rows, c.cols, c.z, c.edges) == (N, K, rows, cols, z, E)
    G, state = c.group, 2 * N + E * z
    assert G >= 1 and (G == 1 or G * z <= 256) and G * state <= c.lds_bytes <= 65536
    assert (G + 1) * z > 256 or (G + 1) * (state + 1) > 65536, "a further codeword would have fitted"
    assert z >= 256 or G * z >= 64 or (G + 1) * (state + 1) > 65536, "fewer than 64 busy lanes where z and the LDS allow more"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", sorted(CODES))
def test_decode_against_the_restatement(objects, mem, name, kind):
    c = objects(name)
    F = 3 * c.group + 1 if name != "limit" else 3
    soft = soft_of(name, kind, F)
    for max_iter, early in RUNS:
        want_bits, want_rec = truth_of(name, kind, F, max_iter, early)
        for payload in (0, T.PAYLOAD):
            bits, rec = d_decode(mem, c, soft, max_iter, early | payload)
            tag = (name, kind, max_iter, early, payload)
            assert rec.tolist() == want_rec.tolist(), tag
            assert bits.tobytes() == np.ascontiguousarray(want_bits[:, :bits.shape[1]]).tobytes(), tag
        mem.free()
    if kind == "zero":
        bits, rec = truth_of(name, kind, F, 50, T.EARLY)
        assert not bits.any() and rec.tolist() == [[1, 0]] * F
    if kind == "uniform":
        for Fs in group_counts(c.group):
            for max_iter, early in ((7, T.EARLY), (7, 0)):
                want_bits, want_rec = truth_of(name, kind, F, max_iter, early)
                bits, rec = d_decode(mem, c, soft[:Fs * c.n], max_iter, early)
                assert rec.tolist() == want_rec[:Fs].tolist() and bits.tobytes() == want_bits[:Fs].tobytes(), (name, Fs, max_iter, early)
            mem.free()
        bits, rec = d_decode(mem, c, soft, 7, T.EARLY | T.PAYLOAD, records=False)
        assert rec is None and bits.tobytes() == np.ascontiguousarray(truth_of(name, kind, F, 7, T.EARLY)[0][:, :c.k]).tobytes()


def test_a_noisy_codeword_is_corrected(objects):
    """the restatement's own verdict on the noisy input of the (12, 24, 81) code: raw errors, none after decoding"""
    name = "12x24x81"
    shift, z = CODES[name]
    F = 3 * objects(name).group + 1
    soft = soft_of(name, "noisy", F)
    bits, rec = truth_of(name, "noisy", F, 50, T.EARLY)
    hard = (soft < 0).reshape(F, -1)
    assert (hard != bits).any() and not rec[:, 1].any() and rec[:, 0].max() < 50
    rows, cols, N, M, K = T.dims(shift, z)
    assert T.encode(shift, z, bits[:, :K].ravel(), generator_of(name)).tobytes() == bits.tobytes()


# ---- 2 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_off", (0, 1, 2, 3))
def test_any_byte_alignment(objects, mem, in_off):
    name = "4x8x27"
    c = objects(name)
    F = c.group + 1
    soft = soft_of(name, "uniform", 3 * c.group + 1)[:F * c.n]
    want_bits, want_rec = truth_of(name, "uniform", 3 * c.group + 1, 7, T.EARLY)
    for out_off in (0, 1):
        for payload in (0, T.PAYLOAD):
            bits, rec = d_decode(mem, c, soft, 7, T.EARLY | payload, True, in_off, out_off)
            assert rec.tolist() == want_rec[:F].tolist()
            assert bits.tobytes() == np.ascontiguousarray(want_bits[:F, :bits.shape[1]]).tobytes(), (in_off, out_off, payload)


# ---- 3 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("4x8x27", "12x24x81", "2x4x300"))
def test_same_bytes_twice_and_two_calls_equal_one(objects, mem, name):
    c = objects(name)
    G = c.group
    F = 3 * G + 1
    soft = soft_of(name, "noisy", F)
    one = d_decode(mem, c, soft, 7, T.EARLY)
    again = d_decode(mem, c, soft, 7, T.EARLY)
    assert one[0].tobytes() == again[0].tobytes() and one[1].tobytes() == again[1].tobytes()
    for cut in sorted({1, max(G - 1, 1), G, G + 1, F - 1}):
        a = d_decode(mem, c, soft[:cut * c.n], 7, T.EARLY)
        b = d_decode(mem, c, soft[cut * c.n:], 7, T.EARLY)
        assert a[0].tobytes() + b[0].tobytes() == one[0].tobytes() and a[1].tobytes() + b[1].tobytes() == one[1].tobytes(), cut
        mem.free()


# ---- 4 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CODES))
def test_encode_against_the_restatement(objects, mem, name):
    shift, z = CODES[name]
    c = objects(name)
    G = c.group
    Fm = 3 * G + 1 if name != "limit" else 9
    rng = np.random.default_rng(c.n)
    u = rng.integers(0, 256, Fm * c.k, dtype=np.uint8)
    u[:c.k] = 255
    want = T.encode(shift, z, u, generator_of(name)).reshape(Fm, c.n)
    for F in sorted({1, 7, 8, 9, Fm} | set(group_counts(G))):
        if F > Fm:
            continue
        for in_off, out_off in ((0, 0), (1, 3)):
            o = mem.out(F * c.n, out_off)
            _lib.check(c._lib.aeth_ldpc_encode(c.h, mem.inp(u[:F * c.k], in_off), F * c.k, mem.ptr(o), F * c.n))
            assert mem.get(o).tobytes() == want[:F].tobytes(), (name, F, in_off, out_off)
        mem.free()
    # the Python layer, and a decode of what it encoded
    coded = c.encode(u)
    assert coded.to_host().tobytes() == want.tobytes()
    soft = (64 - 128 * want.ravel().astype(np.int16)).astype(np.int8)
    bits, rec = c.decode(soft, payload=True)
    assert bits.to_host().tobytes() == (u & 1).tobytes() and rec.to_host().tolist() == [(1, 0)] * Fm


# ---- 5 -----------------------------------------------------------------------------------------------------------------
def test_refusals_launch_nothing(ctx, objects, mem):
    c = objects("3x6x5")
    N, K = c.n, c.k
    soft = mem.inp(np.zeros(2 * N, np.int8))
    o, r = mem.out(2 * N), mem.out(16, 4)
    lib = c._lib
    assert lib.aeth_ldpc_decode(c.h, soft, 2 * N - 1, 5, 0, mem.ptr(o), 2 * N, mem.ptr(r)) == _lib.E_LEN
    assert lib.aeth_ldpc_decode(c.h, soft, 2 * N, 5, 0, mem.ptr(o), 2 * K, mem.ptr(r)) == _lib.E_LEN
    assert lib.aeth_ldpc_decode(c.h, soft, 2 * N, 1001, 0, mem.ptr(o), 2 * N, mem.ptr(r)) == _lib.E_ARG
    assert lib.aeth_ldpc_decode(c.h, soft, 2 * N, 5, 4, mem.ptr(o), 2 * N, mem.ptr(r)) == _lib.E_ARG
    assert lib.aeth_ldpc_decode(c.h, soft, 2 * N, 5, 0, mem.ptr(o), 2 * N, C.c_void_p(mem.ptr(o).value + 2 * N - 4)) == _lib.E_ARG
    assert lib.aeth_ldpc_decode(c.h, soft, 2 * N, 5, 0, mem.ptr(o), 2 * N, C.c_void_p(mem.ptr(r).value + 1)) == _lib.E_ALIGN
    assert lib.aeth_ldpc_encode(c.h, soft, 2 * K, mem.ptr(o), 2 * N - 1) == _lib.E_LEN
    assert lib.aeth_ldpc_encode(c.h, soft, 2 * K + 1, mem.ptr(o), 2 * N) == _lib.E_LEN
    assert lib.aeth_ldpc_encode(c.h, mem.ptr(o), 2 * K, mem.ptr(o), 2 * N) == _lib.E_ARG
    assert lib.aeth_ldpc_decode(c.h, soft, 0, 5, 0, mem.ptr(o), 0, mem.ptr(r)) == _lib.OK          # F = 0: nothing is launched
    assert lib.aeth_ldpc_encode(c.h, soft, 0, mem.ptr(o), 0) == _lib.OK
    ctx.sync()
    assert (mem.get(o) == SENTINEL).all() and (mem.get(r) == SENTINEL).all()


def _free_bytes():
    hip = _lib.load()                              # hipMemGetInfo of the runtime the library is bound to
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_refused_creates_leave_the_free_memory_unchanged(ctx):
    singular = ldpc.staircase(3, 6, 5)
    singular[2, 3:] = singular[1, 3:]
    empty_row = ldpc.staircase(4, 8, 7)
    empty_row[2, :] = -1
    entry = ldpc.staircase(3, 6, 5)
    entry[1, 1] = 5
    big = ldpc.staircase(12, 24, 81)
    ctx.sync()
    free0 = _free_bytes()
    for _ in range(20):
        for shift, z, code, word in ((singular, 5, _lib.E_ARG, "parity part singular"), (empty_row, 7, _lib.E_ARG, "row 2"),
                                     (entry, 5, _lib.E_ARG, "shift[1][1] = 5"), (big, 1000, _lib.E_UNSUPPORTED, "65536"),
                                     (np.zeros((3, 3), np.int32), 4, _lib.E_ARG, "cols = 3")):
            with pytest.raises(ap.AetherError) as e:
                ap.Ldpc(ctx, shift, z)
            assert e.value.code == code and word in str(e.value)
    ctx.sync()
    assert _free_bytes() == free0
