"""CPU: every refusal of aeth_turbo_* with its code and the value it names, before any device work (the context and object
handles below are never followed past their own fields), the order of consecutive checks, overlap pairs, the grid
refusal, the null behaviours, aeth_turbo_qpp / aeth_turbo_named against the restatement, and the ctypes table."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from aether_primitives_amd import _lib, turbo          # noqa: E402
import turbo_truth as T                                # noqa: E402

FAKE = (C.c_char * 4096)()
CTX = C.cast(FAKE, C.c_void_p)           # never dereferenced: every call below returns before any device work
A = C.c_void_p(0x100000)
B = C.c_void_p(0x900000000)
D = C.c_void_p(0x1200000000)
FAR = C.c_void_p(0x40000000000)
K, NU, N = 40, 3, 3 * 40 + 4 * 3         # the fake object: the lte code at K = 40


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


class FakeTurbo(C.Structure):
    """what a call reads of an object before it refuses: the context pointer and the dimensions"""
    _fields_ = [("ctx", C.c_void_p), ("K", C.c_uint32), ("N", C.c_uint32), ("k", C.c_uint32), ("S", C.c_uint32), ("W", C.c_uint32),
                ("A", C.c_uint32), ("nwin", C.c_uint32), ("G", C.c_uint32), ("cwb", C.c_uint32), ("slots", C.c_uint32), ("slab", C.c_uint64),
                ("code", C.c_uint32 * 3), ("rest", C.c_uint64 * 8)]


def fake(G=4):
    return FakeTurbo(CTX.value, K, N, 4, 8, 16, 8, 3, G, 332, 1, 3 * 16 * 8 * G, (C.c_uint32 * 3)(4, 0o13, 0o15))


def create(lib, code, k, pi, W, Aw, ctx=CTX):
    c = turbo.Code(*code) if code is not None else None
    p = np.ascontiguousarray(pi, np.uint32) if pi is not None else None
    h = C.c_void_p(0x55)
    rc = lib.aeth_turbo_create(ctx, C.byref(c) if c is not None else None, k, p.ctypes.data_as(C.c_void_p) if p is not None else None, W, Aw,
                               C.byref(h))
    return rc, h, lib.aeth_last_error().decode()


LTE = (4, 0o13, 0o15)
PI40 = T.qpp(40, 3, 10)


def test_null_handles_and_pointers(lib):
    c = turbo.Code(*LTE)
    assert lib.aeth_turbo_create(CTX, C.byref(c), 40, PI40.ctypes.data_as(C.c_void_p), 16, 8, None) == _lib.E_ARG
    assert b"out is null" in lib.aeth_last_error()
    rc, h, msg = create(lib, LTE, 40, PI40, 16, 8, ctx=None)
    assert rc == _lib.E_ARG and "ctx is null" in msg and not h.value
    rc, h, msg = create(lib, None, 40, PI40, 16, 8)
    assert rc == _lib.E_ARG and "code is null" in msg and not h.value
    rc, h, msg = create(lib, LTE, 40, None, 16, 8)
    assert rc == _lib.E_ARG and "pi is null" in msg and not h.value
    assert lib.aeth_turbo_destroy(None) == _lib.OK
    for f in (lib.aeth_turbo_k, lib.aeth_turbo_n, lib.aeth_turbo_states, lib.aeth_turbo_window, lib.aeth_turbo_warmup, lib.aeth_turbo_windows,
              lib.aeth_turbo_group, lib.aeth_turbo_lds_bytes):
        assert f(None) == 0
    assert lib.aeth_turbo_encode(None, A, K, B, N) == _lib.E_ARG and b"turbo is null" in lib.aeth_last_error()
    assert lib.aeth_turbo_decode(None, A, N, 1, 0, B, K, None) == _lib.E_ARG and b"turbo is null" in lib.aeth_last_error()
    p = C.byref(fake())
    assert lib.aeth_turbo_encode(p, None, K, B, N) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_turbo_encode(p, A, K, None, N) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_turbo_decode(p, None, N, 1, 0, B, K, None) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_turbo_decode(p, A, N, 1, 0, None, K, None) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    # nothing to do is no refusal, and needs no pointers
    assert lib.aeth_turbo_encode(p, None, 0, None, 0) == _lib.OK
    assert lib.aeth_turbo_decode(p, None, 0, 8, 1, None, 0, None) == _lib.OK
    # the getters read the object's own fields
    got = (lib.aeth_turbo_k(p), lib.aeth_turbo_n(p), lib.aeth_turbo_states(p), lib.aeth_turbo_window(p), lib.aeth_turbo_warmup(p),
           lib.aeth_turbo_windows(p), lib.aeth_turbo_group(p), lib.aeth_turbo_lds_bytes(p))
    assert got == (K, N, 8, 16, 8, 3, 4, 4 * (132 + 40 + 160) + 4 * 8 + 8)


@pytest.mark.parametrize("k", (0, 1, 2, 6, 7, 32, 0xFFFFFFFF))
def test_constraint_length_outside_the_definition(lib, k):
    rc, h, msg = create(lib, (k, 0o13, 0o15), 40, PI40, 16, 8)
    assert rc == _lib.E_UNSUPPORTED and f"k = {k}" in msg and "3 .. 5" in msg and not h.value


@pytest.mark.parametrize("k,fb,ff,which", ((4, 0o03, 0o15, "fb"), (4, 0o12, 0o15, "fb"), (4, 0o33, 0o15, "fb"), (4, 0, 0o15, "fb"),
                                           (4, 0o13, 0o14, "ff"), (4, 0o13, 0o35, "ff"), (4, 0o13, 0, "ff"), (3, 0o13, 0o5, "fb"),
                                           (5, 0o13, 0o33, "fb"), (5, 0o23, 0o73, "ff"), (3, 0o7, 0o15, "ff")))
def test_bad_polynomials(lib, k, fb, ff, which):
    rc, h, msg = create(lib, (k, fb, ff), 40, PI40, 16, 8)
    bad = fb if which == "fb" else ff
    assert rc == _lib.E_ARG and f"{which} = 0{bad:o}" in msg and not h.value


@pytest.mark.parametrize("Kb", (0, 1, 7, 8193, 1 << 20, 0xFFFFFFFF))
def test_frame_length_outside_the_definition(lib, Kb):
    rc, h, msg = create(lib, LTE, Kb, PI40, 16, 8)
    assert rc == _lib.E_ARG and f"K = {Kb}" in msg and "8 .. 8192" in msg and not h.value
    out = np.full(8, 0xA5A5A5A5, np.uint32)
    assert lib.aeth_turbo_qpp(Kb, 3, 10, out.ctypes.data_as(C.c_void_p), 1 << 20) == _lib.E_ARG and f"K = {Kb}".encode() in lib.aeth_last_error()
    assert (out == 0xA5A5A5A5).all()


def test_window_and_warmup(lib):
    rc, h, msg = create(lib, LTE, 40, PI40, 0, 8)
    assert rc == _lib.E_ARG and "window = 0" in msg and not h.value
    for Aw in (8193, 1 << 20, 0xFFFFFFFF):
        rc, h, msg = create(lib, LTE, 40, PI40, 16, Aw)
        assert rc == _lib.E_ARG and f"warmup = {Aw}" in msg and "8192" in msg and not h.value


@pytest.mark.parametrize("i,v", ((0, 40), (39, 41), (17, 0xFFFFFFFF), (5, 1 << 16)))
def test_an_interleaver_entry_outside_the_frame(lib, i, v):
    pi = PI40.copy()
    pi[i] = v
    rc, h, msg = create(lib, LTE, 40, pi, 16, 8)
    assert rc == _lib.E_ARG and f"pi[{i}] = {v}" in msg and "K = 40" in msg and not h.value


@pytest.mark.parametrize("i,j", ((1, 0), (39, 38), (20, 3)))
def test_a_repeated_interleaver_entry(lib, i, j):
    pi = PI40.copy()
    pi[i] = pi[j]
    rc, h, msg = create(lib, LTE, 40, pi, 16, 8)
    assert rc == _lib.E_ARG and f"pi[{i}] = {pi[j]}" in msg and f"pi[{j}]" in msg and "repeats" in msg and not h.value


@pytest.mark.parametrize("Kb,W,n", ((8192, 7, 1171), (8192, 1, 8192), (1025, 1, 1025), (4100, 4, 1025)))
def test_more_than_1024_windows(lib, Kb, W, n):
    rc, h, msg = create(lib, LTE, Kb, np.arange(Kb, dtype=np.uint32), W, 0)
    assert rc == _lib.E_UNSUPPORTED and f"{n} windows" in msg and f"K = {Kb}" in msg and "1024" in msg and not h.value


def test_order_of_the_create_checks(lib):
    """a call wrong in two consecutive ways gets the earlier refusal"""
    dup = PI40.copy()
    dup[1] = dup[0]
    rows = (((9, 0, 0o15), 40, PI40, 16, 8, _lib.E_UNSUPPORTED, "k = 9"),
            ((4, 0o12, 0o14), 40, PI40, 16, 8, _lib.E_ARG, "fb = 012"),
            ((4, 0o13, 0o14), 7, PI40, 16, 8, _lib.E_ARG, "ff = 014"),
            (LTE, 7, PI40, 0, 8, _lib.E_ARG, "K = 7"),
            (LTE, 40, PI40, 0, 9000, _lib.E_ARG, "window = 0"),
            (LTE, 40, None, 16, 9000, _lib.E_ARG, "warmup = 9000"),
            (LTE, 8192, None, 1, 0, _lib.E_ARG, "pi is null"),
            (LTE, 40, dup, 16, 8, _lib.E_ARG, "repeats"))
    for code, Kb, pi, W, Aw, want, text in rows:
        rc, h, msg = create(lib, code, Kb, pi, W, Aw)
        assert rc == want and text in msg and not h.value, (text, msg)
    big = np.arange(8192, dtype=np.uint32)
    big[5] = 9999
    rc, h, msg = create(lib, LTE, 8192, big, 1, 0)
    assert rc == _lib.E_ARG and "pi[5] = 9999" in msg


def test_lengths(lib):
    p = C.byref(fake())
    for nbits, ncoded in ((K - 1, N), (K + 1, N), (K, N - 1), (K, 2 * N), (2 * K, N), (0, N), (K, 0)):
        assert lib.aeth_turbo_encode(p, A, nbits, B, ncoded) == _lib.E_LEN, (nbits, ncoded)
        msg = lib.aeth_last_error().decode()
        assert str(nbits) in msg or str(ncoded) in msg, msg
    for nsoft, nbits in ((N - 1, K), (N + 1, K), (N, K - 1), (N, N), (2 * N, K), (2 * N, 2 * K + 1), (0, K), (N, 0)):
        assert lib.aeth_turbo_decode(p, A, nsoft, 1, 0, B, nbits, None) == _lib.E_LEN, (nsoft, nbits)
        msg = lib.aeth_last_error().decode()
        assert str(nsoft) in msg or str(nbits) in msg, msg


def test_iterations_flags_alignment_and_overlap(lib):
    p = C.byref(fake())
    a = A.value
    for it in (0, 65, 1000, 0xFFFFFFFF):
        assert lib.aeth_turbo_decode(p, A, N, it, 0, B, K, None) == _lib.E_ARG
        assert f"max_iter {it}".encode() in lib.aeth_last_error() and b"1 .. 64" in lib.aeth_last_error()
    for flags in (2, 4, 0x80000001):
        assert lib.aeth_turbo_decode(p, A, N, 1, flags, B, K, None) == _lib.E_ARG
        assert f"0x{flags & ~1:x}".encode() in lib.aeth_last_error()
    for off in (1, 2, 3):
        assert lib.aeth_turbo_decode(p, A, N, 1, 0, B, K, C.c_void_p(D.value + off)) == _lib.E_ALIGN
        assert b"rec_dev" in lib.aeth_last_error() and b"4-byte" in lib.aeth_last_error()
    # every (output, input) and (output, output) pair sharing one byte at either end
    assert lib.aeth_turbo_encode(p, A, 2 * K, C.c_void_p(a + 2 * K - 1), 2 * N) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_turbo_encode(p, A, 2 * K, C.c_void_p(a - 2 * N + 1), 2 * N) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_turbo_decode(p, A, 2 * N, 1, 0, C.c_void_p(a + 2 * N - 1), 2 * K, None) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_turbo_decode(p, A, 2 * N, 1, 0, C.c_void_p(a - 2 * K + 1), 2 * K, None) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_turbo_decode(p, A, 2 * N, 1, 0, B, 2 * K, C.c_void_p(a + 2 * N - 4)) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_turbo_decode(p, A, 2 * N, 1, 0, B, 2 * K, C.c_void_p(a - 12)) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_turbo_decode(p, A, 2 * N, 1, 0, B, 2 * K, C.c_void_p(B.value + 2 * K - 4)) == _lib.E_ARG
    assert b"outputs overlap" in lib.aeth_last_error()
    assert lib.aeth_turbo_decode(p, A, 2 * N, 1, 0, B, 2 * K, C.c_void_p(B.value - 12)) == _lib.E_ARG and b"outputs overlap" in lib.aeth_last_error()


def test_order_of_the_decode_checks(lib):
    p = C.byref(fake())
    assert lib.aeth_turbo_decode(p, A, N - 1, 0, 2, B, K, None) == _lib.E_ARG and b"max_iter 0" in lib.aeth_last_error()
    assert lib.aeth_turbo_decode(p, A, N - 1, 1, 2, B, K, None) == _lib.E_ARG and b"flag" in lib.aeth_last_error()
    assert lib.aeth_turbo_decode(p, None, N - 1, 1, 0, B, K, None) == _lib.E_LEN
    assert lib.aeth_turbo_decode(p, None, N, 1, 0, B, K, C.c_void_p(D.value + 1)) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_turbo_decode(p, A, N, 1, 0, A, K, C.c_void_p(D.value + 1)) == _lib.E_ALIGN
    # an overlap in a call that would also need 2^31 workgroups
    one = C.byref(fake(G=1))
    F = 1 << 31
    assert lib.aeth_turbo_decode(one, A, F * N, 1, 0, C.c_void_p(A.value + 8), F * K, None) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_turbo_encode(p, None, K + 1, B, N) == _lib.E_LEN
    assert lib.aeth_turbo_encode(p, A, K, A, N) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()


def test_grid_refusal(lib):
    one = C.byref(fake(G=1))
    for F in (1 << 31, (1 << 31) + 5, 1 << 33):
        assert lib.aeth_turbo_decode(one, A, F * N, 1, 0, FAR, F * K, None) == _lib.E_UNSUPPORTED
        msg = lib.aeth_last_error().decode()
        assert f"{F} codewords" in msg and "2^31" in msg
    four = C.byref(fake(G=4))
    F = 4 << 31
    assert lib.aeth_turbo_decode(four, A, (F + 1) * N, 1, 0, FAR, (F + 1) * K, None) == _lib.E_UNSUPPORTED
    F = 1 << 36                                                     # the encoder: two lanes per codeword, 64 per workgroup
    assert lib.aeth_turbo_encode(one, A, F * K, FAR, F * N) == _lib.E_UNSUPPORTED and f"{F} codewords".encode() in lib.aeth_last_error()


@pytest.mark.parametrize("Kb,f1,f2", ((40, 3, 10), (64, 7, 16), (128, 15, 32), (512, 31, 64), (1024, 31, 64), (6144, 263, 480), (8, 3, 4),
                                      (8192, 31, 64), (40, 3 + 40 * 100000000, 10), (6144, 263 + 6144 * 1000, 480 + 6144 * 600000)))
def test_qpp_through_the_library(lib, Kb, f1, f2):
    want = T.qpp(Kb, f1, f2)
    assert want is not None
    assert turbo.qpp(Kb, f1, f2).tolist() == want.tolist()
    out = np.full(Kb + 4, 0xA5A5A5A5, np.uint32)
    assert lib.aeth_turbo_qpp(Kb, f1, f2, out.ctypes.data_as(C.c_void_p), Kb - 1) == _lib.E_LEN and str(Kb - 1).encode() in lib.aeth_last_error()
    assert lib.aeth_turbo_qpp(Kb, f1, f2, None, Kb) == _lib.E_ARG and b"pi_out is null" in lib.aeth_last_error()
    assert (out == 0xA5A5A5A5).all(), "a refused call wrote"
    assert lib.aeth_turbo_qpp(Kb, f1, f2, out.ctypes.data_as(C.c_void_p), Kb) == _lib.OK and (out[Kb:] == 0xA5A5A5A5).all()


@pytest.mark.parametrize("Kb,f1,f2", ((40, 2, 10), (40, 5, 10), (64, 2, 16), (8, 0, 0)))
def test_qpp_refuses_what_is_no_permutation(lib, Kb, f1, f2):
    assert T.qpp(Kb, f1, f2) is None
    out = np.full(Kb, 0xA5A5A5A5, np.uint32)
    assert lib.aeth_turbo_qpp(Kb, f1, f2, out.ctypes.data_as(C.c_void_p), Kb) == _lib.E_ARG
    msg = lib.aeth_last_error().decode()
    assert "repeats" in msg and "pi[" in msg and (out == 0xA5A5A5A5).all()
    pi = [(f1 * i + f2 * i * i) % Kb for i in range(Kb)]
    i = next(i for i in range(Kb) if pi[i] in pi[:i])
    assert f"pi[{i}] = {pi[i]} repeats pi[{pi.index(pi[i])}]" in msg


def test_named_through_the_library(lib):
    for name, want in T.NAMED.items():
        assert turbo.named(name) == want
    c = turbo.Code(9, 9, 9)
    for name in (b"", b"LTE", b"umts", b"lte "):
        assert lib.aeth_turbo_named(name, C.byref(c)) == _lib.E_ARG and name in lib.aeth_last_error()
    assert (c.k, c.fb, c.ff) == (9, 9, 9)
    assert lib.aeth_turbo_named(None, C.byref(c)) == _lib.E_ARG and b"name is null" in lib.aeth_last_error()
    assert lib.aeth_turbo_named(b"lte", None) == _lib.E_ARG and b"code_out is null" in lib.aeth_last_error()


def test_ctypes_table_and_python_mirror():
    import aether_primitives_amd as ap
    for name in ("aeth_turbo_named", "aeth_turbo_qpp", "aeth_turbo_create", "aeth_turbo_destroy", "aeth_turbo_k", "aeth_turbo_n",
                 "aeth_turbo_states", "aeth_turbo_window", "aeth_turbo_warmup", "aeth_turbo_windows", "aeth_turbo_group", "aeth_turbo_lds_bytes",
                 "aeth_turbo_encode", "aeth_turbo_decode"):
        assert name in _lib.PROTOTYPES and hasattr(_lib.load(), name), name
    for name in ("encode", "decode", "close", "k", "n", "states", "window", "warmup", "windows", "group", "lds_bytes"):
        assert hasattr(ap.Turbo, name), name
    for name in ("turbo", "Turbo"):
        assert name in ap.__all__, name
    assert ap.turbo.EARLY == 1 == T.EARLY
    assert ap.turbo.RECORD.itemsize == 8 and ap.turbo.RECORD == T.RECORD
    assert ap.turbo.RECORD.fields["iterations"][1] == 0 and ap.turbo.RECORD.fields["disagreements"][1] == 4
    assert C.sizeof(ap.turbo.Code) == 12
    assert issubclass(ap.turbo.DeviceRecords, ap._device.DeviceArray) and issubclass(ap.Turbo, ap._device.Handle)
