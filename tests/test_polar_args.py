"""CPU: every refusal of aeth_polar_* with its code and the value it names, before any device work (the context and object
handles below are never followed past their own fields), the null behaviours, aeth_polar_rank / aeth_polar_mask against
the restatement, and the ctypes table."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from aether_primitives_amd import _lib, polar          # noqa: E402
import polar_truth as T                                # noqa: E402

FAKE = (C.c_char * 4096)()
CTX = C.cast(FAKE, C.c_void_p)           # never dereferenced: every call below returns before any device work
A = C.c_void_p(0x100000)
B = C.c_void_p(0x900000000)
D = C.c_void_p(0x1200000000)
E = C.c_void_p(0x1800000000)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


class FakePolar(C.Structure):
    """what a call reads of an object before it refuses: the context pointer and the dimensions"""
    _fields_ = [("ctx", C.c_void_p), ("n", C.c_uint32), ("N", C.c_uint32), ("K", C.c_uint32), ("T", C.c_uint32), ("G", C.c_uint32),
                ("stride", C.c_uint32), ("nsched", C.c_uint32), ("rest", C.c_uint64 * 8)]


def fake():
    return FakePolar(CTX.value, 5, 32, 12, 8, 8, 144, 9)


def create(lib, n, mask, ctx=CTX):
    m = np.ascontiguousarray(mask, np.uint8)
    h = C.c_void_p(0x55)
    rc = lib.aeth_polar_create(ctx, n, m.ctypes.data_as(C.c_void_p) if m.size else None, C.byref(h))
    return rc, h, lib.aeth_last_error().decode()


def test_null_handles_and_pointers(lib):
    good = T.mask(5, 12)
    assert lib.aeth_polar_create(CTX, 5, good.ctypes.data_as(C.c_void_p), None) == _lib.E_ARG and b"out is null" in lib.aeth_last_error()
    rc, h, msg = create(lib, 5, good, ctx=None)
    assert rc == _lib.E_ARG and "ctx is null" in msg and not h.value
    h = C.c_void_p(0x55)
    assert lib.aeth_polar_create(CTX, 5, None, C.byref(h)) == _lib.E_ARG and b"mask is null" in lib.aeth_last_error() and not h.value
    assert lib.aeth_polar_destroy(None) == _lib.OK
    for f in (lib.aeth_polar_n, lib.aeth_polar_k, lib.aeth_polar_lanes, lib.aeth_polar_group, lib.aeth_polar_lds_bytes):
        assert f(None) == 0
    assert lib.aeth_polar_encode(None, A, 12, B, 32) == _lib.E_ARG and b"polar is null" in lib.aeth_last_error()
    assert lib.aeth_polar_decode(None, A, 32, None, 0, B, 12, None) == _lib.E_ARG and b"polar is null" in lib.aeth_last_error()
    p = C.byref(fake())
    assert lib.aeth_polar_encode(p, None, 12, B, 32) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_polar_encode(p, A, 12, None, 32) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_polar_decode(p, None, 32, None, 0, B, 12, None) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_polar_decode(p, A, 32, None, 0, None, 12, None) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    # nothing to do is no refusal, and needs no pointers
    assert lib.aeth_polar_encode(p, None, 0, None, 0) == _lib.OK
    assert lib.aeth_polar_decode(p, None, 0, None, 1, None, 0, None) == _lib.OK
    # the getters read the object's own fields
    assert (lib.aeth_polar_n(p), lib.aeth_polar_k(p), lib.aeth_polar_lanes(p), lib.aeth_polar_group(p), lib.aeth_polar_lds_bytes(p)) == (32, 12, 8, 8, 8 * 144)


@pytest.mark.parametrize("n", (0, 1, 2, 11, 12, 32, 0xFFFFFFFF))
def test_n_outside_the_definition(lib, n):
    rc, h, msg = create(lib, n, np.ones(8, np.uint8))
    assert rc == _lib.E_UNSUPPORTED and f"n = {n}" in msg and "3 .. 10" in msg and not h.value
    out = np.zeros(8, np.uint32)
    assert lib.aeth_polar_rank(n, out.ctypes.data_as(C.c_void_p), 1 << 20) == _lib.E_UNSUPPORTED and f"n = {n}".encode() in lib.aeth_last_error()
    assert lib.aeth_polar_mask(n, 1, out.ctypes.data_as(C.c_void_p), 1 << 20) == _lib.E_UNSUPPORTED and f"n = {n}".encode() in lib.aeth_last_error()


@pytest.mark.parametrize("n,i,v", ((3, 0, 2), (5, 31, 255), (10, 517, 3), (7, 64, 128)))
def test_a_mask_byte_above_one(lib, n, i, v):
    m = T.mask(n, (1 << n) // 2)
    m[i] = v
    rc, h, msg = create(lib, n, m)
    assert rc == _lib.E_ARG and f"mask[{i}] = {v}" in msg and not h.value


@pytest.mark.parametrize("n", (3, 6, 10))
def test_a_mask_without_information(lib, n):
    rc, h, msg = create(lib, n, np.zeros(1 << n, np.uint8))
    assert rc == _lib.E_ARG and "K = 0" in msg and not h.value


def test_lengths(lib):
    p = C.byref(fake())
    for nbits, ncoded in ((11, 32), (13, 32), (12, 31), (12, 64), (24, 32), (0, 32), (12, 0)):
        assert lib.aeth_polar_encode(p, A, nbits, B, ncoded) == _lib.E_LEN, (nbits, ncoded)
        msg = lib.aeth_last_error().decode()
        assert str(nbits) in msg or str(ncoded) in msg, msg
    for nsoft, flags, nbits in ((31, 0, 12), (33, 0, 12), (32, 0, 32), (32, 1, 12), (64, 1, 36), (64, 0, 23), (0, 0, 12), (32, 1, 0)):
        assert lib.aeth_polar_decode(p, A, nsoft, None, flags, B, nbits, None) == _lib.E_LEN, (nsoft, flags, nbits)
        msg = lib.aeth_last_error().decode()
        assert str(nsoft) in msg or str(nbits) in msg, msg


def test_flags_alignment_and_overlap(lib):
    p = C.byref(fake())
    a = A.value
    for flags in (2, 4, 0x80000001):
        assert lib.aeth_polar_decode(p, A, 32, None, flags, B, 32 if flags & 1 else 12, None) == _lib.E_ARG
        assert f"0x{flags & ~1:x}".encode() in lib.aeth_last_error()
    for off in (1, 2, 3):
        assert lib.aeth_polar_decode(p, A, 32, C.c_void_p(E.value + off), 0, B, 12, None) == _lib.E_ALIGN
        assert b"flip_dev" in lib.aeth_last_error() and b"4-byte" in lib.aeth_last_error()
        assert lib.aeth_polar_decode(p, A, 32, None, 0, B, 12, C.c_void_p(D.value + off)) == _lib.E_ALIGN
        assert b"rec_dev" in lib.aeth_last_error() and b"4-byte" in lib.aeth_last_error()
    assert lib.aeth_polar_encode(p, A, 24, C.c_void_p(a + 23), 64) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_polar_encode(p, A, 24, C.c_void_p(a - 63), 64) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_polar_decode(p, A, 64, None, 1, C.c_void_p(a + 63), 64, None) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_polar_decode(p, A, 64, None, 0, C.c_void_p(a - 23), 24, None) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_polar_decode(p, A, 64, None, 0, B, 24, C.c_void_p(a + 60)) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_polar_decode(p, A, 64, None, 0, B, 24, C.c_void_p(B.value - 60)) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_polar_decode(p, A, 64, C.c_void_p(B.value + 20), 0, B, 24, None) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_polar_decode(p, A, 64, E, 0, B, 24, C.c_void_p(E.value + 4)) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()


@pytest.mark.parametrize("n", range(3, 11))
def test_rank_and_mask_through_the_library(lib, n):
    N = 1 << n
    assert polar.rank(n).tolist() == T.rank(n).tolist()
    for K in (1, 2, N // 2, N - 1, N):
        assert polar.mask(n, K).tobytes() == T.mask(n, K).tobytes(), (n, K)
    out = np.full(N + 4, 0xA5, np.uint8)
    for K in (0, N + 1, 0xFFFFFFFF):
        assert lib.aeth_polar_mask(n, K, out.ctypes.data_as(C.c_void_p), N) == _lib.E_ARG and f"K = {K}".encode() in lib.aeth_last_error()
    assert lib.aeth_polar_mask(n, 1, out.ctypes.data_as(C.c_void_p), N - 1) == _lib.E_LEN and str(N - 1).encode() in lib.aeth_last_error()
    assert lib.aeth_polar_mask(n, 1, None, N) == _lib.E_ARG and b"mask_out is null" in lib.aeth_last_error()
    order = np.full(N + 4, 0xA5A5A5A5, np.uint32)
    assert lib.aeth_polar_rank(n, order.ctypes.data_as(C.c_void_p), N - 1) == _lib.E_LEN and str(N - 1).encode() in lib.aeth_last_error()
    assert lib.aeth_polar_rank(n, None, N) == _lib.E_ARG and b"order_out is null" in lib.aeth_last_error()
    assert (out == 0xA5).all() and (order == 0xA5A5A5A5).all(), "a refused call wrote"
    assert lib.aeth_polar_mask(n, N // 2, out.ctypes.data_as(C.c_void_p), N) == _lib.OK and (out[N:] == 0xA5).all()
    assert lib.aeth_polar_rank(n, order.ctypes.data_as(C.c_void_p), N) == _lib.OK and (order[N:] == 0xA5A5A5A5).all()


def test_the_two_literal_orders(lib):
    assert polar.rank(3).tolist() == [7, 6, 5, 3, 4, 2, 1, 0]
    assert polar.rank(4).tolist() == [15, 14, 13, 11, 7, 12, 10, 9, 6, 5, 3, 8, 4, 2, 1, 0]


def test_ctypes_table_and_python_mirror():
    import aether_primitives_amd as ap
    for name in ("aeth_polar_rank", "aeth_polar_mask", "aeth_polar_create", "aeth_polar_destroy", "aeth_polar_n", "aeth_polar_k",
                 "aeth_polar_lanes", "aeth_polar_group", "aeth_polar_lds_bytes", "aeth_polar_encode", "aeth_polar_decode"):
        assert name in _lib.PROTOTYPES and hasattr(_lib.load(), name), name
    for name in ("encode", "decode", "close", "n", "k", "lanes", "group", "lds_bytes"):
        assert hasattr(ap.Polar, name), name
    for name in ("polar", "Polar"):
        assert name in ap.__all__, name
    assert (ap.polar.CODEWORD, ap.polar.NONE) == (1, 0xFFFFFFFF)
    assert ap.polar.RECORD.itemsize == 32 and ap.polar.RECORD == T.RECORD
    assert ap.polar.RECORD.fields["index"][1] == 0 and ap.polar.RECORD.fields["abs"][1] == 16
