"""CPU: every refusal of aeth_polar_list_* with its code and the value it names, before any device work (the context and
object handles below are never followed past their own fields), the null behaviours and the ctypes table."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from aether_primitives_amd import _lib                 # noqa: E402
import polar_truth as T                                # noqa: E402
import polar_list_truth as LT                          # noqa: E402

FAKE = (C.c_char * 4096)()
CTX = C.cast(FAKE, C.c_void_p)           # never dereferenced: every call below returns before any device work
A = C.c_void_p(0x100000)
B = C.c_void_p(0x900000000)
D = C.c_void_p(0x1200000000)
E = C.c_void_p(0x1800000000)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


class FakeList(C.Structure):
    """what a call reads of an object before it refuses: the context pointer and the dimensions"""
    _fields_ = [("ctx", C.c_void_p), ("n", C.c_uint32), ("N", C.c_uint32), ("K", C.c_uint32), ("L", C.c_uint32), ("T", C.c_uint32),
                ("G", C.c_uint32), ("stride", C.c_uint32), ("nsched", C.c_uint32), ("rest", C.c_uint64 * 8)]


def fake():
    return FakeList(CTX.value, 5, 32, 12, 4, 16, 1, 160, 9)


def create(lib, n, mask, L, ctx=CTX):
    m = np.ascontiguousarray(mask, np.uint8)
    h = C.c_void_p(0x55)
    rc = lib.aeth_polar_list_create(ctx, n, m.ctypes.data_as(C.c_void_p) if m.size else None, L, C.byref(h))
    return rc, h, lib.aeth_last_error().decode()


def test_null_handles_and_pointers(lib):
    good = T.mask(5, 12)
    assert lib.aeth_polar_list_create(CTX, 5, good.ctypes.data_as(C.c_void_p), 4, None) == _lib.E_ARG and b"out is null" in lib.aeth_last_error()
    rc, h, msg = create(lib, 5, good, 4, ctx=None)
    assert rc == _lib.E_ARG and "ctx is null" in msg and not h.value
    h = C.c_void_p(0x55)
    assert lib.aeth_polar_list_create(CTX, 5, None, 4, C.byref(h)) == _lib.E_ARG and b"mask is null" in lib.aeth_last_error() and not h.value
    assert lib.aeth_polar_list_destroy(None) == _lib.OK
    for f in (lib.aeth_polar_list_n, lib.aeth_polar_list_k, lib.aeth_polar_list_paths, lib.aeth_polar_list_lanes, lib.aeth_polar_list_group,
              lib.aeth_polar_list_lds_bytes):
        assert f(None) == 0
    assert lib.aeth_polar_list_decode(None, A, 32, 0, B, 12, None) == _lib.E_ARG and b"polar list is null" in lib.aeth_last_error()
    p = C.byref(fake())
    assert lib.aeth_polar_list_decode(p, None, 32, 0, B, 12, None) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_polar_list_decode(p, A, 32, 0, None, 12, None) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_polar_list_decode(p, None, 0, 3, None, 0, None) == _lib.OK          # nothing to do is no refusal
    assert (lib.aeth_polar_list_n(p), lib.aeth_polar_list_k(p), lib.aeth_polar_list_paths(p), lib.aeth_polar_list_lanes(p),
            lib.aeth_polar_list_group(p), lib.aeth_polar_list_lds_bytes(p)) == (32, 12, 4, 16, 1, 4 * 164)
    assert lib.aeth_polar_list_pick(None, A, 12, 1, 4, D, B, None) == _lib.E_ARG and b"ctx is null" in lib.aeth_last_error()
    for rows, diff, out in ((None, D, B), (A, None, B), (A, D, None)):
        assert lib.aeth_polar_list_pick(CTX, rows, 12, 1, 4, diff, out, None) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_polar_list_pick(CTX, None, 12, 0, 4, None, None, None) == _lib.OK


@pytest.mark.parametrize("L", (0, 3, 5, 6, 7, 9, 16, 0xFFFFFFFF))
def test_a_list_size_outside_the_definition(lib, L):
    rc, h, msg = create(lib, 5, T.mask(5, 12), L)
    assert rc == _lib.E_ARG and f"L = {L}" in msg and "1, 2, 4 or 8" in msg and not h.value


@pytest.mark.parametrize("K,L", ((1, 4), (1, 8), (2, 8)))
def test_fewer_codewords_than_paths(lib, K, L):
    rc, h, msg = create(lib, 4, T.mask(4, K), L)
    assert rc == _lib.E_ARG and f"K = {K}" in msg and f"L = {L}" in msg and f"{1 << K} words" in msg and not h.value


def test_the_code_is_checked_as_for_the_sc_decoder(lib):
    for n in (0, 2, 11, 0xFFFFFFFF):
        rc, h, msg = create(lib, n, np.ones(8, np.uint8), 2)
        assert rc == _lib.E_UNSUPPORTED and f"n = {n}" in msg and "3 .. 10" in msg and not h.value
    m = T.mask(5, 16)
    m[31] = 3
    rc, h, msg = create(lib, 5, m, 2)
    assert rc == _lib.E_ARG and "mask[31] = 3" in msg and not h.value
    rc, h, msg = create(lib, 6, np.zeros(64, np.uint8), 1)
    assert rc == _lib.E_ARG and "K = 0" in msg and not h.value


def test_lengths_for_each_flag_combination(lib):
    p = C.byref(fake())                                             # N = 32, K = 12, L = 4
    right = {0: 12, LT.CODEWORD: 32, LT.ALL: 48, LT.ALL | LT.CODEWORD: 128}
    for flags, per in right.items():
        for nsoft, nbits in ((31, per), (33, per), (32, per - 1), (32, per + 1), (64, per), (64, 2 * per + 1), (0, per), (32, 0)):
            assert lib.aeth_polar_list_decode(p, A, nsoft, flags, B, nbits, None) == _lib.E_LEN, (flags, nsoft, nbits)
            msg = lib.aeth_last_error().decode()
            assert str(nsoft) in msg or str(nbits) in msg, msg
        for other in right.values():
            if other != per:
                assert lib.aeth_polar_list_decode(p, A, 32, flags, B, other, None) == _lib.E_LEN, (flags, other)


def test_flags_alignment_and_overlap(lib):
    p = C.byref(fake())
    a = A.value
    for flags in (4, 8, 0x80000001, 0x10):
        assert lib.aeth_polar_list_decode(p, A, 32, flags, B, 12, None) == _lib.E_ARG
        assert f"0x{flags & ~3:x}".encode() in lib.aeth_last_error()
    for off in (1, 2, 3):
        assert lib.aeth_polar_list_decode(p, A, 32, 0, B, 12, C.c_void_p(D.value + off)) == _lib.E_ALIGN
        assert b"rec_dev" in lib.aeth_last_error() and b"4-byte" in lib.aeth_last_error()
    assert lib.aeth_polar_list_decode(p, A, 64, 1, C.c_void_p(a + 63), 64, None) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_polar_list_decode(p, A, 64, 0, C.c_void_p(a - 23), 24, None) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_polar_list_decode(p, A, 64, 2, C.c_void_p(a - 95), 96, None) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_polar_list_decode(p, A, 64, 0, B, 24, C.c_void_p(a + 60)) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_polar_list_decode(p, A, 64, 0, B, 24, C.c_void_p(B.value - 60)) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_polar_list_decode(p, A, 64, 3, B, 256, C.c_void_p(B.value + 252)) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()


def test_pick_refusals(lib):
    for L in (0, 9, 0xFFFFFFFF):
        assert lib.aeth_polar_list_pick(CTX, A, 12, 3, L, D, B, E) == _lib.E_ARG and f"L = {L}".encode() in lib.aeth_last_error()
    assert lib.aeth_polar_list_pick(CTX, A, 0, 3, 4, D, B, E) == _lib.E_LEN and b"row_bytes = 0" in lib.aeth_last_error()
    assert lib.aeth_polar_list_pick(CTX, A, (1 << 30) + 1, 3, 4, D, B, E) == _lib.E_UNSUPPORTED and str((1 << 30) + 1).encode() in lib.aeth_last_error()
    for off in (1, 2, 4, 7):
        assert lib.aeth_polar_list_pick(CTX, A, 12, 3, 4, C.c_void_p(D.value + off), B, E) == _lib.E_ALIGN
        assert b"diff_dev" in lib.aeth_last_error() and b"8-byte" in lib.aeth_last_error()
    for off in (1, 2, 3):
        assert lib.aeth_polar_list_pick(CTX, A, 12, 3, 4, D, B, C.c_void_p(E.value + off)) == _lib.E_ALIGN
        assert b"which_dev" in lib.aeth_last_error() and b"4-byte" in lib.aeth_last_error()
    a, d = A.value, D.value
    # rows: 3 x 4 x 12 = 144 bytes, diff 96, out 36, which 12
    assert lib.aeth_polar_list_pick(CTX, A, 12, 3, 4, D, C.c_void_p(a + 143), E) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_polar_list_pick(CTX, A, 12, 3, 4, D, C.c_void_p(a - 35), E) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_polar_list_pick(CTX, A, 12, 3, 4, D, C.c_void_p(d + 95), E) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_polar_list_pick(CTX, A, 12, 3, 4, D, B, C.c_void_p(a + 140)) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_polar_list_pick(CTX, A, 12, 3, 4, D, B, C.c_void_p(d + 92)) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_polar_list_pick(CTX, A, 12, 3, 4, D, B, C.c_void_p(B.value + 32)) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_polar_list_pick(CTX, A, 1 << 30, 1 << 20, 8, D, B, E) == _lib.E_LEN and b"2^48" in lib.aeth_last_error()


def test_ctypes_table_and_python_mirror():
    import aether_primitives_amd as ap
    for name in ("aeth_polar_list_create", "aeth_polar_list_destroy", "aeth_polar_list_n", "aeth_polar_list_k", "aeth_polar_list_paths",
                 "aeth_polar_list_lanes", "aeth_polar_list_group", "aeth_polar_list_lds_bytes", "aeth_polar_list_decode", "aeth_polar_list_pick"):
        assert name in _lib.PROTOTYPES and hasattr(_lib.load(), name), name
    for name in ("decode", "close", "n", "k", "paths", "lanes", "group", "lds_bytes"):
        assert hasattr(ap.PolarList, name), name
    assert "PolarList" in ap.__all__ and issubclass(ap.PolarList, ap._device.Handle)
    assert (ap.polar.CODEWORD, ap.polar.ALL, ap.polar.NONE) == (1, 2, 0xFFFFFFFF)
    assert ap.polar.LIST_RECORD.itemsize == 32 and ap.polar.LIST_RECORD == LT.LIST_RECORD
    assert issubclass(ap.polar.DeviceListRecords, ap._device.DeviceArray) and callable(ap.polar.pick)
