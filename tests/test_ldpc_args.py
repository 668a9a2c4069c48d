"""CPU: every refusal of aeth_ldpc_* with its code and the value it names, before any device work (the context and object
handles below are never followed past their own fields), the null behaviours, the 64 KiB state boundary on both sides,
and the ctypes table."""
import ctypes as C

import numpy as np
import pytest

from aether_primitives_amd import _lib, ldpc

FAKE = (C.c_char * 4096)()
CTX = C.cast(FAKE, C.c_void_p)           # never dereferenced: every call below returns before any device work
A = C.c_void_p(0x100000)
B = C.c_void_p(0x900000000)
D = C.c_void_p(0x1200000000)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


class FakeLdpc(C.Structure):
    """what a call reads of an object before it refuses: the context pointer and the dimensions"""
    _fields_ = [("ctx", C.c_void_p), ("rows", C.c_uint32), ("cols", C.c_uint32), ("z", C.c_uint32), ("N", C.c_uint32), ("M", C.c_uint32),
                ("K", C.c_uint32), ("E", C.c_uint32), ("G", C.c_uint32), ("KW", C.c_uint32), ("rest", C.c_uint64 * 8)]


def fake():
    return FakeLdpc(CTX.value, 3, 6, 5, 30, 15, 15, 14, 51, 1)


def create(lib, shift, z, ctx=CTX):
    code, tab = ldpc._code(shift, z)
    h = C.c_void_p(0x55)
    rc = lib.aeth_ldpc_create(ctx, C.byref(code), C.byref(h))
    return rc, h, lib.aeth_last_error().decode()


def gen(lib, shift, z, nwords=0):
    """aeth_ldpc_generator with room for `nwords` words: everything but the elimination happens in front of the length check"""
    code, tab = ldpc._code(shift, z)
    buf = np.zeros(max(nwords, 1), np.uint64)
    rc = lib.aeth_ldpc_generator(C.byref(code), buf.ctypes.data_as(C.c_void_p), nwords)
    return rc, lib.aeth_last_error().decode()


def both(lib, shift, z, code, *words):
    """create and generator refuse alike"""
    rc, h, msg = create(lib, shift, z)
    assert rc == code and not h.value and all(w in msg for w in words), msg
    rc, msg = gen(lib, shift, z, 1 << 16)
    assert rc == code and all(w in msg for w in words), msg


def test_null_handles_and_pointers(lib):
    good = ldpc.staircase(3, 6, 5)
    code, tab = ldpc._code(good, 5)
    assert lib.aeth_ldpc_create(CTX, C.byref(code), None) == _lib.E_ARG and b"out is null" in lib.aeth_last_error()
    rc, h, msg = create(lib, good, 5, ctx=None)
    assert rc == _lib.E_ARG and "ctx is null" in msg and not h.value
    h = C.c_void_p(0x55)
    assert lib.aeth_ldpc_create(CTX, None, C.byref(h)) == _lib.E_ARG and b"code is null" in lib.aeth_last_error() and not h.value
    null_tab = ldpc.Code(3, 6, 5, None)
    assert lib.aeth_ldpc_create(CTX, C.byref(null_tab), C.byref(h)) == _lib.E_ARG and b"shift is null" in lib.aeth_last_error()
    assert lib.aeth_ldpc_generator(None, A, 100) == _lib.E_ARG and b"code is null" in lib.aeth_last_error()
    assert lib.aeth_ldpc_generator(C.byref(code), None, 100) == _lib.E_ARG and b"p_out is null" in lib.aeth_last_error()
    assert lib.aeth_ldpc_destroy(None) == _lib.OK
    for f in (lib.aeth_ldpc_n, lib.aeth_ldpc_k, lib.aeth_ldpc_rows, lib.aeth_ldpc_cols, lib.aeth_ldpc_z, lib.aeth_ldpc_edges,
              lib.aeth_ldpc_lds_bytes, lib.aeth_ldpc_group):
        assert f(None) == 0
    assert lib.aeth_ldpc_encode(None, A, 15, B, 30) == _lib.E_ARG and b"ldpc is null" in lib.aeth_last_error()
    assert lib.aeth_ldpc_decode(None, A, 30, 1, 0, B, 30, None) == _lib.E_ARG and b"ldpc is null" in lib.aeth_last_error()
    p = C.byref(fake())
    assert lib.aeth_ldpc_encode(p, None, 15, B, 30) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_ldpc_encode(p, A, 15, None, 30) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_ldpc_decode(p, None, 30, 1, 0, B, 30, None) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_ldpc_decode(p, A, 30, 1, 0, None, 30, None) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    # nothing to do is no refusal, and needs no pointers
    assert lib.aeth_ldpc_encode(p, None, 0, None, 0) == _lib.OK
    assert lib.aeth_ldpc_decode(p, None, 0, 20, 3, None, 0, None) == _lib.OK
    # the getters read the object's own fields
    assert (lib.aeth_ldpc_n(p), lib.aeth_ldpc_k(p), lib.aeth_ldpc_rows(p), lib.aeth_ldpc_cols(p), lib.aeth_ldpc_z(p), lib.aeth_ldpc_edges(p),
            lib.aeth_ldpc_group(p)) == (30, 15, 3, 6, 5, 14, 51)


def test_dimensions_outside_the_definition(lib):
    both(lib, np.zeros((0, 4), np.int32), 4, _lib.E_ARG, "rows = 0")
    both(lib, np.zeros((257, 300), np.int32), 1, _lib.E_ARG, "rows = 257")
    both(lib, np.zeros((3, 3), np.int32), 4, _lib.E_ARG, "cols = 3", "rows = 3")
    both(lib, np.zeros((3, 2), np.int32), 4, _lib.E_ARG, "cols = 2", "rows = 3")
    both(lib, ldpc.staircase(3, 6, 5), 0, _lib.E_ARG, "z = 0")
    assert gen(lib, ldpc.staircase(256, 257, 1), 1)[0] == _lib.E_LEN                       # 256 rows are served: only the room is missing


@pytest.mark.parametrize("r,c,v", ((0, 0, -2), (2, 5, 5), (1, 3, 1 << 20), (2, 0, -(1 << 31))))
def test_an_entry_outside_the_block(lib, r, c, v):
    shift = ldpc.staircase(3, 6, 5)
    shift[r, c] = v
    both(lib, shift, 5, _lib.E_ARG, f"shift[{r}][{c}] = {v}", "-1 .. 4")


def test_a_row_without_a_block(lib):
    shift = ldpc.staircase(4, 8, 7)
    shift[2, :] = -1
    both(lib, shift, 7, _lib.E_ARG, "row 2 holds no block")


def test_a_singular_parity_part(lib):
    shift = ldpc.staircase(3, 6, 5)
    shift[2, 3:] = shift[1, 3:]
    both(lib, shift, 5, _lib.E_ARG, "parity part singular")


def table(rows, cols, per_row, extra=0):
    """staircase parity part plus information blocks: `per_row` blocks in every row, `extra` more in row 0"""
    shift = ldpc.staircase(rows, cols, 1, col_weight=0)
    for r in range(rows):
        have = int((shift[r] >= 0).sum())
        shift[r, :per_row - have + (extra if r == 0 else 0)] = 0
    return shift


def test_the_64_kib_state_boundary(lib):
    # z = 1: 2 N + E = 2 * 32000 + 1536 = 65536 is served, one block more is not
    at = table(256, 32000, 6)
    assert int((at >= 0).sum()) == 1536
    assert gen(lib, at, 1)[0] == _lib.E_LEN and "words" in lib.aeth_last_error().decode()
    over = table(256, 32000, 6, extra=1)
    both(lib, over, 1, _lib.E_UNSUPPORTED, "65537", "65536")
    # z = 256: 2 * 64 * 256 + 128 * 256 = 65536 / 129 blocks: 65792
    at = table(32, 64, 4)
    assert int((at >= 0).sum()) == 128
    code, tab = ldpc._code(at, 256)
    assert lib.aeth_ldpc_generator(C.byref(code), A, 0) == _lib.E_LEN
    both(lib, table(32, 64, 4, extra=1), 256, _lib.E_UNSUPPORTED, "65792", "65536")
    # N alone above the limit: refused before the table is read
    code = ldpc.Code(2, 1 << 20, 1 << 20, A.value)
    h = C.c_void_p(0x55)
    assert lib.aeth_ldpc_create(CTX, C.byref(code), C.byref(h)) == _lib.E_UNSUPPORTED and not h.value
    assert str(2 << 40).encode() in lib.aeth_last_error() and b"65536" in lib.aeth_last_error()


def test_lengths(lib):
    p = C.byref(fake())
    for nbits, ncoded in ((14, 30), (16, 30), (15, 29), (15, 60), (30, 30), (0, 30), (15, 0)):
        assert lib.aeth_ldpc_encode(p, A, nbits, B, ncoded) == _lib.E_LEN, (nbits, ncoded)
        msg = lib.aeth_last_error().decode()
        assert str(nbits) in msg or str(ncoded) in msg, msg
    for nsoft, flags, nbits in ((29, 0, 30), (31, 0, 30), (30, 0, 15), (30, 2, 30), (60, 2, 45), (60, 1, 59), (0, 0, 30), (30, 3, 0)):
        assert lib.aeth_ldpc_decode(p, A, nsoft, 5, flags, B, nbits, None) == _lib.E_LEN, (nsoft, flags, nbits)
        msg = lib.aeth_last_error().decode()
        assert str(nsoft) in msg or str(nbits) in msg, msg


def test_iterations_flags_alignment_and_overlap(lib):
    p = C.byref(fake())
    a = A.value
    assert lib.aeth_ldpc_decode(p, A, 30, 1001, 0, B, 30, None) == _lib.E_ARG and b"max_iter 1001" in lib.aeth_last_error()
    assert lib.aeth_ldpc_decode(p, A, 30, 1 << 31, 0, B, 30, None) == _lib.E_ARG
    for flags in (4, 8, 0x80000001):
        assert lib.aeth_ldpc_decode(p, A, 30, 5, flags, B, 30, None) == _lib.E_ARG
        assert f"0x{flags & ~3:x}".encode() in lib.aeth_last_error()
    assert lib.aeth_ldpc_decode(p, A, 30, 5, 0, B, 30, C.c_void_p(D.value + 2)) == _lib.E_ALIGN and b"4-byte" in lib.aeth_last_error()
    assert lib.aeth_ldpc_encode(p, A, 30, C.c_void_p(a + 29), 60) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_ldpc_encode(p, A, 30, C.c_void_p(a - 59), 60) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_ldpc_decode(p, A, 60, 5, 0, C.c_void_p(a + 59), 60, None) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_ldpc_decode(p, A, 60, 5, 2, C.c_void_p(a - 29), 30, None) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_ldpc_decode(p, A, 60, 5, 0, B, 60, C.c_void_p(a + 56)) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_ldpc_decode(p, A, 60, 5, 0, B, 60, C.c_void_p(B.value - 12)) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()


def test_ctypes_table_and_python_mirror():
    import aether_primitives_amd as ap
    for name in ("aeth_ldpc_generator", "aeth_ldpc_create", "aeth_ldpc_destroy", "aeth_ldpc_n", "aeth_ldpc_k", "aeth_ldpc_rows",
                 "aeth_ldpc_cols", "aeth_ldpc_z", "aeth_ldpc_edges", "aeth_ldpc_lds_bytes", "aeth_ldpc_group", "aeth_ldpc_encode",
                 "aeth_ldpc_decode"):
        assert name in _lib.PROTOTYPES and hasattr(_lib.load(), name), name
    for name in ("encode", "decode", "close", "n", "k", "rows", "cols", "z", "edges", "lds_bytes", "group"):
        assert hasattr(ap.Ldpc, name), name
    for name in ("ldpc", "Ldpc"):
        assert name in ap.__all__, name
    assert (ap.ldpc.EARLY, ap.ldpc.PAYLOAD, ap.ldpc.MAX_ITER, ap.ldpc.MAX_STATE) == (1, 2, 1000, 65536)
    shift = ap.ldpc.staircase(12, 24, 81)
    assert shift.shape == (12, 24) and shift.dtype == np.int32 and ((shift[:, :12] >= 0).sum(axis=0) == 3).all()
    assert (np.diag(shift[:, 12:]) == 0).all() and (np.diag(shift[:, 12:], -1) == 0).all() and int((shift[:, 12:] >= 0).sum()) == 23
    assert ap.ldpc.staircase(12, 24, 81).tobytes() == shift.tobytes() and ap.ldpc.staircase(12, 24, 81, seed=1).tobytes() != shift.tobytes()
