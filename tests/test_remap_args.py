"""CPU: every refusal of aeth_remap_create and of the table builders with its code and the value it names, before any
device work (the context handle below is never followed), the null handles, and the ctypes table."""
import ctypes as C

import numpy as np
import pytest

from aether_primitives_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


FAKE = (C.c_char * 4096)()
CTX = C.cast(FAKE, C.c_void_p)           # never dereferenced: every call below returns before any device work
A = C.c_void_p(0x100000)
B = C.c_void_p(0x200000)
MAXP = 1 << 20


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def create(lib, m, r_in, r_out=None, ctx=CTX):
    m = np.ascontiguousarray(m, np.int32)
    h = C.c_void_p(0x55)
    rc = lib.aeth_remap_create(ctx, ptr(m), m.size if r_out is None else r_out, r_in, C.byref(h))
    return rc, h, lib.aeth_last_error().decode()


def test_null_handles(lib):
    m = np.zeros(4, np.int32)
    assert lib.aeth_remap_create(CTX, ptr(m), 4, 4, None) == _lib.E_ARG and b"out" in lib.aeth_last_error()
    rc, h, msg = create(lib, m, 4, ctx=None)
    assert rc == _lib.E_ARG and "ctx" in msg and not h.value
    h = C.c_void_p(0x55)
    assert lib.aeth_remap_create(CTX, None, 4, 4, C.byref(h)) == _lib.E_ARG and b"map is null" in lib.aeth_last_error() and not h.value
    assert lib.aeth_remap_destroy(None) == _lib.OK
    for f in (lib.aeth_remap_in_period, lib.aeth_remap_out_period, lib.aeth_remap_route, lib.aeth_remap_tile):
        assert f(None) == 0
    assert lib.aeth_remap_in_count(None, 100) == 0
    assert lib.aeth_remap_exec(None, A, 8, B, 8, 0) == _lib.E_ARG and b"rm is null" in lib.aeth_last_error()


@pytest.mark.parametrize("r_in,r_out,named", ((0, 4, "input period 0"), (MAXP + 1, 4, f"input period {MAXP + 1}"),
                                              (4, 0, "output period 0"), (4, MAXP + 1, f"output period {MAXP + 1}")))
def test_periods_outside_1_to_2_to_the_20(lib, r_in, r_out, named):
    rc, h, msg = create(lib, np.zeros(4, np.int32), r_in, r_out)
    assert rc == _lib.E_ARG and named in msg and not h.value, msg


@pytest.mark.parametrize("pos,bad,r_in", ((0, -2, 4), (3, 4, 4), (2, 5, 4), (1, MAXP, MAXP), (191, -7, 288)))
def test_a_table_entry_outside_minus_one_to_r_in(lib, pos, bad, r_in):
    m = np.zeros(max(pos + 1, 4), np.int32)
    m[pos] = bad
    rc, h, msg = create(lib, m, r_in)
    assert rc == _lib.E_ARG and f"map[{pos}] = {bad}" in msg and not h.value, msg


def test_puncture_refusals(lib):
    keep, m, n = np.array([1, 1, 0, 1], np.uint8), np.zeros(8, np.int32), C.c_size_t(77)
    assert lib.aeth_remap_puncture(ptr(keep), 4, ptr(m), 2, C.byref(n)) == _lib.E_LEN
    msg = lib.aeth_last_error().decode()
    assert "holds 2" in msg and "keeps 3" in msg, msg
    assert lib.aeth_remap_puncture(ptr(keep), 4, ptr(m), 3, C.byref(n)) == _lib.OK and n.value == 3 and m[:3].tolist() == [0, 1, 3]
    zero = np.array([0, 2, 4, 0, 0], np.uint8)                         # only bit 0 counts
    assert lib.aeth_remap_puncture(ptr(zero), 5, ptr(m), 8, C.byref(n)) == _lib.E_ARG and b"none of its 5" in lib.aeth_last_error()
    assert lib.aeth_remap_puncture(ptr(keep), 0, ptr(m), 8, C.byref(n)) == _lib.E_ARG and b"period 0" in lib.aeth_last_error()
    assert lib.aeth_remap_puncture(None, 4, ptr(m), 8, C.byref(n)) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_remap_puncture(ptr(keep), 4, None, 8, C.byref(n)) == _lib.E_ARG
    assert lib.aeth_remap_puncture(ptr(keep), 4, ptr(m), 8, None) == _lib.E_ARG


def test_invert_refusals(lib):
    m, inv = np.array([0, 1, 9, 2], np.int32), np.zeros(8, np.int32)
    assert lib.aeth_remap_invert(ptr(m), 4, 4, ptr(inv)) == _lib.E_ARG and b"map[2] = 9" in lib.aeth_last_error()
    assert lib.aeth_remap_invert(ptr(m), 4, 0, ptr(inv)) == _lib.E_ARG and b"input period 0" in lib.aeth_last_error()
    assert lib.aeth_remap_invert(ptr(m), 0, 4, ptr(inv)) == _lib.E_ARG and b"output period 0" in lib.aeth_last_error()
    assert lib.aeth_remap_invert(None, 4, 4, ptr(inv)) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_remap_invert(ptr(m), 4, 10, None) == _lib.E_ARG and b"inv is null" in lib.aeth_last_error()


def test_compose_refusals(lib):
    a, b, out = np.array([0, 1, 2, 5], np.int32), np.arange(192, dtype=np.int32), np.zeros(192, np.int32)
    ro, ri = C.c_size_t(0), C.c_size_t(0)
    call = lambda a_, ao, ai, b_, bo, bi, cap: lib.aeth_remap_compose(ptr(a_), ao, ai, ptr(b_), bo, bi, ptr(out), cap, C.byref(ro), C.byref(ri))
    assert call(a, 4, 6, b, 192, 192, 191) == _lib.E_LEN
    msg = lib.aeth_last_error().decode()
    assert "holds 191" in msg and "192" in msg, msg
    assert call(a, 4, 6, b, 192, 192, 192) == _lib.OK and (ro.value, ri.value) == (192, 288)
    assert call(a, 4, 5, b, 192, 192, 192) == _lib.E_ARG and b"a[3] = 5" in lib.aeth_last_error()
    assert call(a, 4, 6, b, 192, 191, 192) == _lib.E_ARG and b"b[191] = 191" in lib.aeth_last_error()
    assert call(a, 0, 6, b, 192, 192, 192) == _lib.E_ARG and b"a: output period 0" in lib.aeth_last_error()
    assert call(a, 4, 6, b, 192, MAXP + 1, 192) == _lib.E_ARG and f"b: input period {MAXP + 1}".encode() in lib.aeth_last_error()
    # lcm(1021, 1031) = 1052651 periods of the intermediate stream: above 2^20 on both sides
    p, q = np.zeros(1021, np.int32), np.zeros(1031, np.int32)
    big = np.zeros(MAXP, np.int32)
    assert lib.aeth_remap_compose(ptr(p), 1021, 1021, ptr(q), 1031, 1031, ptr(big), MAXP, C.byref(ro), C.byref(ri)) == _lib.E_UNSUPPORTED
    assert b"1052651" in lib.aeth_last_error()
    assert lib.aeth_remap_compose(ptr(a), 4, 6, ptr(b), 192, 192, None, 192, C.byref(ro), C.byref(ri)) == _lib.E_ARG


def test_rows_cols_and_bicm16_refusals(lib):
    out = np.zeros(4096, np.int32)
    assert lib.aeth_remap_rows_cols(0, 5, ptr(out)) == _lib.E_ARG and b"rows 0" in lib.aeth_last_error()
    assert lib.aeth_remap_rows_cols(5, 0, ptr(out)) == _lib.E_ARG and b"cols 0" in lib.aeth_last_error()
    assert lib.aeth_remap_rows_cols(1024, 1025, ptr(out)) == _lib.E_ARG and b"1049600" in lib.aeth_last_error()
    assert lib.aeth_remap_rows_cols(3, 5, None) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_remap_bicm16(190, 4, ptr(out)) == _lib.E_ARG and b"n_cbps 190" in lib.aeth_last_error()
    assert lib.aeth_remap_bicm16(64, 6, ptr(out)) == _lib.E_ARG and b"n_cbps 64" in lib.aeth_last_error()      # 16 s = 48
    assert lib.aeth_remap_bicm16(96, 5, ptr(out)) == _lib.E_ARG and b"n_bpsc 5" in lib.aeth_last_error()       # 16 s = 32 divides, 5 does not
    assert lib.aeth_remap_bicm16(0, 1, ptr(out)) == _lib.E_ARG and b"n_cbps 0" in lib.aeth_last_error()
    assert lib.aeth_remap_bicm16(48, 0, ptr(out)) == _lib.E_ARG and b"n_bpsc 0" in lib.aeth_last_error()
    assert lib.aeth_remap_bicm16(48, 1, None) == _lib.E_ARG and b"null" in lib.aeth_last_error()


def test_ctypes_table_and_python_mirror():
    import aether_primitives_amd as ap
    for name in ("aeth_remap_create", "aeth_remap_destroy", "aeth_remap_in_period", "aeth_remap_out_period", "aeth_remap_in_count",
                 "aeth_remap_route", "aeth_remap_tile", "aeth_remap_exec", "aeth_remap_puncture", "aeth_remap_invert",
                 "aeth_remap_compose", "aeth_remap_rows_cols", "aeth_remap_bicm16"):
        assert name in _lib.PROTOTYPES and hasattr(_lib.load(), name), name
    for name in ("exec", "in_count", "puncture", "rows_cols", "bicm16", "inverse", "then", "route", "tile"):
        assert hasattr(ap.Remap, name), name
    assert "remap" in ap.__all__ and "Remap" in ap.__all__
    assert (ap.remap.ROUTE_TILE, ap.remap.ROUTE_GATHER) == (1, 2)
