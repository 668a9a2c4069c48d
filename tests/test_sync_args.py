"""CPU: aeth_sync_line and aeth_sync_lag refuse every bad call with the status include/aether_hip.h names, before any
device work: the context handle below is never followed and the "device" addresses are never dereferenced."""
import ctypes as C

import pytest

from aether_primitives_amd import _lib
from aether_primitives_amd.nco import _Words

A = C.c_void_p(0x100000)             # 16-byte aligned "device" addresses, far apart
H = C.c_void_p(0x80000)
R = C.c_void_p(0x40000000)
N = 4096


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def ctx():
    fake = (C.c_char * 4096)()
    return C.cast(fake, C.c_void_p), fake


def line(lib, ctx, kind=0, w=None, n0=0, x=A, n=N, block=0, rec=R, total=None):
    return lib.aeth_sync_line(ctx, kind, w, n0, x, n, block, rec, total)


def lag(lib, ctx, power=4, lag_=1, hist=H, x=A, n=N, block=0, rec=R, total=None):
    return lib.aeth_sync_lag(ctx, power, lag_, hist, x, n, block, rec, total)


def test_null_arguments(lib, ctx):
    ctx = ctx[0]
    tot = _lib.SyncRecord()
    assert line(lib, None) == _lib.E_ARG and b"ctx" in lib.aeth_last_error()
    assert lag(lib, None) == _lib.E_ARG and b"ctx" in lib.aeth_last_error()
    assert line(lib, ctx, x=None) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lag(lib, ctx, x=None) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert line(lib, ctx, rec=None, total=None) == _lib.E_ARG and b"outputs" in lib.aeth_last_error()
    assert lag(lib, ctx, rec=None, total=None) == _lib.E_ARG and b"outputs" in lib.aeth_last_error()
    assert line(lib, ctx, x=None, rec=None, total=C.byref(tot)) == _lib.E_ARG


def test_empty_input_is_a_length_error(lib, ctx):
    ctx = ctx[0]
    assert line(lib, ctx, n=0) == _lib.E_LEN and b"empty" in lib.aeth_last_error()
    assert lag(lib, ctx, n=0) == _lib.E_LEN and b"empty" in lib.aeth_last_error()


def test_unknown_kind_and_power(lib, ctx):
    ctx = ctx[0]
    for kind in (-1, 3, 5, 6, 7, 9, 16):
        assert line(lib, ctx, kind=kind) == _lib.E_ARG and str(kind).encode() in lib.aeth_last_error()
    for power in (-1, 0, 3, 5, 16):
        assert lag(lib, ctx, power=power) == _lib.E_ARG and str(power).encode() in lib.aeth_last_error()


def test_lag_range(lib, ctx):
    ctx = ctx[0]
    assert lag(lib, ctx, lag_=0) == _lib.E_ARG and b"lag 0" in lib.aeth_last_error()
    assert lag(lib, ctx, lag_=2 ** 20 + 1, hist=None) == _lib.E_ARG and str(2 ** 20 + 1).encode() in lib.aeth_last_error()


def test_alignment(lib, ctx):
    ctx = ctx[0]
    odd = lambda p: C.c_void_p(p.value + 4)             # noqa: E731
    assert line(lib, ctx, x=odd(A)) == _lib.E_ALIGN
    assert line(lib, ctx, rec=odd(R)) == _lib.E_ALIGN
    assert lag(lib, ctx, x=odd(A)) == _lib.E_ALIGN
    assert lag(lib, ctx, hist=odd(H)) == _lib.E_ALIGN
    assert lag(lib, ctx, rec=odd(R)) == _lib.E_ALIGN


def test_position_past_the_end_of_the_counter(lib, ctx):
    ctx = ctx[0]
    w = _Words(1, 2, 3)
    assert line(lib, ctx, w=C.byref(w), n0=2 ** 64 - N + 1) == _lib.E_UNSUPPORTED
    msg = lib.aeth_last_error().decode()
    assert str(2 ** 64 - N + 1) in msg and f"{N} samples" in msg, msg
    assert line(lib, ctx, w=None, n0=2 ** 64 - N + 1) == _lib.E_UNSUPPORTED      # the position is checked with or without words


def test_too_many_workgroups(lib, ctx):
    ctx = ctx[0]
    big = C.c_void_p(1 << 44)
    assert line(lib, ctx, n=2 ** 31, block=1, rec=big) == _lib.E_UNSUPPORTED and b"2^31" in lib.aeth_last_error()
    assert lag(lib, ctx, n=2 ** 31, block=1, rec=big) == _lib.E_UNSUPPORTED and b"2^31" in lib.aeth_last_error()
    chunk = lib.aeth_sync_chunk()
    assert line(lib, ctx, n=2 ** 31 * chunk, block=0, rec=big) == _lib.E_UNSUPPORTED


def test_records_overlapping_the_input(lib, ctx):
    ctx = ctx[0]
    inside = C.c_void_p(A.value + 8 * (N - 1))
    assert line(lib, ctx, rec=inside) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lag(lib, ctx, rec=inside) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lag(lib, ctx, lag_=16, rec=C.c_void_p(H.value + 8 * 15)) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    # room for 64 records in front of x; blocks of 63 samples make 66
    before = C.c_void_p(A.value - 48 * 64)
    assert line(lib, ctx, block=N // 64 - 1, rec=before) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
