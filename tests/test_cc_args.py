"""CPU: every refusal of the convolutional-code entry points with its code and the value it names, before any device
work (the context handle below is never followed), and the ctypes table."""
import ctypes as C

import pytest

from aether_primitives_amd import _lib
from aether_primitives_amd.cc import _Code


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


FAKE = (C.c_char * 4096)()
CTX = C.cast(FAKE, C.c_void_p)           # never dereferenced: every call below returns before any device work
A = C.c_void_p(0x100000)                 # "device" addresses, 1 MiB apart
B = C.c_void_p(0x200000)
H = C.c_void_p(0x300000)


def code(k=7, polys=(0o171, 0o133)):
    return _Code(k, len(polys), (C.c_uint32 * 4)(*(list(polys) + [0] * 4)[:4]))


def create(lib, c, D=512, Aw=64, T=64, ctx=CTX):
    h = C.c_void_p(0x55)
    rc = lib.aeth_cc_create(ctx, C.byref(c) if c is not None else None, D, Aw, T, C.byref(h))
    return rc, h, lib.aeth_last_error().decode()


def test_null_handles(lib):
    c = code()
    assert lib.aeth_cc_create(CTX, C.byref(c), 512, 64, 64, None) == _lib.E_ARG and b"out" in lib.aeth_last_error()
    rc, h, msg = create(lib, c, ctx=None)
    assert rc == _lib.E_ARG and "ctx" in msg and not h.value
    rc, h, msg = create(lib, None)
    assert rc == _lib.E_ARG and "code" in msg and not h.value
    assert lib.aeth_cc_destroy(None) == _lib.OK
    for f in (lib.aeth_cc_k, lib.aeth_cc_n, lib.aeth_cc_block, lib.aeth_cc_warmup, lib.aeth_cc_traceback, lib.aeth_cc_history):
        assert f(None) == 0
    assert lib.aeth_cc_encode(None, None, A, 8, B, 16) == _lib.E_ARG and b"cc is null" in lib.aeth_last_error()
    assert lib.aeth_cc_decode(None, None, A, 16, B, 8) == _lib.E_ARG and b"cc is null" in lib.aeth_last_error()
    assert lib.aeth_demod_soft(None, A, 8, 2, None, 1.0, B, 16) == _lib.E_ARG and b"ctx" in lib.aeth_last_error()


@pytest.mark.parametrize("k,rc_want", ((2, _lib.E_ARG), (8, _lib.E_UNSUPPORTED), (9, _lib.E_UNSUPPORTED), (10, _lib.E_ARG)))
def test_k_outside_the_built_range(lib, k, rc_want):
    rc, h, msg = create(lib, code(k, (1, 3)))
    assert rc == rc_want and f"k {k}" in msg and not h.value, msg


@pytest.mark.parametrize("polys", ((0o171,), (1, 2, 3, 4, 5)))
def test_n_outside_2_to_4(lib, polys):
    c = code(7, polys[:4])
    c.n = len(polys)
    rc, h, msg = create(lib, c)
    assert rc == _lib.E_ARG and f"n {len(polys)}" in msg and not h.value, msg


@pytest.mark.parametrize("k", (3, 7))
@pytest.mark.parametrize("which", (0, 1))
def test_polynomial_of_zero_or_two_to_the_k(lib, k, which):
    for bad in (0, 1 << k):
        polys = [(1 << k) - 1, (1 << k) - 1]
        polys[which] = bad
        rc, h, msg = create(lib, code(k, polys))
        assert rc == _lib.E_ARG and f"poly[{which}] {bad}" in msg and not h.value, msg


def test_block_warmup_and_traceback_limits(lib):
    rc, h, msg = create(lib, code(), D=0)
    assert rc == _lib.E_ARG and "block 0" in msg and not h.value, msg
    rc, h, msg = create(lib, code(), D=4000, T=97)
    assert rc == _lib.E_ARG and "4097" in msg and not h.value, msg
    rc, h, msg = create(lib, code(), D=4097, T=0)
    assert rc == _lib.E_ARG and "4097" in msg and not h.value, msg
    rc, h, msg = create(lib, code(), Aw=4097)
    assert rc == _lib.E_ARG and "warmup 4097" in msg and not h.value, msg


def test_an_object_needs_no_device_and_refuses_bad_calls(lib):
    rc, h, msg = create(lib, code(4, (0o15, 0o17, 0o13)), D=4000, Aw=4096, T=96)       # every limit is served
    assert rc == _lib.OK and h.value, msg
    try:
        assert (lib.aeth_cc_k(h), lib.aeth_cc_n(h), lib.aeth_cc_block(h), lib.aeth_cc_warmup(h), lib.aeth_cc_traceback(h)) == (4, 3, 4000, 4096, 96)
        assert lib.aeth_cc_history(h) == 4096 + 96
        assert lib.aeth_cc_encode(h, None, A, 8, B, 25) == _lib.E_LEN and b"25" in lib.aeth_last_error()
        assert lib.aeth_cc_decode(h, None, A, 25, B, 8) == _lib.E_LEN and b"25" in lib.aeth_last_error()
        assert lib.aeth_cc_encode(h, None, None, 0, None, 0) == _lib.OK                 # nothing to do
        assert lib.aeth_cc_decode(h, None, None, 0, None, 0) == _lib.OK
        assert lib.aeth_cc_encode(h, None, None, 8, B, 24) == _lib.E_ARG and b"null" in lib.aeth_last_error()
        assert lib.aeth_cc_decode(h, None, A, 24, None, 8) == _lib.E_ARG and b"null" in lib.aeth_last_error()
        # an output that shares a byte with an input or with the history
        assert lib.aeth_cc_encode(h, None, A, 8, C.c_void_p(A.value + 7), 24) == _lib.E_ARG and b"overlaps" in lib.aeth_last_error()
        assert lib.aeth_cc_encode(h, H, A, 8, C.c_void_p(H.value + 2), 24) == _lib.E_ARG and b"overlaps" in lib.aeth_last_error()
        assert lib.aeth_cc_decode(h, None, A, 24, C.c_void_p(A.value + 23), 8) == _lib.E_ARG and b"overlaps" in lib.aeth_last_error()
        assert lib.aeth_cc_decode(h, H, A, 24, C.c_void_p(H.value + 3 * (4096 + 96) - 1), 8) == _lib.E_ARG and b"overlaps" in lib.aeth_last_error()
    finally:
        assert lib.aeth_cc_destroy(h) == _lib.OK


def test_soft_demodulator_refusals(lib):
    assert lib.aeth_demod_soft(CTX, A, 8, 0, None, 1.0, B, 0) == _lib.E_UNSUPPORTED and b"bits_per_symbol 0" in lib.aeth_last_error()
    assert lib.aeth_demod_soft(CTX, A, 8, 9, None, 1.0, B, 72) == _lib.E_UNSUPPORTED and b"bits_per_symbol 9" in lib.aeth_last_error()
    assert lib.aeth_demod_soft(CTX, A, 8, 4, None, 1.0, B, 32) == _lib.E_ARG and b"table" in lib.aeth_last_error()
    assert lib.aeth_demod_soft(CTX, A, 8, 2, None, 1.0, B, 15) == _lib.E_LEN and b"15" in lib.aeth_last_error()
    assert lib.aeth_demod_soft(CTX, A, 0, 2, None, 1.0, None, 0) == _lib.OK
    assert lib.aeth_demod_soft(CTX, None, 8, 2, None, 1.0, B, 16) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_demod_soft(CTX, C.c_void_p(A.value + 4), 8, 2, None, 1.0, B, 16) == _lib.E_ALIGN
    assert lib.aeth_demod_soft(CTX, A, 8, 2, None, 1.0, C.c_void_p(A.value + 63), 16) == _lib.E_ARG and b"overlaps" in lib.aeth_last_error()


def test_ctypes_table_and_python_mirror():
    import aether_primitives_amd as ap
    for name in ("aeth_cc_create", "aeth_cc_destroy", "aeth_cc_k", "aeth_cc_n", "aeth_cc_block", "aeth_cc_warmup", "aeth_cc_traceback",
                 "aeth_cc_history", "aeth_cc_encode", "aeth_cc_decode", "aeth_demod_soft"):
        assert name in _lib.PROTOTYPES and hasattr(_lib.load(), name), name
    for name in ("encode", "decode", "decode_stream", "block", "warmup", "traceback", "history"):
        assert hasattr(ap.ConvCode, name), name
    assert hasattr(ap.modulation._Modulation, "demod_soft") and ap.DeviceSoft is ap.modulation.DeviceSoft
    assert "cc" in ap.__all__ and "ConvCode" in ap.__all__ and "DeviceSoft" in ap.__all__
