"""CPU: every refusal of aeth_crc_* and aeth_bits_* with its code and the value it names, before any device work (the
context and object handles below are never followed past their own fields), the null behaviours, and the ctypes table."""
import ctypes as C

import numpy as np
import pytest

from aether_primitives_amd import _lib

FAKE = (C.c_char * 4096)()
CTX = C.cast(FAKE, C.c_void_p)           # never dereferenced: every call below returns before any device work
A = C.c_void_p(0x100000)
B = C.c_void_p(0x900000000)
D = C.c_void_p(0x1200000000)
S = C.c_void_p(0x1b00000000)
G32 = 1 << 32


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def create(lib, r, poly, init=0, xorout=0, ctx=CTX):
    h = C.c_void_p(0x55)
    rc = lib.aeth_crc_create(ctx, r, poly, init, xorout, C.byref(h))
    return rc, h, lib.aeth_last_error().decode()


class FakeCrc(C.Structure):
    """what a call reads of an object before it refuses: the context pointer and the parameters"""
    _fields_ = [("ctx", C.c_void_p), ("r", C.c_uint32), ("poly", C.c_uint64), ("init", C.c_uint64), ("xorout", C.c_uint64),
                ("rest", C.c_uint64 * 8)]


def fake_crc(r=16, poly=0x1021):
    return FakeCrc(CTX.value, r, poly, 0, 0)


def test_null_handles_and_pointers(lib):
    assert lib.aeth_crc_create(CTX, 16, 0x1021, 0, 0, None) == _lib.E_ARG and b"out is null" in lib.aeth_last_error()
    rc, h, msg = create(lib, 16, 0x1021, ctx=None)
    assert rc == _lib.E_ARG and "ctx" in msg and not h.value
    assert lib.aeth_crc_destroy(None) == _lib.OK
    for f in (lib.aeth_crc_width, lib.aeth_crc_poly, lib.aeth_crc_init, lib.aeth_crc_xorout, lib.aeth_crc_residue,
              lib.aeth_crc_route_frame_bits):
        assert f(None) == 0
    assert lib.aeth_crc_route(None, 100, 1) == 0 and lib.aeth_crc_frames_per_workgroup(None, 100) == 0
    assert lib.aeth_crc_exec(None, A, 8, 1, None, B) == _lib.E_ARG and b"crc is null" in lib.aeth_last_error()
    assert lib.aeth_crc_attach(None, A, 8, 1, B) == _lib.E_ARG and b"crc is null" in lib.aeth_last_error()
    assert lib.aeth_crc_check(None, A, 8, 1, 0, B, None, None) == _lib.E_ARG and b"crc is null" in lib.aeth_last_error()
    c = fake_crc()
    p = C.byref(c)
    assert lib.aeth_crc_exec(p, A, 8, 1, None, None) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_crc_exec(p, None, 8, 1, None, B) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_crc_attach(p, A, 8, 1, None) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_crc_attach(p, None, 8, 1, B) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_crc_check(p, None, 8, 1, 0, B, None, None) == _lib.E_ARG and b"in_dev is null" in lib.aeth_last_error()
    assert lib.aeth_crc_check(p, A, 8, 1, 0, None, None, None) == _lib.E_ARG and b"all null" in lib.aeth_last_error()
    assert lib.aeth_bits_pack(None, A, 8, 0, B, 1) == _lib.E_ARG and b"ctx is null" in lib.aeth_last_error()
    assert lib.aeth_bits_unpack(None, A, 1, 0, B, 8) == _lib.E_ARG and b"ctx is null" in lib.aeth_last_error()
    assert lib.aeth_bits_pack(CTX, None, 8, 0, B, 1) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_bits_pack(CTX, A, 8, 0, None, 1) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_bits_unpack(CTX, None, 1, 0, B, 8) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_bits_unpack(CTX, A, 1, 0, None, 8) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    # nothing to do is no refusal, and needs no pointers
    assert lib.aeth_crc_exec(p, None, 8, 0, None, None) == _lib.OK
    assert lib.aeth_crc_attach(p, None, 8, 0, None) == _lib.OK
    assert lib.aeth_crc_check(p, None, 8, 0, 0, B, None, None) == _lib.OK
    assert lib.aeth_bits_pack(CTX, None, 0, 0, None, 0) == _lib.OK and lib.aeth_bits_unpack(CTX, None, 0, 0, None, 0) == _lib.OK


@pytest.mark.parametrize("r,poly,init,xorout,named", (
    (0, 1, 0, 0, "r = 0"), (65, 1, 0, 0, "r = 65"), (16, 0x1020, 0, 0, "poly 0x1020 is even"), (16, 0x11021, 0, 0, "poly 0x11021"),
    (16, 0x1021, 0x10000, 0, "init 0x10000"), (16, 0x1021, 0, 0x10000, "xorout 0x10000"), (1, 3, 0, 0, "poly 0x3"),
    (63, (1 << 63) | 1, 0, 0, "poly 0x8000000000000001"), (8, 0x07, 0x100, 0, "init 0x100")))
def test_parameters_outside_the_definition(lib, r, poly, init, xorout, named):
    rc, h, msg = create(lib, r, poly, init, xorout)
    assert rc == _lib.E_ARG and named in msg and not h.value, msg
    reg = C.c_uint64()
    bits = np.zeros(4, np.uint8)
    assert lib.aeth_crc_host(r, poly, init, xorout, bits.ctypes.data_as(C.c_void_p), 4, C.byref(reg)) == _lib.E_ARG
    assert named in lib.aeth_last_error().decode()


def test_host_and_named_refusals(lib):
    reg = C.c_uint64()
    assert lib.aeth_crc_host(16, 0x1021, 0, 0, None, 4, C.byref(reg)) == _lib.E_ARG and b"bits_host is null" in lib.aeth_last_error()
    assert lib.aeth_crc_host(16, 0x1021, 0, 0, None, 4, None) == _lib.E_ARG and b"reg is null" in lib.aeth_last_error()
    assert lib.aeth_crc_host(16, 0x1021, 0x1234, 0, None, 0, C.byref(reg)) == _lib.OK and reg.value == 0x1234      # L = 0: the start state
    r, p, i, x = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    assert lib.aeth_crc_named(b"crc-99", C.byref(r), C.byref(p), C.byref(i), C.byref(x)) == _lib.E_ARG
    msg = lib.aeth_last_error().decode()
    assert "crc-99" in msg and "crc-24/lte-a" in msg and "crc-64/ecma-182" in msg, msg
    assert lib.aeth_crc_named(None, C.byref(r), C.byref(p), C.byref(i), C.byref(x)) == _lib.E_ARG
    assert lib.aeth_crc_named(b"crc-8", None, C.byref(p), C.byref(i), C.byref(x)) == _lib.E_ARG
    assert lib.aeth_crc_named(b"crc-24/lte-b", C.byref(r), C.byref(p), C.byref(i), C.byref(x)) == _lib.OK
    assert (r.value, p.value, i.value, x.value) == (24, 0x800063, 0, 0)


def test_mask_at_or_above_two_to_the_r(lib):
    p = C.byref(fake_crc())
    assert lib.aeth_crc_check(p, A, 8, 1, 0x10000, B, None, None) == _lib.E_ARG and b"mask 0x10000" in lib.aeth_last_error()
    assert lib.aeth_crc_check(C.byref(fake_crc(64, 0x1B)), A, 8, 0, (1 << 64) - 1, B, None, None) == _lib.OK


def test_calls_that_reach_two_to_the_32_bytes(lib):
    p = C.byref(fake_crc())
    assert lib.aeth_crc_exec(p, A, G32, 1, None, B) == _lib.E_UNSUPPORTED and str(G32).encode() in lib.aeth_last_error()
    assert lib.aeth_crc_exec(p, A, 1 << 16, 1 << 16, None, B) == _lib.E_UNSUPPORTED and b"65536" in lib.aeth_last_error()
    assert lib.aeth_crc_exec(p, A, 0, 1 << 29, None, B) == _lib.E_UNSUPPORTED and b"states" in lib.aeth_last_error()
    assert lib.aeth_crc_exec(p, A, 1 << 63, 4, None, B) == _lib.E_UNSUPPORTED
    assert lib.aeth_crc_attach(p, A, G32 - 16, 1, B) == _lib.E_UNSUPPORTED and str(G32 - 16).encode() in lib.aeth_last_error()
    assert lib.aeth_crc_attach(p, A, (1 << 64) - 8, 1, B) == _lib.E_UNSUPPORTED
    assert lib.aeth_crc_check(p, A, G32 - 16, 1, 0, B, None, None) == _lib.E_UNSUPPORTED and str(G32 - 16).encode() in lib.aeth_last_error()
    assert lib.aeth_crc_check(p, A, 0, 1 << 29, 0, B, None, None) == _lib.E_UNSUPPORTED
    assert lib.aeth_bits_pack(CTX, A, G32, 0, B, G32 // 8) == _lib.E_UNSUPPORTED and str(G32).encode() in lib.aeth_last_error()
    assert lib.aeth_bits_unpack(CTX, A, G32 // 8, 0, B, G32) == _lib.E_UNSUPPORTED and str(G32).encode() in lib.aeth_last_error()


def test_an_output_that_shares_a_byte_with_an_input(lib):
    p = C.byref(fake_crc())
    a = A.value
    assert lib.aeth_crc_exec(p, A, 64, 2, None, C.c_void_p(a + 120)) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_crc_exec(p, A, 64, 2, B, C.c_void_p(B.value + 8)) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_crc_attach(p, A, 64, 2, C.c_void_p(a + 127)) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_crc_attach(p, A, 64, 2, C.c_void_p(a - 159)) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    for outs in ((C.c_void_p(a + 152), None, None), (None, C.c_void_p(a - 127), None), (None, None, C.c_void_p(a - 8))):
        assert lib.aeth_crc_check(p, A, 64, 2, 0, *outs) == _lib.E_ARG and b"overlap" in lib.aeth_last_error(), outs
    assert lib.aeth_crc_check(p, A, 64, 2, 0, B, C.c_void_p(B.value + 15), None) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_bits_pack(CTX, A, 64, 0, C.c_void_p(a + 63), 8) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()
    assert lib.aeth_bits_unpack(CTX, A, 8, 0, C.c_void_p(a - 63), 64) == _lib.E_ARG and b"overlap" in lib.aeth_last_error()


def test_bit_order_and_lengths(lib):
    for order in (-1, 2, 7):
        assert lib.aeth_bits_pack(CTX, A, 64, order, B, 8) == _lib.E_ARG and f"order {order}".encode() in lib.aeth_last_error()
        assert lib.aeth_bits_unpack(CTX, A, 8, order, B, 64) == _lib.E_ARG and f"order {order}".encode() in lib.aeth_last_error()
    for nbits, nbytes in ((64, 7), (64, 9), (65, 8), (1, 0), (0, 1)):
        assert lib.aeth_bits_pack(CTX, A, nbits, 0, B, nbytes) == _lib.E_LEN, (nbits, nbytes)
        msg = lib.aeth_last_error().decode()
        assert str(nbits) in msg and str(nbytes) in msg, msg
    for nbytes, nbits in ((8, 65), (0, 1), (3, 32)):
        assert lib.aeth_bits_unpack(CTX, A, nbytes, 1, B, nbits) == _lib.E_LEN, (nbytes, nbits)
        msg = lib.aeth_last_error().decode()
        assert str(nbits) in msg and str(nbytes) in msg, msg


def test_ctypes_table_and_python_mirror():
    import aether_primitives_amd as ap
    for name in ("aeth_crc_create", "aeth_crc_destroy", "aeth_crc_width", "aeth_crc_poly", "aeth_crc_init", "aeth_crc_xorout",
                 "aeth_crc_residue", "aeth_crc_route", "aeth_crc_route_frame_bits", "aeth_crc_frames_per_workgroup", "aeth_crc_named",
                 "aeth_crc_host", "aeth_crc_exec", "aeth_crc_attach", "aeth_crc_check", "aeth_bits_pack", "aeth_bits_unpack"):
        assert name in _lib.PROTOTYPES and hasattr(_lib.load(), name), name
    for name in ("named", "registers", "attach", "check", "residue", "route", "route_frame_bits", "frames_per_workgroup"):
        assert hasattr(ap.Crc, name), name
    for name in ("crc", "Crc", "DeviceU64", "pack_bits", "unpack_bits"):
        assert name in ap.__all__, name
    assert hasattr(ap.DeviceBits, "pack_bits") and hasattr(ap.DeviceBits, "unpack_bits")
    assert (ap.crc.ROUTE_FRAMES, ap.crc.ROUTE_LONG, ap.crc.LSB_FIRST, ap.crc.MSB_FIRST) == (1, 2, 0, 1)


def test_words_are_eight_byte_aligned(lib):
    p = C.byref(fake_crc())
    odd = C.c_void_p(B.value + 4)
    assert lib.aeth_crc_exec(p, A, 8, 1, None, odd) == _lib.E_ALIGN and b"8-byte" in lib.aeth_last_error()
    assert lib.aeth_crc_exec(p, A, 8, 1, odd, D) == _lib.E_ALIGN
    assert lib.aeth_crc_check(p, A, 8, 1, 0, odd, None, None) == _lib.E_ALIGN and b"8-byte" in lib.aeth_last_error()
    assert lib.aeth_crc_check(p, A, 8, 1, 0, None, None, odd) == _lib.E_ALIGN
