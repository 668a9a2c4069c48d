"""CPU: every refusal of aeth_rs_* with its code and the value it names, before any device work (the context and object
handles below are never followed past their own fields), the null behaviours and the catalogue's unknown name."""
import ctypes as C

import numpy as np
import pytest

from aether_primitives_amd import _lib, rs

FAKE = (C.c_char * 4096)()
CTX = C.cast(FAKE, C.c_void_p)           # never dereferenced: every call below returns before any device work
A = C.c_void_p(0x100000)
B = C.c_void_p(0x900000000)
D = C.c_void_p(0x1200000000)
E = C.c_void_p(0x1800000000)
GOOD = (4, 0x13, 1, 1, 4, 15)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


class FakeRs(C.Structure):
    """what a call reads of an object before it refuses: the context pointer, the code and the group's size"""
    _fields_ = [("ctx", C.c_void_p), ("code", rs.Code), ("lg", C.c_uint32), ("tab", C.c_void_p), ("rest", C.c_uint64 * 8)]


def fake():
    return FakeRs(CTX.value, rs.Code(*GOOD), 2, None)


def refused(lib, code, status, *words):
    """create, generator, host_encode and host_decode refuse a code alike"""
    c = rs.Code(*code)
    h = C.c_void_p(0x55)
    buf = np.zeros(1 << 16, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    calls = (lambda: lib.aeth_rs_create(CTX, C.byref(c), C.byref(h)),
             lambda: lib.aeth_rs_generator(C.byref(c), p, 65),
             lambda: lib.aeth_rs_host_encode(C.byref(c), p, 0, 1, p, 0),
             lambda: lib.aeth_rs_host_decode(C.byref(c), p, 0, None, 1, 0, p, 0, None, None))
    for call in calls:
        assert call() == status
        msg = lib.aeth_last_error().decode()
        assert all(w in msg for w in words), msg
    assert not h.value


def test_null_handles_and_pointers(lib):
    c = rs.Code(*GOOD)
    h = C.c_void_p(0x55)
    assert lib.aeth_rs_create(CTX, C.byref(c), None) == _lib.E_ARG and b"out is null" in lib.aeth_last_error()
    assert lib.aeth_rs_create(None, C.byref(c), C.byref(h)) == _lib.E_ARG and b"ctx is null" in lib.aeth_last_error() and not h.value
    h = C.c_void_p(0x55)
    assert lib.aeth_rs_create(CTX, None, C.byref(h)) == _lib.E_ARG and b"code is null" in lib.aeth_last_error() and not h.value
    assert lib.aeth_rs_generator(None, A, 100) == _lib.E_ARG and b"code is null" in lib.aeth_last_error()
    assert lib.aeth_rs_generator(C.byref(c), None, 100) == _lib.E_ARG and b"g_out is null" in lib.aeth_last_error()
    assert lib.aeth_rs_generator(C.byref(c), A, 4) == _lib.E_LEN and b"5 coefficients" in lib.aeth_last_error()
    assert lib.aeth_rs_named(None, C.byref(c)) == _lib.E_ARG and lib.aeth_rs_named(b"rs-15-11", None) == _lib.E_ARG
    assert lib.aeth_rs_destroy(None) == _lib.OK
    for f in (lib.aeth_rs_n, lib.aeth_rs_k, lib.aeth_rs_nroots, lib.aeth_rs_m, lib.aeth_rs_group):
        assert f(None) == 0
    assert lib.aeth_rs_lds_bytes(None, 1) == 0
    assert lib.aeth_rs_encode(None, A, 11, 1, B, 15) == _lib.E_ARG and b"rs is null" in lib.aeth_last_error()
    assert lib.aeth_rs_decode(None, A, 15, None, 1, 0, B, 15, None, None) == _lib.E_ARG and b"rs is null" in lib.aeth_last_error()
    f = fake()
    assert lib.aeth_rs_encode(C.byref(f), None, 11, 1, B, 15) == _lib.E_ARG and b"null pointer" in lib.aeth_last_error()
    assert lib.aeth_rs_encode(C.byref(f), A, 11, 1, None, 15) == _lib.E_ARG and b"null pointer" in lib.aeth_last_error()
    assert lib.aeth_rs_decode(C.byref(f), None, 15, None, 1, 0, B, 15, None, None) == _lib.E_ARG and b"null pointer" in lib.aeth_last_error()
    assert lib.aeth_rs_decode(C.byref(f), A, 15, None, 1, 0, None, 15, None, None) == _lib.E_ARG and b"null pointer" in lib.aeth_last_error()
    buf = np.zeros(64, np.uint8).ctypes.data_as(C.c_void_p)
    assert lib.aeth_rs_host_encode(C.byref(c), None, 11, 1, buf, 15) == _lib.E_ARG
    assert lib.aeth_rs_host_decode(C.byref(c), buf, 15, None, 1, 0, None, 15, None, None) == _lib.E_ARG


def test_the_fake_object_answers_its_getters(lib):
    f = fake()
    p = C.byref(f)
    assert (lib.aeth_rs_n(p), lib.aeth_rs_k(p), lib.aeth_rs_nroots(p), lib.aeth_rs_m(p), lib.aeth_rs_group(p)) == (15, 11, 4, 4, 64)
    assert lib.aeth_rs_lds_bytes(p, 1) == lib.aeth_rs_lds_bytes(p, 64) == 64 * 8 * 5 + 64 * 12
    assert lib.aeth_rs_lds_bytes(p, 0) == 0 and lib.aeth_rs_lds_bytes(p, 65) == 0


def test_unknown_name_lists_the_known_ones(lib):
    c = rs.Code()
    assert lib.aeth_rs_named(b"rs-255-251", C.byref(c)) == _lib.E_ARG
    msg = lib.aeth_last_error().decode()
    assert "rs-255-251" in msg
    for name in ("ccsds-255-223", "ccsds-255-239", "dvb-204-188", "rs-15-11"):
        assert name in msg
        assert rs.named(name).n in (255, 204, 15)
    with pytest.raises(_lib.AetherError):
        rs.named("nothing")


def test_every_rule_of_the_code(lib):
    m, poly, fcr, prim, r, n = GOOD
    refused(lib, (2, 0x7, 0, 1, 1, 3), _lib.E_ARG, "m = 2")
    refused(lib, (9, 0x211, 0, 1, 4, 15), _lib.E_ARG, "m = 9")
    refused(lib, (4, 0x3, 1, 1, 4, 15), _lib.E_ARG, "poly 0x3", "degree")                  # the x^m term is missing
    refused(lib, (4, 0x33, 1, 1, 4, 15), _lib.E_ARG, "poly 0x33", "degree")
    refused(lib, (4, 0x1f, 1, 1, 4, 15), _lib.E_ARG, "polynomial not primitive", "0x1f")    # irreducible, x of order 5
    refused(lib, (4, 0x15, 1, 1, 4, 15), _lib.E_ARG, "polynomial not primitive", "0x15")    # reducible
    refused(lib, (4, 0x12, 1, 1, 4, 15), _lib.E_ARG, "polynomial not primitive", "0x12")    # no constant term
    refused(lib, (8, 0x11b, 0, 1, 16, 255), _lib.E_ARG, "polynomial not primitive", "0x11b")   # the AES polynomial: irreducible, not primitive
    refused(lib, (4, 0x13, 1, 3, 4, 15), _lib.E_ARG, "prim 3")
    refused(lib, (4, 0x13, 1, 0, 4, 15), _lib.E_ARG, "prim 0")
    refused(lib, (4, 0x13, 1, 15, 4, 15), _lib.E_ARG, "prim 15")
    refused(lib, (4, 0x13, 15, 1, 4, 15), _lib.E_ARG, "fcr 15")
    refused(lib, (4, 0x13, 1, 1, 0, 15), _lib.E_ARG, "nroots 0")
    refused(lib, (8, 0x11d, 0, 1, 65, 255), _lib.E_UNSUPPORTED, "nroots 65")
    refused(lib, (4, 0x13, 1, 1, 4, 4), _lib.E_ARG, "n = 4")
    refused(lib, (4, 0x13, 1, 1, 4, 16), _lib.E_ARG, "n = 16")
    refused(lib, (4, 0x13, 1, 1, 15, 15), _lib.E_ARG, "n = 15")
    # the boundaries on the inside are accepted by the host calls
    for code in ((4, 0x13, 14, 14, 14, 15), (3, 0xb, 0, 1, 1, 2), (8, 0x11d, 254, 254, 64, 65), (4, 0x13, 1, 16, 4, 15)):
        assert rs.generator(code).size == code[4] + 1


def test_depth_flags_lengths(lib):
    f = fake()
    p = C.byref(f)
    for depth in (0, 65, 1 << 31):
        assert lib.aeth_rs_encode(p, A, 11, depth, B, 15) == _lib.E_ARG and f"depth {depth}".encode() in lib.aeth_last_error()
        assert lib.aeth_rs_decode(p, A, 15, None, depth, 0, B, 15, None, None) == _lib.E_ARG and f"depth {depth}".encode() in lib.aeth_last_error()
    assert lib.aeth_rs_decode(p, A, 15, None, 1, 2, B, 15, None, None) == _lib.E_ARG and b"0x2" in lib.aeth_last_error()
    assert lib.aeth_rs_decode(p, A, 15, None, 1, 0x81, B, 11, None, None) == _lib.E_ARG and b"0x80" in lib.aeth_last_error()
    # whole frames on both sides
    assert lib.aeth_rs_encode(p, A, 12, 1, B, 15) == _lib.E_LEN and b"12" in lib.aeth_last_error()
    assert lib.aeth_rs_encode(p, A, 22, 4, B, 30) == _lib.E_LEN and b"44 bytes" in lib.aeth_last_error()      # depth 4: a frame is 44 bytes
    assert lib.aeth_rs_encode(p, A, 44, 4, B, 59) == _lib.E_LEN and b"59" in lib.aeth_last_error()
    assert lib.aeth_rs_encode(p, A, 44, 4, B, 120) == _lib.E_LEN
    assert lib.aeth_rs_decode(p, A, 16, None, 1, 0, B, 16, None, None) == _lib.E_LEN and b"16" in lib.aeth_last_error()
    assert lib.aeth_rs_decode(p, A, 30, None, 1, 0, B, 22, None, None) == _lib.E_LEN and b"22" in lib.aeth_last_error()    # 22 is the payload size
    assert lib.aeth_rs_decode(p, A, 30, None, 1, 1, B, 30, None, None) == _lib.E_LEN
    assert lib.aeth_rs_decode(p, A, 60, None, 4, 0, B, 59, None, None) == _lib.E_LEN
    assert lib.aeth_rs_decode(p, A, 30, None, 2, 0, B, 0, None, None) == _lib.E_LEN


def test_alignment_and_overlap(lib):
    f = fake()
    p = C.byref(f)
    rec, summ = C.c_void_p(D.value + 4), C.c_void_p(E.value + 8)
    for off in (1, 2, 3):
        assert lib.aeth_rs_decode(p, A, 15, None, 1, 0, B, 15, C.c_void_p(D.value + off), None) == _lib.E_ALIGN and b"rec_dev" in lib.aeth_last_error()
    for off in (1, 2, 4, 7):
        assert lib.aeth_rs_decode(p, A, 15, None, 1, 0, B, 15, None, C.c_void_p(E.value + off)) == _lib.E_ALIGN and b"summary_dev" in lib.aeth_last_error()
    assert lib.aeth_rs_encode(p, A, 11, 1, C.c_void_p(A.value + 10), 15) == _lib.E_ARG and b"overlaps" in lib.aeth_last_error()
    assert lib.aeth_rs_encode(p, A, 11, 1, C.c_void_p(A.value - 14), 15) == _lib.E_ARG
    n = 150                                                               # ten codewords: records of 80 bytes
    for bad in ((A, None, C.c_void_p(A.value + n - 1), rec, summ),         # output on the input's last byte
                (A, B, C.c_void_p(B.value + n - 1), rec, summ),            # output on the erasure flags
                (A, None, B, C.c_void_p(A.value + 148), summ),             # records on the input
                (A, B, D, C.c_void_p(B.value - 76), summ),                 # records on the erasure flags
                (A, None, B, rec, C.c_void_p(A.value + 144)),              # summary on the input
                (A, B, D, None, C.c_void_p(B.value + 8)),                  # summary on the erasure flags
                (A, None, B, C.c_void_p(B.value + 148), summ),             # records on the output
                (A, None, B, rec, C.c_void_p(B.value - 8)),                # summary on the output
                (A, None, B, rec, C.c_void_p(rec.value + 76))):            # summary on the records
        i, e, o, r, s = bad
        assert lib.aeth_rs_decode(p, i, n, e, 1, 0, o, n, r, s) == _lib.E_ARG and b"overlap" in lib.aeth_last_error(), bad


def test_python_wrappers_refuse_alike():
    with pytest.raises(_lib.AetherError):
        rs.generator((4, 0x1f, 1, 1, 4, 15))
    with pytest.raises(_lib.AetherError):
        rs.host_encode(GOOD, np.zeros(12, np.uint8))
    with pytest.raises(_lib.AetherError):
        rs.host_decode(GOOD, np.zeros(15, np.uint8), depth=65)
    out, rec, summ = rs.host_decode("rs-15-11", np.zeros(0, np.uint8))
    assert out.size == 0 and rec.size == 0 and int(summ["n_failed"]) == 0
