"""CPU: the aeth_seq_* entry points validate their arguments before any device work, as the other entry points do
(tests/test_corr_args.py): every bad call returns its AETH_E_* code with a message and touches nothing.

A sequence object cannot be created without a device (create uploads its jump table).  aeth_seq_create receives the
address of a zeroed block as its context (validation only asks whether the pointer is null, and every call here is
refused before the device is looked at).  The device calls receive a hand-made object: struct aeth_seq starts with
{ctx, nregs, order[4], mask[4]} (csrc/aeth_sequence.hip); the pointers behind stay null and are never reached, because
each call is refused first (a call that passed validation would go on to the device and is not made here)."""
import ctypes as C

import pytest

from aether_primitives_amd import _lib
from aether_primitives_amd.sequence import _SeqReg


class _Seq(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("nregs", C.c_size_t), ("order", C.c_size_t * 4), ("mask", C.c_uint64 * 4),
                ("pw", C.c_void_p), ("tab_dev", C.c_void_p), ("spare", C.c_char * 64)]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def fake_ctx():
    block = (C.c_char * 4096)()
    return C.cast(block, C.c_void_p), block


def fake_seq(ctx):
    """what aeth_seq_create would have built for the LTE Gold pair, minus its tables"""
    s = _Seq(ctx=ctx, nregs=2)
    s.order[0], s.order[1] = 31, 31
    s.mask[0] = (1 << (64 - 28)) | (1 << (64 - 31))
    s.mask[1] = sum(1 << (64 - d) for d in (28, 29, 30, 31))
    return C.cast(C.pointer(s), C.c_void_p), s


def reg(*delays):
    d = (C.c_uint32 * max(len(delays), 1))(*delays)
    return _SeqReg(C.cast(d, C.POINTER(C.c_uint32)), len(delays)), d


def regs(*sets):
    built = [reg(*s) for s in sets]
    return (_SeqReg * max(len(built), 1))(*[b[0] for b in built]), built


def _err(lib, rc, code, *words):
    assert rc == code, (rc, lib.aeth_last_error())
    msg = lib.aeth_last_error().decode()
    assert msg and all(w in msg for w in words), msg


INIT = (C.c_uint64 * 4)(1, 2, 3, 4)
A = C.c_void_p(0x100000)             # never dereferenced: 16-byte aligned "device" addresses, 1 MiB apart
B = C.c_void_p(0x200000)
N = 5000
BIG = 2 ** 64 - 1
Z = _lib.Cf32(1.0, 1.0)
O = _lib.Cf32(-1.0, -1.0)


def test_create_arguments(lib, fake_ctx):
    ctx, _ = fake_ctx
    out = C.c_void_p(0x55)
    good, k0 = regs((28, 31), (28, 29, 30, 31))
    _err(lib, lib.aeth_seq_create(None, good, 2, C.byref(out)), _lib.E_ARG, "ctx", "null")
    assert not out.value                                              # cleared, as aeth_fir_create does
    _err(lib, lib.aeth_seq_create(ctx, good, 2, None), _lib.E_ARG, "null")
    _err(lib, lib.aeth_seq_create(ctx, None, 2, C.byref(out)), _lib.E_ARG, "regs", "null")
    _err(lib, lib.aeth_seq_create(ctx, good, 0, C.byref(out)), _lib.E_ARG, "0 registers", "1 .. 4")
    five, k1 = regs((1,), (2,), (3,), (4,), (5,))
    _err(lib, lib.aeth_seq_create(ctx, five, 5, C.byref(out)), _lib.E_ARG, "5 registers", "1 .. 4")
    null_delays = (_SeqReg * 1)(_SeqReg(None, 2))
    _err(lib, lib.aeth_seq_create(ctx, null_delays, 1, C.byref(out)), _lib.E_ARG, "register 0", "null")
    none, k2 = regs((28, 31), ())
    _err(lib, lib.aeth_seq_create(ctx, none, 2, C.byref(out)), _lib.E_ARG, "register 1", "0 delays", "1 .. 64")
    many, k3 = regs(tuple(range(1, 65)) + (1,))
    _err(lib, lib.aeth_seq_create(ctx, many, 1, C.byref(out)), _lib.E_ARG, "65 delays", "1 .. 64")
    zero, k4 = regs((3, 0))
    _err(lib, lib.aeth_seq_create(ctx, zero, 1, C.byref(out)), _lib.E_ARG, "delay 0", "1 .. 64")
    high, k5 = regs((3, 5), (7, 65))
    _err(lib, lib.aeth_seq_create(ctx, high, 2, C.byref(out)), _lib.E_ARG, "register 1", "delay 65", "1 .. 64")
    twice, k6 = regs((3, 5, 9, 5))
    _err(lib, lib.aeth_seq_create(ctx, twice, 1, C.byref(out)), _lib.E_ARG, "delay 5", "repeated")
    assert not out.value
    assert lib.aeth_seq_destroy(None) == _lib.OK
    assert lib.aeth_seq_nregs(None) == 0 and lib.aeth_seq_order(None, 0) == 0


def test_accessors_read_the_object(lib, fake_ctx):
    seq, keep = fake_seq(fake_ctx[0])
    assert lib.aeth_seq_nregs(seq) == 2 and lib.aeth_seq_order(seq, 0) == 31 and lib.aeth_seq_order(seq, 1) == 31
    assert lib.aeth_seq_order(seq, 2) == 0
    c = lib.aeth_seq_chunk(seq)
    assert c >= 4096 and c % 4096 == 0 and c == lib.aeth_seq_chunk(None)


def test_window_arguments(lib):
    w = C.c_uint64(0x5a)
    r, k = reg(6, 7)
    _err(lib, lib.aeth_seq_window(None, 1, 0, C.byref(w)), _lib.E_ARG, "null")
    _err(lib, lib.aeth_seq_window(C.byref(r), 1, 0, None), _lib.E_ARG, "null")
    for bad, words in (((), ("0 delays",)), ((0,), ("delay 0",)), ((65, 2), ("delay 65",)), ((2, 2), ("repeated",))):
        r, k = reg(*bad)
        _err(lib, lib.aeth_seq_window(C.byref(r), 1, 0, C.byref(w)), _lib.E_ARG, *words)
    assert w.value == 0x5a


def test_bits_and_host_bits_arguments(lib, fake_ctx):
    seq, keep = fake_seq(fake_ctx[0])
    for f in (lib.aeth_seq_bits, lib.aeth_host_seq_bits):
        _err(lib, f(None, INIT, 0, A, N), _lib.E_ARG, "seq", "null")
        _err(lib, f(seq, None, 0, A, N), _lib.E_ARG, "init", "null")
        _err(lib, f(seq, INIT, 0, None, N), _lib.E_ARG, "null")
        _err(lib, f(seq, INIT, BIG, A, 1), _lib.E_ARG, "overflows")
        _err(lib, f(seq, INIT, BIG - N + 1, A, N), _lib.E_ARG, "overflows")
        _err(lib, f(seq, INIT, 2 ** 63, A, 2 ** 63), _lib.E_ARG, "overflows")
        assert f(seq, INIT, BIG, None, 0) == _lib.OK                  # nothing to generate: no error and no launch


def test_scramble_arguments(lib, fake_ctx):
    seq, keep = fake_seq(fake_ctx[0])
    f = lib.aeth_seq_scramble
    _err(lib, f(None, INIT, 0, A, B, N), _lib.E_ARG, "seq", "null")
    _err(lib, f(seq, None, 0, A, B, N), _lib.E_ARG, "init", "null")
    _err(lib, f(seq, INIT, 0, None, B, N), _lib.E_ARG, "null")
    _err(lib, f(seq, INIT, 0, A, None, N), _lib.E_ARG, "null")
    _err(lib, f(seq, INIT, BIG, A, B, 1), _lib.E_ARG, "overflows")
    for out in (A.value + 1, A.value - 1, A.value + N - 1, A.value - N + 1, A.value + 16):
        _err(lib, f(seq, INIT, 0, A, C.c_void_p(out), N), _lib.E_ARG, "overlaps", "in place")
    assert f(seq, INIT, 0, None, None, 0) == _lib.OK


def test_chips_arguments(lib, fake_ctx):
    seq, keep = fake_seq(fake_ctx[0])
    f = lib.aeth_seq_chips
    _err(lib, f(None, INIT, 0, Z, O, A, N), _lib.E_ARG, "seq", "null")
    _err(lib, f(seq, None, 0, Z, O, A, N), _lib.E_ARG, "init", "null")
    _err(lib, f(seq, INIT, 0, Z, O, None, N), _lib.E_ARG, "null")
    _err(lib, f(seq, INIT, BIG - 1, Z, O, A, 2), _lib.E_ARG, "overflows")
    for off in (1, 2, 4, 7, 12):
        _err(lib, f(seq, INIT, 0, Z, O, C.c_void_p(A.value + off), N), _lib.E_ALIGN, "8-byte aligned")
    assert f(seq, INIT, 0, Z, O, None, 0) == _lib.OK


def test_spread_arguments(lib, fake_ctx):
    seq, keep = fake_seq(fake_ctx[0])
    f = lib.aeth_seq_spread
    _err(lib, f(None, INIT, 0, A, 40, 125, B, N), _lib.E_ARG, "seq", "null")
    _err(lib, f(seq, None, 0, A, 40, 125, B, N), _lib.E_ARG, "init", "null")
    _err(lib, f(seq, INIT, 0, None, 40, 125, B, N), _lib.E_ARG, "null")
    _err(lib, f(seq, INIT, 0, A, 40, 125, None, N), _lib.E_ARG, "null")
    _err(lib, f(seq, INIT, 0, A, 40, 0, B, 0), _lib.E_ARG, "spreading factor")
    _err(lib, f(seq, INIT, 0, A, 40, 125, B, N - 1), _lib.E_LEN, "4999 chips", "40 symbols")
    _err(lib, f(seq, INIT, 0, A, 41, 125, B, N), _lib.E_LEN, "5000 chips")
    _err(lib, f(seq, INIT, 0, A, 2 ** 40, 2 ** 40, B, 0), _lib.E_LEN, "chips")       # nsym * sf overflows
    _err(lib, f(seq, INIT, BIG, A, 40, 125, B, N), _lib.E_ARG, "overflows")
    _err(lib, f(seq, INIT, 0, C.c_void_p(A.value + 4), 40, 125, B, N), _lib.E_ALIGN, "8-byte aligned")
    _err(lib, f(seq, INIT, 0, A, 40, 125, C.c_void_p(B.value + 4), N), _lib.E_ALIGN, "8-byte aligned")
    # in place only for sf == 1 with out == sym
    _err(lib, f(seq, INIT, 0, A, 40, 125, A, N), _lib.E_ARG, "overlaps", "in place")
    _err(lib, f(seq, INIT, 0, A, N, 1, C.c_void_p(A.value + 8), N), _lib.E_ARG, "overlaps", "in place")
    _err(lib, f(seq, INIT, 0, A, 40, 125, C.c_void_p(A.value + 39 * 8), N), _lib.E_ARG, "overlaps")
    _err(lib, f(seq, INIT, 0, A, 40, 125, C.c_void_p(A.value - N * 8 + 8), N), _lib.E_ARG, "overlaps")
    assert f(seq, INIT, 0, None, 0, 7, None, 0) == _lib.OK


def test_python_mirror_has_the_new_surface():
    import aether_primitives_amd as ap
    for name in ("bits", "scramble", "chips", "spread", "window", "chunk", "order", "nregs"):
        assert hasattr(ap.Sequence, name), name
    assert callable(ap.lte_gold) and callable(ap.sequence.expand) and callable(ap.sequence.generate)
