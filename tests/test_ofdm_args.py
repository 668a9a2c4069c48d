"""CPU: the aeth_ofdm_* entry points refuse every bad call with the status include/aether_hip.h names and a message that
names the offending value, before any device work (the pattern of tests/test_sync_args.py and tests/test_seq_args.py).

An object cannot be created without a device (create plans a transform and uploads its tables).  aeth_ofdm_create gets
the address of a zeroed block as its context and is refused before the context is looked at.  The other calls get an
object made by hand: struct aeth_ofdm starts with {ctx, n_fft, cp, n_bins, max_symbols, flags, fused} (csrc/aeth_fft_plan.h);
what lies behind stays null and is never reached, because every call here is refused first.  The read-outs, `span` and
`route` of a created object are exercised in tests/test_gpu_ofdm.py."""
import ctypes as C

import pytest

from aether_primitives_amd import _lib


class _Ofdm(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("n_fft", C.c_size_t), ("cp", C.c_size_t), ("n_bins", C.c_size_t), ("max_symbols", C.c_size_t),
                ("flags", C.c_int), ("fused", C.c_int), ("spare", C.c_char * 256)]


A = C.c_void_p(0x100000)             # 16-byte aligned "device" addresses, far apart, never dereferenced
B = C.c_void_p(0x40000000)
E = C.c_void_p(0x80000)
H = C.c_void_p(0x90000)
S = C.c_void_p(0xA0000)
N, G, K = 64, 16, 52
L = N + G


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def ctx():
    fake = (C.c_char * 4096)()
    return C.cast(fake, C.c_void_p), fake


@pytest.fixture()
def ofdm(ctx):
    o = _Ofdm(ctx=ctx[0], n_fft=N, cp=G, n_bins=K, max_symbols=0, flags=0, fused=1)
    return C.cast(C.pointer(o), C.c_void_p), o


def err(lib, rc, code, *words):
    assert rc == code, (rc, lib.aeth_last_error())
    msg = lib.aeth_last_error().decode()
    assert msg and all(str(w) in msg for w in words), msg


def create(lib, ctx, n_fft=N, cp=G, bins=tuple(range(1, K + 1)), n_bins=None, max_symbols=0, flags=0, out=True, null_bins=False):
    b = (C.c_uint32 * max(len(bins), 1))(*bins)
    h = C.c_void_p(0x5a5a)
    rc = lib.aeth_ofdm_create(ctx, n_fft, cp, None if null_bins else b, len(bins) if n_bins is None else n_bins, max_symbols, flags,
                              C.byref(h) if out else None)
    assert not out or not h.value                    # a refused create hands out no object
    return rc


def demod(lib, o, x=A, n_in=None, n_sym=3, eq=E, kind=0, out=B, n_out=None):
    n_in = (n_sym - 1) * L + N if n_in is None and n_sym else (0 if n_in is None else n_in)
    return lib.aeth_ofdm_demod(o, x, n_in, n_sym, eq, kind, 0.0, out, n_sym * K if n_out is None else n_out)


def mod(lib, o, car=A, n_car=None, n_sym=3, kind=0, out=B, n_out=None):
    return lib.aeth_ofdm_mod(o, car, n_sym * K if n_car is None else n_car, n_sym, kind, 0.0, out, n_sym * L if n_out is None else n_out)


def estimate(lib, o, y=A, x=B, n_sym=2, x_sym=1, nv=0.0, kind=0, h=H, eq=E, csi=S):
    return lib.aeth_ofdm_estimate(o, y, x, n_sym, x_sym, nv, kind, h, eq, csi)


def test_create_null_arguments(lib, ctx):
    err(lib, create(lib, None), _lib.E_ARG, "null")
    err(lib, create(lib, ctx[0], out=False), _lib.E_ARG, "null")
    err(lib, create(lib, ctx[0], null_bins=True), _lib.E_ARG, "bins")


def test_create_lengths(lib, ctx):
    for n in (0, 1):
        err(lib, create(lib, ctx[0], n_fft=n, cp=0, bins=(0,)), _lib.E_ARG, f"length {n}")
    # a length aeth_fft_create refuses: its status and its message
    err(lib, create(lib, ctx[0], n_fft=2 ** 24 + 1, cp=0, bins=(0,)), _lib.E_UNSUPPORTED, 2 ** 24 + 1)
    assert lib.aeth_fft_create(ctx[0], 2 ** 24 + 1, 1, C.byref(C.c_void_p())) == _lib.E_UNSUPPORTED
    err(lib, create(lib, ctx[0], cp=N + 1), _lib.E_ARG, f"prefix {N + 1}", N)
    err(lib, create(lib, ctx[0], bins=()), _lib.E_ARG, "0 carriers")
    err(lib, create(lib, ctx[0], bins=tuple(range(N)), n_bins=N + 1), _lib.E_ARG, f"{N + 1} carriers", f"{N} bins")
    err(lib, create(lib, ctx[0], flags=6), _lib.E_ARG, "flags", "0x6")


def test_create_carrier_list(lib, ctx):
    err(lib, create(lib, ctx[0], bins=(1, 2, N, 3)), _lib.E_ARG, "carrier 2", f"bin {N}")
    err(lib, create(lib, ctx[0], bins=(1, 2, 2 ** 32 - 1)), _lib.E_ARG, f"bin {2 ** 32 - 1}")
    err(lib, create(lib, ctx[0], bins=(5, 9, 7, 9)), _lib.E_ARG, "carrier 3", "bin 9", "carrier 1")


def test_null_handles(lib):
    err(lib, demod(lib, None), _lib.E_ARG, "null")
    err(lib, mod(lib, None), _lib.E_ARG, "null")
    err(lib, estimate(lib, None), _lib.E_ARG, "null")
    assert lib.aeth_ofdm_destroy(None) == _lib.OK
    assert lib.aeth_ofdm_len(None) == 0 and lib.aeth_ofdm_cp(None) == 0 and lib.aeth_ofdm_symbol(None) == 0
    assert lib.aeth_ofdm_carriers(None) == 0 and lib.aeth_ofdm_span(None, 3) == 0 and lib.aeth_ofdm_route(None) == b""


def test_read_outs_of_the_object(lib, ofdm):
    o = ofdm[0]
    assert (lib.aeth_ofdm_len(o), lib.aeth_ofdm_cp(o), lib.aeth_ofdm_symbol(o), lib.aeth_ofdm_carriers(o)) == (N, G, L, K)
    assert [lib.aeth_ofdm_span(o, s) for s in (0, 1, 2, 10)] == [0, N, L + N, 9 * L + N]


def test_null_pointers(lib, ofdm):
    o = ofdm[0]
    err(lib, demod(lib, o, x=None), _lib.E_ARG, "null")
    err(lib, demod(lib, o, out=None), _lib.E_ARG, "null")
    err(lib, mod(lib, o, car=None), _lib.E_ARG, "null")
    err(lib, mod(lib, o, out=None), _lib.E_ARG, "null")
    err(lib, estimate(lib, o, y=None), _lib.E_ARG, "null")
    err(lib, estimate(lib, o, x=None), _lib.E_ARG, "null")
    err(lib, estimate(lib, o, h=None, eq=None, csi=None), _lib.E_ARG, "outputs")


def test_lengths(lib, ofdm):
    o = ofdm[0]
    span = 2 * L + N
    err(lib, demod(lib, o, n_in=span - 1), _lib.E_LEN, span - 1, span)
    err(lib, demod(lib, o, n_out=3 * K + 1), _lib.E_LEN, 3 * K + 1, 3 * K)
    err(lib, demod(lib, o, n_out=3 * L), _lib.E_LEN, 3 * L)
    err(lib, mod(lib, o, n_car=3 * K - 1), _lib.E_LEN, 3 * K - 1, 3 * K)
    err(lib, mod(lib, o, n_out=3 * L - 1), _lib.E_LEN, 3 * L - 1, 3 * L)
    err(lib, mod(lib, o, n_out=2 * L + N), _lib.E_LEN, 2 * L + N)          # the span is what demod reads, not what mod writes
    assert demod(lib, o, n_in=span + 5, x=None) == _lib.E_ARG               # more input than the span is fine; the null is not


def test_empty_calls_succeed_without_pointers(lib, ofdm):
    o = ofdm[0]
    assert demod(lib, o, x=None, out=None, n_sym=0) == _lib.OK
    assert mod(lib, o, car=None, out=None, n_sym=0) == _lib.OK
    err(lib, demod(lib, o, n_sym=0, n_out=1), _lib.E_LEN, "1 output")
    err(lib, estimate(lib, o, n_sym=0, x_sym=0), _lib.E_LEN, "0 training")


def test_symbols_above_max_symbols(lib, ofdm):
    o, s = ofdm
    s.max_symbols = 2
    err(lib, demod(lib, o, n_sym=3), _lib.E_ARG, "3 symbols", "for 2")
    err(lib, mod(lib, o, n_sym=3), _lib.E_ARG, "3 symbols", "for 2")
    err(lib, estimate(lib, o, n_sym=3, x_sym=1), _lib.E_ARG, "3 symbols", "for 2")
    assert demod(lib, o, n_sym=2, x=None) == _lib.E_ARG and b"null" in lib.aeth_last_error()      # 2 passes the bound


def test_scale_and_equaliser_kinds(lib, ofdm):
    o = ofdm[0]
    for kind in (-1, 4):
        err(lib, demod(lib, o, kind=kind), _lib.E_ARG, kind)
        err(lib, mod(lib, o, kind=kind), _lib.E_ARG, kind)
    for kind in (-1, 3):
        err(lib, estimate(lib, o, kind=kind), _lib.E_ARG, f"kind {kind}")


def test_x_sym(lib, ofdm):
    o = ofdm[0]
    for x_sym in (0, 2, 4):
        err(lib, estimate(lib, o, n_sym=3, x_sym=x_sym), _lib.E_ARG, f"x_sym {x_sym}", "3")
    assert estimate(lib, o, n_sym=3, x_sym=3, y=None) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert estimate(lib, o, n_sym=3, x_sym=1, y=None) == _lib.E_ARG and b"null" in lib.aeth_last_error()


def test_alignment(lib, ofdm):
    o = ofdm[0]
    odd = lambda p, by=4: C.c_void_p(p.value + by)             # noqa: E731
    assert demod(lib, o, x=odd(A)) == _lib.E_ALIGN
    assert demod(lib, o, out=odd(B)) == _lib.E_ALIGN
    assert demod(lib, o, eq=odd(E)) == _lib.E_ALIGN
    assert mod(lib, o, car=odd(A)) == _lib.E_ALIGN
    assert mod(lib, o, out=odd(B)) == _lib.E_ALIGN
    for name in ("y", "x", "h", "eq"):
        assert estimate(lib, o, **{name: odd({"y": A, "x": B, "h": H, "eq": E}[name])}) == _lib.E_ALIGN, name
    assert estimate(lib, o, csi=odd(S, 2)) == _lib.E_ALIGN
    assert estimate(lib, o, csi=odd(S, 4), y=None) == _lib.E_ARG           # 4-byte alignment is enough for csi
    # only 8-byte alignment is asked of the samples: both parities pass and go on to the next check
    assert demod(lib, o, x=odd(A, 8), out=None) == _lib.E_ARG and b"null" in lib.aeth_last_error()


def test_in_place_is_refused(lib, ofdm):
    o = ofdm[0]
    span = 2 * L + N
    err(lib, demod(lib, o, out=A), _lib.E_ARG, "overlap")
    err(lib, demod(lib, o, out=C.c_void_p(A.value + 8 * (span - 1))), _lib.E_ARG, "overlap")
    err(lib, demod(lib, o, out=C.c_void_p(A.value - 8 * (3 * K - 1))), _lib.E_ARG, "overlap")
    err(lib, demod(lib, o, out=C.c_void_p(E.value + 8 * (K - 1))), _lib.E_ARG, "overlap")
    err(lib, mod(lib, o, out=A), _lib.E_ARG, "overlap")
    err(lib, mod(lib, o, out=C.c_void_p(A.value + 8 * (3 * K - 1))), _lib.E_ARG, "overlap")
    err(lib, estimate(lib, o, h=A), _lib.E_ARG, "overlap")
    err(lib, estimate(lib, o, csi=C.c_void_p(B.value + 8 * K - 4)), _lib.E_ARG, "overlap")
    err(lib, estimate(lib, o, h=H, eq=C.c_void_p(H.value + 8 * (K - 1))), _lib.E_ARG, "overlap")
