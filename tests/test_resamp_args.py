"""CPU: aeth_resamp_prototype against its formula in numpy f64, and the aeth_resamp_* entry points refusing null handles
and null contexts before any device work (tests/test_chan_args.py does the same for the analysis bank)."""
import ctypes as C

import numpy as np
import pytest

from aether_primitives_amd import _lib
from aether_primitives_amd import resamp

CASES = ((1, 1, 1), (1, 1, 16), (2, 1, 8), (1, 4, 16), (3, 2, 8), (2, 3, 3), (147, 160, 16), (160, 147, 16), (7, 5, 64),
         (1, 64, 2), (5, 1, 1))                                     # (U, Q, P)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def formula(U, Q, P):
    L, c = U * P, max(U, Q)
    if L == 1:
        return np.ones(1)
    n = np.arange(L, dtype=np.float64)
    h = np.sinc((n - (L - 1) / 2) / c) * (0.54 - 0.46 * np.cos(2 * np.pi * n / (L - 1)))      # np.sinc(x) = sin(pi x) / (pi x)
    return h * U / h.sum()


def ulps_apart(a, b):
    """distance of two float32 arrays in units in the last place (both finite, same sign or zero)"""
    ia, ib = (v.view(np.int32).astype(np.int64) for v in (a, b))
    ia, ib = (np.where(i < 0, -(i & 0x7fffffff), i) for i in (ia, ib))
    return np.abs(ia - ib)


@pytest.mark.parametrize("U,Q,P", CASES)
def test_prototype_is_the_formula_rounded_once(U, Q, P):
    got = resamp.prototype(U, Q, P)
    assert got.dtype == np.float32 and got.size == U * P
    want = formula(U, Q, P).astype(np.float32)
    # the two f64 evaluations differ by far less than an f32 ulp: only a rounding tie can move a tap, by one ulp
    assert ulps_apart(got, want).max() <= 1, (U, Q, P, int(ulps_apart(got, want).max()))
    # every tap is rounded by at most half an ulp of a value no larger than the largest tap
    assert abs(got.astype(np.float64).sum() - U) <= U * P * 2.0 ** -24 * max(1.0, float(np.abs(got).max()))
    assert (got.view(np.uint32) == got[::-1].view(np.uint32)).all()               # symmetric


def test_prototype_refusals(lib):
    assert resamp.prototype(1, 7, 1).tolist() == [1.0]
    out = (C.c_float * 8)(*([7.0] * 8))

    def err(rc, *words):
        msg = lib.aeth_last_error().decode()
        assert rc == _lib.E_ARG, (rc, msg)
        assert all(w in msg for w in words), msg

    err(lib.aeth_resamp_prototype(0, 1, 2, out), "up 0")
    err(lib.aeth_resamp_prototype(2, 0, 2, out), "down 0")
    err(lib.aeth_resamp_prototype(2, 1, 0, out), "0 taps per phase")
    err(lib.aeth_resamp_prototype(2 ** 40, 1, 2 ** 40, out), "overflow")
    err(lib.aeth_resamp_prototype(4, 1, 2, None), "null")
    assert list(out) == [7.0] * 8                                   # nothing was written
    assert lib.aeth_resamp_prototype(4, 1, 2, out) == _lib.OK and list(out) != [7.0] * 8


A = C.c_void_p(0x100000)             # never dereferenced: 16-byte aligned "device" addresses, 1 MiB apart
B = C.c_void_p(0x200000)


def test_null_handles_and_null_contexts_are_refused_without_a_device(lib):
    w = (C.c_float * 16)(*([1.0] * 16))
    h = C.c_void_p(0x55)
    assert lib.aeth_resamp_create(None, w, 16, 4, 3, C.byref(h)) == _lib.E_ARG and not h.value       # cleared, as aeth_chan_create does
    assert b"ctx" in lib.aeth_last_error() and b"null" in lib.aeth_last_error()
    assert lib.aeth_resamp_create(None, w, 16, 4, 3, None) == _lib.E_ARG
    assert lib.aeth_resamp_exec(None, None, A, 16, B, 16) == _lib.E_ARG
    assert b"resamp" in lib.aeth_last_error() and b"null" in lib.aeth_last_error()
    assert lib.aeth_resamp_destroy(None) == _lib.OK
    assert lib.aeth_resamp_up(None) == 0 and lib.aeth_resamp_down(None) == 0 and lib.aeth_resamp_ntaps(None) == 0
    assert lib.aeth_resamp_history(None) == 0 and lib.aeth_resamp_tile(None) == 0 and lib.aeth_resamp_route(None) == b""
    assert lib.aeth_resamp_out_count(None, 16) == 0


def test_python_mirror_has_the_new_surface():
    import aether_primitives_amd as ap
    for name in ("exec", "out_count", "history", "route", "tile", "up", "down", "ntaps"):
        assert hasattr(ap.Resampler, name), name
    assert callable(ap.resamp.prototype) and ap.resamp.Resampler is ap.Resampler
    assert "resamp" in ap.__all__ and "Resampler" in ap.__all__
