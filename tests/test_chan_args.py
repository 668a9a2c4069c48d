"""CPU: aeth_chan_prototype against its four formulas in numpy f64, and the aeth_chan_* entry points refusing null handles
and null contexts before any device work (tests/test_seq_args.py does the same for the sequences)."""
import ctypes as C

import numpy as np
import pytest

from aether_primitives_amd import _lib
from aether_primitives_amd import chan

CASES = ((1, 1), (4, 1), (5, 2), (16, 8), (1024, 16))            # (M, P)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def formula(kind, M, P):
    L = M * P
    n = np.arange(L, dtype=np.float64)
    if kind == chan.RECT:
        return np.ones(L)
    if kind == chan.HANN:
        return 0.5 - 0.5 * np.cos(2 * np.pi * n / L)
    if kind == chan.HAMMING:
        return 0.54 - 0.46 * np.cos(2 * np.pi * n / L)
    if L == 1:
        return np.ones(1)
    h = np.sinc((n - (L - 1) / 2) / M) * (0.54 - 0.46 * np.cos(2 * np.pi * n / (L - 1)))      # np.sinc(x) = sin(pi x) / (pi x)
    return h / h.sum()


def ulps_apart(a, b):
    """distance of two float32 arrays in units in the last place (both finite, same sign or zero)"""
    ia, ib = (v.view(np.int32).astype(np.int64) for v in (a, b))
    ia, ib = (np.where(i < 0, -(i & 0x7fffffff), i) for i in (ia, ib))
    return np.abs(ia - ib)


@pytest.mark.parametrize("M,P", CASES)
@pytest.mark.parametrize("kind", (chan.RECT, chan.HANN, chan.HAMMING, chan.SINC_HAMMING))
def test_prototype_is_the_formula_rounded_once(kind, M, P):
    got = chan.prototype(kind, M, P)
    assert got.dtype == np.float32 and got.size == M * P
    want = formula(kind, M, P).astype(np.float32)
    if kind == chan.RECT:
        assert (got.view(np.uint32) == want.view(np.uint32)).all()
    # the two f64 evaluations differ by far less than an f32 ulp: only a rounding tie can move a tap, by one ulp
    assert ulps_apart(got, want).max() <= 1, (kind, M, P, int(ulps_apart(got, want).max()))
    if kind == chan.SINC_HAMMING:
        assert abs(got.astype(np.float64).sum() - 1.0) <= M * P * 2.0 ** -24


def test_prototype_by_name_and_refusals(lib):
    assert (chan.prototype("hann", 8, 2) == chan.prototype(chan.HANN, 8, 2)).all()
    assert chan.prototype("sinc_hamming", 1, 1).tolist() == [1.0]
    out = (C.c_float * 8)(*([7.0] * 8))

    def err(rc, *words):
        msg = lib.aeth_last_error().decode()
        assert rc == _lib.E_ARG, (rc, msg)
        assert all(w in msg for w in words), msg

    err(lib.aeth_chan_prototype(4, 4, 2, out), "kind 4")
    err(lib.aeth_chan_prototype(-1, 4, 2, out), "kind -1")
    err(lib.aeth_chan_prototype(chan.HANN, 0, 2, out), "0 channels")
    err(lib.aeth_chan_prototype(chan.HANN, 4, 0, out), "0 taps per channel")
    err(lib.aeth_chan_prototype(chan.HANN, 2 ** 40, 2 ** 40, out), "overflow")
    err(lib.aeth_chan_prototype(chan.HANN, 4, 2, None), "null")
    assert list(out) == [7.0] * 8                                   # nothing was written


A = C.c_void_p(0x100000)             # never dereferenced: 16-byte aligned "device" addresses, 1 MiB apart
B = C.c_void_p(0x200000)


def test_null_handles_and_null_contexts_are_refused_without_a_device(lib):
    w = (C.c_float * 16)(*([1.0] * 16))
    h = C.c_void_p(0x55)
    assert lib.aeth_chan_create(None, w, 16, 4, 4, 0, 0, C.byref(h)) == _lib.E_ARG and not h.value     # cleared, as aeth_fir_create does
    assert b"ctx" in lib.aeth_last_error() and b"null" in lib.aeth_last_error()
    assert lib.aeth_chan_create(None, w, 16, 4, 4, 0, 0, None) == _lib.E_ARG
    for rc in (lib.aeth_chan_fold(None, None, A, 16, 0, B, 16),
               lib.aeth_chan_exec(None, None, A, 16, 0, 1, 0, 0.0, B, 16),
               lib.aeth_chan_exec_levels(None, None, A, 16, 0, 1, 0, 0.0, 0, 0, B, 16)):
        assert rc == _lib.E_ARG
        assert b"chan" in lib.aeth_last_error() and b"null" in lib.aeth_last_error()
    assert lib.aeth_chan_destroy(None) == _lib.OK
    assert lib.aeth_chan_channels(None) == 0 and lib.aeth_chan_ntaps(None) == 0 and lib.aeth_chan_hop(None) == 0
    assert lib.aeth_chan_phase(None) == 0 and lib.aeth_chan_tile(None) == 0 and lib.aeth_chan_route(None) == b""


def test_python_mirror_has_the_new_surface():
    import aether_primitives_amd as ap
    for name in ("fold", "exec", "levels", "frames", "route", "tile", "channels", "hop", "ntaps", "phase"):
        assert hasattr(ap.Channelizer, name), name
    assert callable(ap.chan.prototype) and ap.chan.PHASE_STREAM == 1
