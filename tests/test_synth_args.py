"""CPU: aeth_synth_dual_window against its formula in numpy f64, and the aeth_synth_* entry points refusing null handles
and null contexts before any device work (tests/test_chan_args.py does the same for the analysis bank)."""
import ctypes as C

import numpy as np
import pytest

from aether_primitives_amd import _lib
from aether_primitives_amd import chan, synth

CASES = ((8, 4, "hann"), (16, 4, "hann"), (8, 3, "hamming"), (100, 50, "hann"), (5, 2, "hamming"), (8, 1, "hann"),
         (2048, 512, "hann"))                                       # (M, D, window)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def ulps_apart(a, b):
    """distance of two float32 arrays in units in the last place (both finite, same sign or zero)"""
    ia, ib = (v.view(np.int32).astype(np.int64) for v in (a, b))
    ia, ib = (np.where(i < 0, -(i & 0x7fffffff), i) for i in (ia, ib))
    return np.abs(ia - ib)


def formula(w, D):
    w = w.astype(np.float64)
    den = np.zeros(D)
    np.add.at(den, np.arange(w.size) % D, w * w)
    return w / den[np.arange(w.size) % D]


@pytest.mark.parametrize("M,D,kind", CASES)
def test_dual_window_is_the_formula_rounded_once(M, D, kind):
    w = chan.prototype(kind, M, 1)
    got = synth.dual_window(w, D)
    assert got.dtype == np.float32 and got.size == M
    want = formula(w, D)
    # the two f64 evaluations differ by far less than an f32 ulp: only a rounding tie can move a tap, by one ulp
    assert ulps_apart(got, want.astype(np.float32)).max() <= 1, (M, D, kind)
    # what the window is for: sum over the hops of g w is 1 at every offset
    rec = np.zeros(D)
    np.add.at(rec, np.arange(M) % D, got.astype(np.float64) * w.astype(np.float64))
    assert np.abs(rec - 1).max() <= M / D * 2.0 ** -23


def test_dual_window_refusals(lib):
    w = (C.c_float * 8)(*chan.prototype("hann", 8, 1))
    out = (C.c_float * 8)(*([7.0] * 8))

    def err(rc, *words):
        msg = lib.aeth_last_error().decode()
        assert rc == _lib.E_ARG, (rc, msg)
        assert all(x in msg for x in words), msg

    err(lib.aeth_synth_dual_window(None, 8, 4, out), "null")
    err(lib.aeth_synth_dual_window(w, 8, 4, None), "null")
    err(lib.aeth_synth_dual_window(w, 0, 4, out), "0 taps")
    err(lib.aeth_synth_dual_window(w, 8, 0, out), "hop 0")
    err(lib.aeth_synth_dual_window(w, 8, 9, out), "hop 9", "8 taps")
    err(lib.aeth_synth_dual_window(w, 8, 8, out), "j = 0", "2^-20")            # periodic Hann: w[0] = 0
    tiny = (C.c_float * 8)(*([1.0] * 5 + [2.0 ** -11] + [1.0] * 2))
    err(lib.aeth_synth_dual_window(tiny, 8, 8, out), "j = 5")
    assert list(out) == [7.0] * 8                                   # nothing was written
    with pytest.raises(_lib.AetherError):
        synth.dual_window(chan.prototype("hann", 8, 1), 8)
    assert lib.aeth_synth_dual_window(w, 8, 4, out) == _lib.OK and list(out) != [7.0] * 8


A = C.c_void_p(0x100000)             # never dereferenced: 16-byte aligned "device" addresses, 1 MiB apart
B = C.c_void_p(0x200000)


def test_null_handles_and_null_contexts_are_refused_without_a_device(lib):
    w = (C.c_float * 16)(*([1.0] * 16))
    h = C.c_void_p(0x55)
    assert lib.aeth_synth_create(None, w, 16, 4, 4, 0, 0, C.byref(h)) == _lib.E_ARG and not h.value     # cleared, as aeth_chan_create does
    assert b"ctx" in lib.aeth_last_error() and b"null" in lib.aeth_last_error()
    assert lib.aeth_synth_create(None, w, 16, 4, 4, 0, 0, None) == _lib.E_ARG
    for rc in (lib.aeth_synth_unfold(None, None, A, 16, 0, B, 16),
               lib.aeth_synth_exec(None, None, A, 16, 0, 1, 0, 0.0, B, 16)):
        assert rc == _lib.E_ARG
        assert b"synth" in lib.aeth_last_error() and b"null" in lib.aeth_last_error()
    assert lib.aeth_synth_destroy(None) == _lib.OK
    assert lib.aeth_synth_channels(None) == 0 and lib.aeth_synth_ntaps(None) == 0 and lib.aeth_synth_hop(None) == 0
    assert lib.aeth_synth_phase(None) == 0 and lib.aeth_synth_tile(None) == 0 and lib.aeth_synth_route(None) == b""
    assert lib.aeth_synth_history(None) == 0


def test_python_mirror_has_the_new_surface():
    import aether_primitives_amd as ap
    for name in ("unfold", "exec", "history", "samples", "route", "tile", "channels", "hop", "ntaps", "phase"):
        assert hasattr(ap.Synthesizer, name), name
    assert callable(ap.synth.dual_window) and ap.synth.Synthesizer is ap.Synthesizer
    assert "synth" in ap.__all__ and "Synthesizer" in ap.__all__
