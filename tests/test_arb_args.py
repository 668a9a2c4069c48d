"""CPU: aeth_arb_advance against Python integers, and the aeth_arb_* entry points refusing their arguments before any
device work (tests/test_resamp_args.py does the same for the rational resampler).

aeth_arb_create checks every argument before it uses the context, so its refusals are reached here with a context
pointer that is never followed.  aeth_arb_exec needs an object for everything but a null handle: its other refusals,
with the proof that nothing was launched and nothing stays allocated, are in tests/test_gpu_arb.py."""
import ctypes as C

import numpy as np
import pytest

from aether_primitives_amd import _lib
from aether_primitives_amd import arb

import arb_truth

ONE = 1 << 32
MIN_STEP, MAX_STEP = 1 << 20, 1 << 44


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def word(ratio):
    return int(float(ratio) * 4294967296.0)


ADVANCE = [
    # (step, phase, n)
    (ONE, 0, 0), (ONE, 0, 1), (ONE, 0, 1000), (ONE - 1, 0, 1000), (ONE + 1, 0, 1000),
    (word(0.731), 0, 977), (word(160 / 147 * (1 + 2e-5)), 0, 48000), (word(64.3), 0, 7),
    (ONE, ONE - 1, 1), (ONE, ONE - 1, 1000), (word(0.731), ONE - 1, 977), (word(4.0001), ONE - 1, 3),
    (ONE, 5 * ONE, 5), (ONE, 5 * ONE + 1, 5), (word(64.3), 40 * ONE + 99, 7), (ONE, 5 * ONE - 1, 5),    # phase at or past the end: 0
    (MIN_STEP, 0, 1), (MIN_STEP, ONE - 1, 3), (MIN_STEP, 0, 1 << 20), (MAX_STEP, 0, 1), (MAX_STEP, 0, 4096), (MAX_STEP, 0, 4097),
    (MAX_STEP, ONE - 1, 3 * 4096 + 1),
    (ONE, 0, 1 << 31), (MIN_STEP, 0, 1 << 31), (MAX_STEP, (1 << 63) - 1, 1 << 31), (word(0.731), 12345, 1 << 31),
    (MIN_STEP, (1 << 63) - 1, 1 << 31), (MAX_STEP, 0, 1 << 31),
]


@pytest.mark.parametrize("step,phase,n", ADVANCE)
def test_advance_is_the_integer_formula(step, phase, n):
    want = arb_truth.advance(step, phase, n)
    assert arb.advance(step, phase, n) == want
    count, nxt = want
    # what the formula means: output count - 1 lies inside the call, output count does not
    assert count == 0 or phase + (count - 1) * step < n * ONE
    assert phase + count * step >= n * ONE and nxt == phase + count * step - n * ONE
    assert arb.ArbResampler.advance(step, phase, n) == want


def test_step_word_truncates():
    assert arb.step_word(1.0) == ONE and arb.step_word(0.5) == 1 << 31 and arb.step_word(4096) == MAX_STEP
    assert arb.step_word(2.0 ** -12) == MIN_STEP
    assert arb.step_word(1.0000123) == int(1.0000123 * 2.0 ** 32)
    assert arb.step_word(1 + 2.0 ** -33) == ONE                      # truncated, not rounded
    assert arb.step_word(160 / 147 * (1 + 2e-5)) == word(160 / 147 * (1 + 2e-5))


def test_advance_refusals_name_the_number(lib):
    count, nxt = C.c_size_t(77), C.c_uint64(78)

    def err(rc, code, *words):
        msg = lib.aeth_last_error().decode()
        assert rc == code, (rc, msg)
        assert all(w in msg for w in words), msg
        assert count.value == 77 and nxt.value == 78                  # nothing was written

    adv = lambda s, p, n: lib.aeth_arb_advance(s, p, n, C.byref(count), C.byref(nxt))      # noqa: E731
    err(adv(MIN_STEP - 1, 0, 10), _lib.E_UNSUPPORTED, f"step {MIN_STEP - 1}", "2^20")
    err(adv(MAX_STEP + 1, 0, 10), _lib.E_UNSUPPORTED, f"step {MAX_STEP + 1}", "2^44")
    err(adv(0, 0, 10), _lib.E_UNSUPPORTED, "step 0")
    err(adv(2 ** 64 - 1, 0, 10), _lib.E_UNSUPPORTED, f"step {2 ** 64 - 1}")
    err(adv(ONE, 1 << 63, 10), _lib.E_UNSUPPORTED, f"phase {1 << 63}", "2^63")
    err(adv(ONE, 2 ** 64 - 1, 10), _lib.E_UNSUPPORTED, f"phase {2 ** 64 - 1}")
    err(adv(ONE, 0, (1 << 31) + 1), _lib.E_UNSUPPORTED, f"{(1 << 31) + 1} input samples", "2^31")
    err(adv(ONE, 0, 2 ** 64 - 1), _lib.E_UNSUPPORTED, f"{2 ** 64 - 1} input samples")
    err(lib.aeth_arb_advance(ONE, 0, 10, None, C.byref(nxt)), _lib.E_ARG, "null")
    err(lib.aeth_arb_advance(ONE, 0, 10, C.byref(count), None), _lib.E_ARG, "null")
    with pytest.raises(_lib.AetherError):
        arb.advance(MIN_STEP - 1, 0, 10)
    # within the three limits no intermediate reaches 2^64: phase + count * step < n * 2^32 + step <= 2^63 + 2^44, and the
    # corner itself is served
    assert adv(MAX_STEP, (1 << 63) - 1, 1 << 31) == _lib.OK
    assert (count.value, nxt.value) == arb_truth.advance(MAX_STEP, (1 << 63) - 1, 1 << 31)


CTX = C.c_void_p(0x100000)            # never followed: aeth_arb_create refuses before it uses the context
A = C.c_void_p(0x100000)              # never dereferenced: 16-byte aligned "device" addresses, 1 MiB apart
B = C.c_void_p(0x200000)


def test_create_refusals_come_before_the_context_is_used(lib):
    w = (C.c_float * 16)(*([1.0] * 16))
    h = C.c_void_p(0x55)

    def err(rc, code, *words):
        msg = lib.aeth_last_error().decode()
        assert rc == code, (rc, msg)
        assert all(x in msg for x in words), msg
        assert not h.value                                            # cleared, as aeth_resamp_create does
        h.value = 0x55

    err(lib.aeth_arb_create(None, w, 16, 2, C.byref(h)), _lib.E_ARG, "ctx", "null")
    assert lib.aeth_arb_create(CTX, w, 16, 2, None) == _lib.E_ARG and b"out is null" in lib.aeth_last_error()
    err(lib.aeth_arb_create(CTX, None, 16, 2, C.byref(h)), _lib.E_ARG, "taps", "null")
    err(lib.aeth_arb_create(CTX, w, 16, 13, C.byref(h)), _lib.E_UNSUPPORTED, "log2_phases 13", "12")
    err(lib.aeth_arb_create(CTX, w, 16, 2 ** 40, C.byref(h)), _lib.E_UNSUPPORTED, f"log2_phases {2 ** 40}")
    err(lib.aeth_arb_create(CTX, w, 0, 2, C.byref(h)), _lib.E_ARG, "0 taps")
    err(lib.aeth_arb_create(CTX, w, 15, 2, C.byref(h)), _lib.E_ARG, "15 taps", "4 phases")
    err(lib.aeth_arb_create(CTX, w, 16, 5, C.byref(h)), _lib.E_ARG, "16 taps", "32 phases")
    err(lib.aeth_arb_create(CTX, w, 65 * 4, 2, C.byref(h)), _lib.E_UNSUPPORTED, "65 taps per phase", "64")   # refused before a tap is read
    err(lib.aeth_arb_create(CTX, w, 65, 0, C.byref(h)), _lib.E_UNSUPPORTED, "65 taps per phase")


def test_null_handles_are_refused_without_a_device(lib):
    assert lib.aeth_arb_exec(None, None, A, 16, ONE, 0, B, 16) == _lib.E_ARG
    assert b"arb" in lib.aeth_last_error() and b"null" in lib.aeth_last_error()
    assert lib.aeth_arb_destroy(None) == _lib.OK
    assert lib.aeth_arb_phases(None) == 0 and lib.aeth_arb_ntaps(None) == 0 and lib.aeth_arb_history(None) == 0
    assert lib.aeth_arb_tile(None, ONE) == 0 and lib.aeth_arb_route(None, ONE) == b""


def test_python_mirror_has_the_new_surface():
    import aether_primitives_amd as ap
    for name in ("exec", "advance", "history", "route", "tile", "phases", "ntaps"):
        assert hasattr(ap.ArbResampler, name), name
    assert ap.arb.ArbResampler is ap.ArbResampler and ap.step_word is ap.arb.step_word
    assert "arb" in ap.__all__ and "ArbResampler" in ap.__all__ and "step_word" in ap.__all__


def test_deltas_are_one_f32_subtraction():
    """d[j] = fl32(h[j + 1] - h[j]) with h[T] = +0.0"""
    h = np.array([1.0, 1.0 + 2.0 ** -23, -3.5, 0.1], np.float32)
    d = arb_truth.deltas(h)
    assert d.dtype == np.float32 and d.tolist() == [np.float32(2.0 ** -23), np.float32(-3.5) - h[1], np.float32(0.1) + np.float32(3.5), -h[3]]
