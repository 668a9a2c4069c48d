"""CPU: the oscillator's host entry points.  aeth_nco_word against its rule, aeth_nco_word_at against Python integers,
aeth_nco_phasor bit for bit against the numpy restatement (tests/nco_truth.py; the kernels run the same text), and the
device calls refusing null arguments before any device work."""
import ctypes as C
import math

import numpy as np
import pytest

import nco_truth
from aether_primitives_amd import _lib
from aether_primitives_amd import nco


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def rule(cycles):
    """frac(cycles) * 2^64 truncated toward zero, in exact arithmetic on the f64 fraction"""
    if math.isnan(cycles) or math.isinf(cycles):
        return 0
    x = cycles - math.floor(cycles)                 # f64, as the definition says
    if x >= 1.0:
        return 0
    num, den = x.as_integer_ratio()
    return (num << 64) // den


@pytest.mark.parametrize("cycles", (0.0, 0.25, -0.25, 1.0, 1e-30, -1e-30, 0.5 - 2.0 ** -54, float("nan"), float("inf"), -float("inf"),
                                    0.2, -0.1, 123456.789, -2.0 ** -64, 1.0 - 2.0 ** -53))
def test_word_follows_its_rule(cycles):
    assert nco.word(cycles) == rule(cycles), cycles


def test_word_values():
    assert nco.word(0.0) == 0 and nco.word(1.0) == 0 and nco.word(float("nan")) == 0
    assert nco.word(0.25) == 1 << 62 and nco.word(-0.25) == 3 << 62 and nco.word(0.5) == 1 << 63
    assert nco.word(1e-30) == 0 and nco.word(-1e-30) == 0           # the fraction of -1e-30 rounds to 1.0
    assert nco.word(0.5 - 2.0 ** -54) == (1 << 63) - (1 << 10)
    assert nco.word(1.0 - 2.0 ** -53) == (1 << 64) - (1 << 11)


def test_word_at_equals_python_integers(lib):
    rng = np.random.default_rng(5)
    sets = [tuple(int(v) for v in rng.integers(0, 2 ** 64, 3, dtype=np.uint64)) for _ in range(4)]
    sets += [(0, 0, 0), (2 ** 64 - 1,) * 3, (1, 2 ** 63, 2 ** 63)]
    for words in sets:
        for n in (0, 1, 2, 3, 2 ** 31 + 5, 2 ** 40 + 7, 2 ** 63, 2 ** 63 + 1, 2 ** 64 - 2, 2 ** 64 - 1):
            assert nco.word_at(words, n) == nco_truth.word_int(words, n), (words, n)
    assert lib.aeth_nco_word_at(None, 5) == 0


def boundary_words():
    out = [0, 1 << 62, 1 << 63, 3 << 62, (1 << 64) - 1]
    for k in range(4):
        b = (k << 62) + (1 << 61)
        out += [(b - 1) % 2 ** 64, b, b + (1 << 32), b - (1 << 32)]
    return out


def test_phasor_is_the_restatement_bit_for_bit(lib):
    rng = np.random.default_rng(9)
    w = np.concatenate([rng.integers(0, 2 ** 64, 1 << 16, dtype=np.uint64), np.array(boundary_words(), np.uint64)])
    c, d = nco_truth.phasor(w)
    got = np.empty(w.size, np.complex64)
    out = _lib.Cf32()
    for i, v in enumerate(w.tolist()):
        assert lib.aeth_nco_phasor(v, C.byref(out)) == _lib.OK
        got[i] = complex(out.re, out.im)
    assert (got.real.view(np.uint32) == c.view(np.uint32)).all()
    assert (got.imag.view(np.uint32) == d.view(np.uint32)).all()


def test_cardinal_words_are_exact():
    bits = lambda z: np.array([z.real, z.imag], np.float32).view(np.uint32).tolist()          # noqa: E731
    assert bits(nco.phasor(0)) == [0x3f800000, 0x00000000]
    assert bits(nco.phasor(1 << 62)) == [0x80000000, 0x3f800000]
    assert bits(nco.phasor(1 << 63)) == [0xbf800000, 0x80000000]
    assert bits(nco.phasor(3 << 62)) == [0x00000000, 0xbf800000]


A = C.c_void_p(0x100000)             # never dereferenced: 16-byte aligned "device" addresses, 1 MiB apart
B = C.c_void_p(0x200000)


def test_null_arguments_are_refused_without_a_device(lib):
    w = nco._Words(1, 2, 3)
    for n in (0, 16):
        assert lib.aeth_nco_mix(None, C.byref(w), 0, A, B, n) == _lib.E_ARG
        assert b"ctx" in lib.aeth_last_error() and b"null" in lib.aeth_last_error()
        assert lib.aeth_nco_tone(None, C.byref(w), 0, 1.0, B, n) == _lib.E_ARG
        assert b"ctx" in lib.aeth_last_error() and b"null" in lib.aeth_last_error()
    assert lib.aeth_nco_phasor(0, None) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    # behind a context: the handle below is never followed, every one of these returns before any device work
    fake = (C.c_char * 4096)()
    ctx = C.cast(fake, C.c_void_p)
    assert lib.aeth_nco_mix(ctx, None, 0, A, B, 16) == _lib.E_ARG and b"words" in lib.aeth_last_error()
    assert lib.aeth_nco_tone(ctx, None, 0, 1.0, B, 16) == _lib.E_ARG and b"words" in lib.aeth_last_error()
    assert lib.aeth_nco_mix(ctx, C.byref(w), 0, None, B, 16) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_nco_mix(ctx, C.byref(w), 0, A, None, 16) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_nco_tone(ctx, C.byref(w), 0, 1.0, None, 16) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert lib.aeth_nco_mix(ctx, C.byref(w), 0, None, None, 0) == _lib.OK          # n == 0: nothing to do
    assert lib.aeth_nco_tone(ctx, C.byref(w), 0, 1.0, None, 0) == _lib.OK
    assert lib.aeth_nco_mix(ctx, C.byref(w), 0, C.c_void_p(0x100004), B, 16) == _lib.E_ALIGN
    assert lib.aeth_nco_mix(ctx, C.byref(w), 2 ** 64 - 16, A, B, 16) == _lib.E_UNSUPPORTED
    msg = lib.aeth_last_error().decode()
    assert str(2 ** 64 - 16) in msg and "16 samples" in msg, msg
    assert lib.aeth_nco_mix(ctx, C.byref(w), 0, A, C.c_void_p(0x100008), 16) == _lib.E_ARG and b"overlaps" in lib.aeth_last_error()


def test_python_mirror_has_the_new_surface():
    import aether_primitives_amd as ap
    for name in ("mix", "tone", "seek", "words", "from_words"):
        assert hasattr(ap.Nco, name), name
    assert callable(ap.nco.word) and callable(ap.nco.word_at) and callable(ap.nco.phasor) and ap.nco.Nco is ap.Nco
    assert "nco" in ap.__all__ and "Nco" in ap.__all__
