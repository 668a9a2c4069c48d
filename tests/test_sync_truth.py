"""CPU: the restatement of the estimators' terms (tests/sync_truth.py) against complex128 closed forms, and the three host
helpers against their formulas.

Bounds.  One sq() of a value with relative error e has relative error 2 e + sqrt(5) u, u = 2^-24 (two rounded products
and a rounded difference in the real part: 2 u |a|^2; one rounded product, doubled exactly, in the imaginary part:
u |a|^2), so pw_M stays within (2 M - 1) sqrt(5) u for M = 2, 4, 8; the oscillator's phasor is within 1.5e-7 of
exp(2 pi j w / 2^64) (include/aether_hip.h); the f64 steps add a few 2^-53, covered by the factor 1 + 1e-6."""
import ctypes as C
import math

import numpy as np
import pytest

import nco_truth
import sync_truth as st
from aether_primitives_amd import _lib, nco, sync

U = 2.0 ** -24
NCO_ERR = 1.5e-7
WORDS = (0x1234_5678_9abc_def0, nco.word(0.0123), nco.word(3e-7))


def chain_bound(m):
    return (2 * m - 1) * math.sqrt(5) * U


def data(n=4096, seed=3):
    r = np.random.default_rng(seed)
    return ((r.standard_normal(n) + 1j * r.standard_normal(n)) * r.uniform(0.25, 4.0, n)).astype(np.complex64)


@pytest.mark.parametrize("words", (None, WORDS))
@pytest.mark.parametrize("kind", st.KINDS)
def test_line_terms_against_complex128(kind, words):
    x = data()
    n0 = 2 ** 40 + 17
    t_re, t_im, wt = st.line_terms(x, kind, words, n0)
    z = x.astype(np.complex128)
    ph = np.ones(x.size, np.complex128) if words is None else \
        nco_truth.phasor_f64([nco_truth.word_int(words, n0 + i) for i in range(x.size)])
    if kind == st.SQUARE:
        f = z.real ** 2 + z.imag ** 2                    # exact products, one rounding (np.abs(z) ** 2 rounds three times)
        want, scale, rel = f * ph, f, NCO_ERR
        assert np.all(np.abs(wt - f) <= 2.0 ** -52 * f)
    else:
        want, scale, rel = z ** kind * ph, np.abs(z) ** kind, chain_bound(kind) + NCO_ERR
        assert np.all(np.abs(wt - scale ** 2) <= 2 * chain_bound(kind) * (1 + 1e-6) * scale ** 2)
    err = np.abs((t_re + 1j * t_im) - want)
    print(kind, words is not None, float((err / scale).max()), rel)
    assert np.all(err <= rel * (1 + 1e-6) * scale)


@pytest.mark.parametrize("lag", (1, 5))
@pytest.mark.parametrize("power", st.POWERS)
def test_lag_terms_against_complex128(power, lag):
    x, hist = data(), data(lag, seed=4)
    for h in (None, hist):
        t_re, t_im, wt, exists = st.lag_terms(x, power, lag, h)
        assert exists.sum() == x.size - (lag if h is None else 0) and exists[lag:].all()
        z = x.astype(np.complex128)
        prev = np.concatenate([(np.zeros(lag) if h is None else h).astype(np.complex128), z])[:x.size]
        want = z ** power * np.conj(prev ** power)
        scale = np.abs(z) ** power * np.abs(prev) ** power
        err = np.abs((t_re + 1j * t_im) - want)[exists]
        assert np.all(err <= 2 * chain_bound(power) * (1 + 1e-6) * scale[exists])
        assert np.all(np.abs(wt - np.abs(z) ** (2 * power)) <= 2 * chain_bound(power) * (1 + 1e-6) * np.abs(z) ** (2 * power))


def test_reference_records_count_and_sum():
    x = data(100)
    t = st.line_terms(x, st.POW2)
    rec, mag = st.records(*t, 7)
    assert rec.size == 15 and rec["n"].sum() == 100 and rec["n"][-1] == 2 and not rec["n_nonfinite"].any()
    assert abs(rec["re"].sum() - math.fsum(t[0])) <= 1e-12 * mag[:, 0].sum()


def rec_of(re, im):
    return _lib.SyncRecord(re, im, 1.0, 1, 0, 0)


def test_turns():
    lib = _lib.load()
    assert lib.aeth_sync_turns(None) == 0.0
    assert sync.turns(rec_of(0.0, 0.0)) == 0.0 and sync.turns(rec_of(-0.0, 0.0)) == 0.0
    assert sync.turns(rec_of(1.0, 1.0)) == 0.125 and sync.turns(rec_of(0.0, -2.0)) == -0.25 and sync.turns(rec_of(-1.0, 0.0)) == 0.5
    r = np.random.default_rng(1)
    for re, im in r.standard_normal((64, 2)):
        assert sync.turns(rec_of(re, im)) == math.atan2(im, re) / (2 * math.pi)
        assert sync.turns(complex(re, im)) == st.turns(re, im)
    assert math.isnan(sync.turns(rec_of(float("nan"), 1.0)))


def test_freq_step():
    lib = _lib.load()
    assert sync.freq_step(rec_of(1.0, 1.0), 4, 2) == nco.word(-1 / 64) == 2 ** 64 - 2 ** 58
    assert sync.freq_step(rec_of(1.0, -1.0), 4, 2) == nco.word(1 / 64) == 2 ** 58
    assert lib.aeth_sync_freq_step(None, 4, 1) == 0 and sync.freq_step(rec_of(0.0, 0.0), 4, 1) == 0
    assert sync.freq_step(rec_of(1.0, 1.0), 0, 2) == 0 and sync.freq_step(rec_of(1.0, 1.0), 4, 0) == 0
    r = np.random.default_rng(2)
    for re, im in r.standard_normal((64, 2)):
        for power, lag in ((1, 1), (4, 1), (8, 1000), (2, 2 ** 20)):
            t = math.atan2(im, re) / (2 * math.pi)
            assert sync.freq_step(rec_of(re, im), power, lag) == nco.word(-t / (float(power) * float(lag)))


def test_timing_phase():
    lib = _lib.load()
    assert lib.aeth_sync_timing_phase(None, 4.0) == 0
    assert sync.timing_phase(rec_of(0.0, -1.0), 4.0) == 1 << 32                     # turns = -1/4: one sample into the symbol
    assert sync.timing_phase(rec_of(0.0, 1.0), 4.0) == 3 << 32                      # turns = +1/4: frac(-1/4) = 3/4
    assert sync.timing_phase(rec_of(1.0, 0.0), 4.0) == 0
    for bad in (0.0, -4.0, float("nan"), float("inf"), 2.0 ** 31 + 1):
        assert sync.timing_phase(rec_of(0.0, -1.0), bad) == 0
    r = np.random.default_rng(3)
    for re, im in r.standard_normal((64, 2)):
        for sps in (2.0, 4.0, 8.25, 1000.0):
            t = -math.atan2(im, re) / (2 * math.pi)
            f = t - math.floor(t)
            f = f if f < 1.0 else 0.0
            assert sync.timing_phase(rec_of(re, im), sps) == int(f * sps * 4294967296.0)


def test_python_mirror_has_the_new_surface():
    import aether_primitives_amd as ap
    for name in ("line", "lag", "line_into", "lag_into", "turns", "freq_step", "timing_phase", "chunk", "DeviceRecords"):
        assert hasattr(ap.sync, name), name
    assert "sync" in ap.__all__
    assert C.sizeof(_lib.SyncRecord) == 48 == sync.RECORD_DTYPE.itemsize == st.RECORD_DTYPE.itemsize
    assert sync.chunk() >= 64 and sync.chunk() % 2 == 0
    assert (sync.SQUARE, sync.POW1, sync.POW2, sync.POW4, sync.POW8) == st.KINDS
