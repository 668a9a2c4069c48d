"""CPU: aeth_corr_create, aeth_corr_exec, aeth_corr_exec_levels and aeth_corr_search validate their arguments before any
device work, as the other entry points do (tests/test_stats_levels_args.py): every bad call returns its AETH_E_* code
with a message and touches nothing.

Neither a context nor a correlator can be created without a device.  aeth_corr_create receives the address of a zeroed
block as its context (validation only asks whether the pointer is null).  The exec calls need to read the correlator's
lengths, so they receive a hand-made object: struct aeth_corr is one pointer to the filter built from the conj-reversed
template, and struct aeth_fir starts with {ctx, ntaps, fft_len, hop} (csrc/aeth_fft_plan.h); the rest of the filter stays
zero and is never reached, because each of these calls is refused before the device is looked at (a call that passed
validation would go on to the device and is not made here)."""
import ctypes as C

import numpy as np
import pytest

from aether_primitives_amd import _lib


class _Fir(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("ntaps", C.c_size_t), ("fft_len", C.c_size_t), ("hop", C.c_size_t),
                ("fft", C.c_void_p), ("Hf", C.c_void_p), ("spare", C.c_char * 64)]


class _Corr(C.Structure):
    _fields_ = [("fir", C.POINTER(_Fir)), ("spare", C.c_char * 64)]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def fake_ctx():
    block = (C.c_char * 4096)()
    return C.cast(block, C.c_void_p), block


def fake_corr(ctx, nref=64, fft_len=2048):
    """what aeth_corr_create would have built for these lengths (hop: aeth_fir_create's rounding to 64 samples)"""
    L = fft_len - nref + 1
    fir = _Fir(ctx=ctx, ntaps=nref, fft_len=fft_len, hop=(L // 64) * 64 if fft_len >= 512 and L >= 64 else L)
    corr = _Corr(fir=C.pointer(fir))
    return C.cast(C.pointer(corr), C.c_void_p), (fir, corr)


def _err(lib, rc, code, *words):
    assert rc == code, (rc, lib.aeth_last_error())
    msg = lib.aeth_last_error().decode()
    assert msg and all(w in msg for w in words), msg


X = C.c_void_p(0x100000)            # never dereferenced: 16-byte aligned "device" addresses, 1 MiB apart
H = C.c_void_p(0x200000)
OUT = C.c_void_p(0x300000)
N = 5000                            # three blocks of 1984


def test_the_peak_record_is_16_bytes_without_padding():
    from aether_primitives_amd.corr import _CorrPeak, PEAK_DTYPE
    assert C.sizeof(_CorrPeak) == 16 and PEAK_DTYPE.itemsize == 16
    assert (_CorrPeak.index.offset, _CorrPeak.norm.offset, _CorrPeak.n_nan.offset) == (0, 8, 12)
    assert [PEAK_DTYPE.fields[k][1] for k in ("index", "norm", "n_nan")] == [0, 8, 12]


def test_create_arguments(lib, fake_ctx):
    ctx, _ = fake_ctx
    ref = np.ones(64, np.complex64)
    rp = ref.ctypes.data_as(C.c_void_p)
    out = C.c_void_p(0x55)
    _err(lib, lib.aeth_corr_create(None, rp, 64, 2048, C.byref(out)), _lib.E_ARG, "null")
    _err(lib, lib.aeth_corr_create(ctx, rp, 64, 2048, None), _lib.E_ARG, "null")
    _err(lib, lib.aeth_corr_create(ctx, None, 64, 2048, C.byref(out)), _lib.E_ARG, "template")
    assert not out.value                                             # cleared, as aeth_fir_create does
    _err(lib, lib.aeth_corr_create(ctx, rp, 0, 2048, C.byref(out)), _lib.E_ARG, "template")
    _err(lib, lib.aeth_corr_create(ctx, rp, 64, 2000, C.byref(out)), _lib.E_UNSUPPORTED, "power of two")
    _err(lib, lib.aeth_corr_create(ctx, rp, 64, 8192, C.byref(out)), _lib.E_UNSUPPORTED, "power of two")
    _err(lib, lib.aeth_corr_create(ctx, rp, 64, 64, C.byref(out)), _lib.E_ARG, "fft_len 64 < 2*nref")
    _err(lib, lib.aeth_corr_create(ctx, rp, 33, 64, C.byref(out)), _lib.E_ARG, "2*nref")
    assert not out.value
    assert lib.aeth_corr_destroy(None) == _lib.OK
    assert lib.aeth_corr_nref(None) == 0 and lib.aeth_corr_fft_len(None) == 0 and lib.aeth_corr_hop(None) == 0


def test_accessors_read_the_filter(lib, fake_ctx):
    corr, keep = fake_corr(fake_ctx[0], 64, 2048)
    assert (lib.aeth_corr_nref(corr), lib.aeth_corr_fft_len(corr), lib.aeth_corr_hop(corr)) == (64, 2048, 1984)


def test_exec_arguments(lib, fake_ctx):
    corr, keep = fake_corr(fake_ctx[0])
    _err(lib, lib.aeth_corr_exec(None, None, X, N, OUT), _lib.E_ARG, "corr", "null")
    _err(lib, lib.aeth_corr_exec(corr, None, None, N, OUT), _lib.E_ARG, "null")
    _err(lib, lib.aeth_corr_exec(corr, None, X, N, None), _lib.E_ARG, "null")
    # the refusals of aeth_fir_exec, with its texts
    for out in (X.value, X.value + 800, X.value + N * 8 - 8, X.value - N * 8 + 8):
        _err(lib, lib.aeth_corr_exec(corr, None, X, N, C.c_void_p(out)), _lib.E_ARG, "FIR cannot run in place", "overlaps the input")
    _err(lib, lib.aeth_corr_exec(corr, H, X, N, C.c_void_p(H.value + 62 * 8)), _lib.E_ARG, "FIR cannot run in place", "history")
    for bad in ((None, C.c_void_p(X.value + 4), OUT), (None, X, C.c_void_p(OUT.value + 4)), (C.c_void_p(H.value + 4), X, OUT)):
        _err(lib, lib.aeth_corr_exec(corr, bad[0], bad[1], N, bad[2]), _lib.E_ALIGN, "not 8-byte aligned")
    assert lib.aeth_corr_exec(corr, None, None, 0, None) == _lib.OK  # an empty stream is no error and no launch


def test_levels_arguments(lib, fake_ctx):
    corr, keep = fake_corr(fake_ctx[0])
    f = lib.aeth_corr_exec_levels
    _err(lib, f(None, None, X, N, 0, OUT, N), _lib.E_ARG, "corr", "null")
    _err(lib, f(corr, None, None, N, 0, OUT, N), _lib.E_ARG, "null")
    _err(lib, f(corr, None, X, N, 0, None, N), _lib.E_ARG, "null")
    _err(lib, f(corr, None, X, N, 0, OUT, N - 1), _lib.E_LEN, "same length")
    _err(lib, f(corr, None, X, N, 0, OUT, N + 1), _lib.E_LEN, "same length")
    for kind in (-1, 3, 99):
        _err(lib, f(corr, None, X, N, kind, OUT, N), _lib.E_ARG, "level kind")
    _err(lib, f(corr, None, C.c_void_p(X.value + 4), N, 0, OUT, N), _lib.E_ALIGN, "aligned")
    _err(lib, f(corr, C.c_void_p(H.value + 4), X, N, 0, OUT, N), _lib.E_ALIGN, "aligned")
    _err(lib, f(corr, None, X, N, 0, C.c_void_p(OUT.value + 2), N), _lib.E_ALIGN, "4-byte aligned")
    # the levels inside, at the start of, straddling the end of and straddling the start of the input: refused
    for lv in (X.value, X.value + 64, X.value + N * 8 - 4, X.value - N * 4 + 4):
        _err(lib, f(corr, None, X, N, 0, C.c_void_p(lv), N), _lib.E_ARG, "overlaps the input")
    # ... and touching the 63 samples of history
    _err(lib, f(corr, H, X, N, 0, C.c_void_p(H.value + 62 * 8 + 4), N), _lib.E_ARG, "overlaps", "history")
    _err(lib, f(corr, H, X, N, 0, C.c_void_p(H.value - N * 4 + 4), N), _lib.E_ARG, "overlaps", "history")
    assert f(corr, None, X, 0, 0, OUT, 0) == _lib.OK and f(corr, None, None, 0, 2, None, 0) == _lib.OK


def test_search_arguments(lib, fake_ctx):
    corr, keep = fake_corr(fake_ctx[0])
    f = lib.aeth_corr_search
    best = (C.c_char * 16)(*([0x5a] * 16))
    _err(lib, f(None, None, X, N, OUT, 3, best), _lib.E_ARG, "corr", "null")
    _err(lib, f(corr, None, X, N, None, 0, None), _lib.E_ARG, "both null")
    _err(lib, f(corr, None, X, N, None, 3, None), _lib.E_ARG, "both null")
    _err(lib, f(corr, None, X, 0, None, 0, best), _lib.E_LEN, "empty")
    # ceil(5000 / 1984) = 3 records; n a multiple of the hop: exactly n / hop
    for n_peaks in (0, 2, 4, N):
        _err(lib, f(corr, None, X, N, OUT, n_peaks, best), _lib.E_LEN, "3 blocks")
    _err(lib, f(corr, None, X, 2 * 1984, OUT, 3, None), _lib.E_LEN, "2 blocks")
    _err(lib, f(corr, None, X, 2 * 1984 + 1, OUT, 2, None), _lib.E_LEN, "3 blocks")
    _err(lib, f(corr, None, None, N, OUT, 3, best), _lib.E_ARG, "null")
    _err(lib, f(corr, None, C.c_void_p(X.value + 4), N, OUT, 3, best), _lib.E_ALIGN, "aligned")
    _err(lib, f(corr, None, X, N, C.c_void_p(OUT.value + 4), 3, best), _lib.E_ALIGN, "aligned")
    _err(lib, f(corr, None, X, N, C.c_void_p(X.value + 16), 3, best), _lib.E_ARG, "overlaps")
    _err(lib, f(corr, H, X, N, C.c_void_p(H.value + 8), 3, None), _lib.E_ARG, "overlaps")
    assert bytes(best) == bytes([0x5a] * 16)                         # nothing was written


def test_fused_calls_refuse_lengths_without_a_build(lib, fake_ctx):
    """fft_len 512 (and every other length outside 1024 .. 4096) filters, but carries no level or peak build"""
    best = (C.c_char * 16)()
    for fft_len in (64, 512):
        corr, keep = fake_corr(fake_ctx[0], 16, fft_len)
        hop = lib.aeth_corr_hop(corr)
        _err(lib, lib.aeth_corr_exec_levels(corr, None, X, N, 0, OUT, N), _lib.E_UNSUPPORTED, f"fft_len {fft_len}", "1024 .. 4096")
        _err(lib, lib.aeth_corr_search(corr, None, X, N, OUT, -(-N // hop), best), _lib.E_UNSUPPORTED, f"fft_len {fft_len}", "1024 .. 4096")
        _err(lib, lib.aeth_corr_search(corr, None, X, N, None, 0, best), _lib.E_UNSUPPORTED, f"fft_len {fft_len}")
    assert bytes(best) == bytes(16)


def test_python_mirror_has_the_new_surface():
    import aether_primitives_amd as ap
    for name in ("correlate", "levels", "search"):
        assert callable(getattr(ap.Corr, name)), name
    assert {"index", "lag", "norm", "n_nan"} <= set(ap.CorrPeak.__slots__)
