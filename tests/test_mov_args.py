"""CPU: aeth_mov_exec and aeth_mov_search refuse every bad call with the status include/aether_hip.h names, before any
device work: the context handle below is never followed and the "device" addresses are never dereferenced.  Also the host
helpers: history, grid, and freq_step against its formula."""
import ctypes as C
import math

import pytest

from aether_primitives_amd import _lib, mov, nco

X = C.c_void_p(0x100000)             # 16-byte aligned "device" addresses, far apart
H = C.c_void_p(0x80000)
P = C.c_void_p(0x40000000)
R = C.c_void_p(0x50000000)
M = C.c_void_p(0x60000000)
K = C.c_void_p(0x70000000)
N = 4096
LAG, POWER = mov.LAG, mov.POWER


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def ctx():
    fake = (C.c_char * 4096)()
    return C.cast(fake, C.c_void_p), fake


def ex(lib, ctx, kind=LAG, window=16, lag=64, hist=H, x=X, n=N, p=P, r=R, m=M):
    return lib.aeth_mov_exec(ctx, kind, window, lag, hist, x, n, p, r, m)


def se(lib, ctx, kind=LAG, window=16, lag=64, r_min=0.0, threshold=0.5, hist=H, x=X, n=N, block=0, peaks=K, best=None):
    return lib.aeth_mov_search(ctx, kind, window, lag, r_min, threshold, hist, x, n, block, peaks, best)


def said(lib, *words):
    msg = lib.aeth_last_error().decode()
    return all(str(w) in msg for w in words)


def test_null_arguments(lib, ctx):
    ctx = ctx[0]
    assert ex(lib, None) == _lib.E_ARG and said(lib, "ctx")
    assert se(lib, None) == _lib.E_ARG and said(lib, "ctx")
    assert ex(lib, ctx, x=None) == _lib.E_ARG and said(lib, "null")
    assert se(lib, ctx, x=None) == _lib.E_ARG and said(lib, "null")
    assert ex(lib, ctx, p=None, r=None, m=None) == _lib.E_ARG and said(lib, "null")
    assert se(lib, ctx, peaks=None, best=None) == _lib.E_ARG and said(lib, "null")


def test_empty_input_is_a_length_error(lib, ctx):
    ctx = ctx[0]
    assert ex(lib, ctx, n=0) == _lib.E_LEN and said(lib, "empty")
    assert se(lib, ctx, n=0) == _lib.E_LEN and said(lib, "empty")


def test_kind_window_and_lag(lib, ctx):
    ctx = ctx[0]
    for call in (ex, se):
        for kind in (-1, 2, 7):
            assert call(lib, ctx, kind=kind) == _lib.E_ARG and said(lib, kind)
        assert call(lib, ctx, window=0) == _lib.E_ARG and said(lib, "window 0")
        assert call(lib, ctx, window=4097) == _lib.E_UNSUPPORTED and said(lib, 4097)
        assert call(lib, ctx, lag=0) == _lib.E_ARG and said(lib, "lag 0")
        assert call(lib, ctx, lag=65537, hist=None) == _lib.E_UNSUPPORTED and said(lib, 65537)
    assert ex(lib, ctx, kind=POWER, lag=3, p=None) == _lib.E_ARG and said(lib, "lag 3")
    assert se(lib, ctx, kind=POWER, lag=3) == _lib.E_ARG and said(lib, "lag 3")
    assert ex(lib, ctx, kind=POWER, lag=0) == _lib.E_ARG and said(lib, "p plane", hex(P.value))


def test_gate_and_threshold(lib, ctx):
    ctx = ctx[0]
    assert se(lib, ctx, r_min=-1.5) == _lib.E_ARG and said(lib, "r_min", "-1.5")
    assert se(lib, ctx, r_min=math.nan) == _lib.E_ARG and said(lib, "r_min", "nan")
    assert se(lib, ctx, threshold=math.nan) == _lib.E_ARG and said(lib, "threshold", "nan")


def test_alignment(lib, ctx):
    ctx = ctx[0]
    off = lambda p, k: C.c_void_p(p.value + k)            # noqa: E731
    for call in (ex, se):
        assert call(lib, ctx, x=off(X, 4)) == _lib.E_ALIGN and said(lib, hex(X.value + 4))
        assert call(lib, ctx, hist=off(H, 4)) == _lib.E_ALIGN and said(lib, hex(H.value + 4))
    assert ex(lib, ctx, p=off(P, 4)) == _lib.E_ALIGN and said(lib, hex(P.value + 4))
    assert ex(lib, ctx, r=off(R, 2)) == _lib.E_ALIGN and said(lib, hex(R.value + 2))
    assert ex(lib, ctx, m=off(M, 1)) == _lib.E_ALIGN and said(lib, hex(M.value + 1))
    assert se(lib, ctx, peaks=off(K, 4)) == _lib.E_ALIGN and said(lib, hex(K.value + 4))
    best = (C.c_char * 80)()
    assert se(lib, ctx, best=C.c_void_p((C.addressof(best) + 7) // 8 * 8 + 4)) == _lib.E_ALIGN


def test_overlapping_ranges(lib, ctx):
    ctx = ctx[0]
    hist_n = lib.aeth_mov_history(LAG, 16, 64)
    inside_x = C.c_void_p(X.value + 8 * (N - 1))
    inside_h = C.c_void_p(H.value + 8 * (hist_n - 1))
    for name in ("p", "r", "m"):
        assert ex(lib, ctx, **{name: inside_x}) == _lib.E_ARG and said(lib, "overlap", name + "_dev", "x_dev")
        assert ex(lib, ctx, **{name: inside_h}) == _lib.E_ARG and said(lib, "overlap", name + "_dev", "hist_dev")
    assert ex(lib, ctx, r=C.c_void_p(P.value + 8 * N - 4)) == _lib.E_ARG and said(lib, "overlap", "r_dev", "p_dev")
    assert ex(lib, ctx, m=C.c_void_p(R.value + 4 * N - 4)) == _lib.E_ARG and said(lib, "overlap", "m_dev", "r_dev")
    assert ex(lib, ctx, m=C.c_void_p(P.value)) == _lib.E_ARG and said(lib, "overlap", "m_dev", "p_dev")
    assert se(lib, ctx, peaks=inside_x) == _lib.E_ARG and said(lib, "overlap", "peaks_dev")
    assert se(lib, ctx, peaks=C.c_void_p(H.value + 8 * (hist_n - 1))) == _lib.E_ARG and said(lib, "overlap", "hist_dev")
    # room for 64 records in front of x; blocks of 63 samples make 66
    before = C.c_void_p(X.value - 64 * 64)
    assert se(lib, ctx, block=N // 64 - 1, peaks=before) == _lib.E_ARG and said(lib, "overlap")


def test_too_many_workgroups(lib, ctx):
    ctx = ctx[0]
    big = C.c_void_p(1 << 44)
    assert se(lib, ctx, n=2 ** 31, block=1, peaks=big) == _lib.E_UNSUPPORTED and said(lib, "2^31", 2 ** 31)
    assert se(lib, ctx, n=2 ** 31 * 2048, peaks=big) == _lib.E_UNSUPPORTED and said(lib, "2^31")
    assert ex(lib, ctx, n=2 ** 31 * 2048, p=None, r=None, m=C.c_void_p(1 << 46)) == _lib.E_UNSUPPORTED and said(lib, "2^31", 2 ** 42)


def test_history_and_grid():
    assert mov.history(LAG, 16, 64) == 79 and mov.history(LAG, 1, 1) == 1 and mov.history(LAG, 4096, 65536) == 4095 + 65536
    assert mov.history(POWER, 16) == 15 and mov.history(POWER, 1) == 0
    assert mov.history(2, 16, 4) == 0 and mov.history(LAG, 0, 4) == 0
    for w in (1, 16, 33, 1000, 4096):
        for kind in (LAG, POWER):
            g = mov.grid(kind, w)
            assert 1 <= g <= 4096 and g == w
    assert mov.grid(LAG, 0) == 0 and mov.grid(LAG, 4097) == 0 and mov.grid(5, 16) == 0


def test_freq_step_is_its_formula(lib):
    for p in (1 + 0j, 0.3 - 0.9j, -2 + 1e-3j, -1 - 1e-9j, 5j):
        for lag in (1, 16, 1024, 65536):
            want = nco.word(-math.atan2(p.imag, p.real) / (2 * math.pi * lag))
            assert mov.freq_step(p, lag) == want, (p, lag)
    rec = _lib.MovPeak(3, 3, 0.0, 1.0, 2.0, 2.0, 0.5, 0, 0)
    assert mov.freq_step(rec, 4) == nco.word(-0.25 / 4) == lib.aeth_mov_freq_step(C.byref(rec), 4)
    assert mov.freq_step(rec, 0) == 0 and mov.freq_step(0j, 16) == 0 and lib.aeth_mov_freq_step(None, 16) == 0
