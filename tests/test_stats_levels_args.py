"""CPU: aeth_vec_stats, aeth_host_vec_stats, aeth_vec_levels and aeth_fft_exec_levels validate their arguments before
any device work, as the other entry points do (tests/test_abi_symbols.py::test_errors_do_not_need_a_gpu): every bad call
returns its AETH_E_* code with a message and touches nothing.

A context cannot be created without a device, so the calls that must get past `ctx is null` receive the address of a
zeroed block as their context: validation only asks whether the pointer is null, and each of these calls is refused
before the context is looked at (a call that passed validation would go on to the device and is not made here)."""
import ctypes as C

import pytest

from aether_primitives_amd import _lib


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def fake_ctx():
    block = (C.c_char * 4096)()
    return C.cast(block, C.c_void_p), block


def _err(lib, rc, code, *words):
    assert rc == code, (rc, lib.aeth_last_error())
    msg = lib.aeth_last_error().decode()
    assert msg and all(w in msg for w in words), msg


X = C.c_void_p(0x10000)             # never dereferenced: 16-byte aligned "device" addresses
LV = C.c_void_p(0x90000)


def test_the_record_is_64_bytes_without_padding():
    from aether_primitives_amd.context import _VecStats
    assert C.sizeof(_VecStats) == 64
    assert _VecStats.power.offset == 56 and _VecStats.min_norm.offset == 32


def test_stats_arguments(lib, fake_ctx):
    ctx, _ = fake_ctx
    out = (C.c_char * 64)()
    for fn in (lib.aeth_vec_stats, lib.aeth_host_vec_stats):
        _err(lib, fn(None, X, 16, out), _lib.E_ARG, "ctx", "null")
        _err(lib, fn(ctx, None, 16, out), _lib.E_ARG, "null")
        _err(lib, fn(ctx, X, 16, None), _lib.E_ARG, "null")
        _err(lib, fn(ctx, X, 0, out), _lib.E_LEN, "empty")
    _err(lib, lib.aeth_vec_stats(ctx, C.c_void_p(0x10004), 16, out), _lib.E_ALIGN, "aligned")
    assert bytes(out) == bytes(64)                                   # nothing was written


def test_levels_arguments(lib, fake_ctx):
    ctx, _ = fake_ctx
    _err(lib, lib.aeth_vec_levels(None, X, 16, 0, LV, 16), _lib.E_ARG, "ctx", "null")
    _err(lib, lib.aeth_vec_levels(ctx, None, 16, 0, LV, 16), _lib.E_ARG, "null")
    _err(lib, lib.aeth_vec_levels(ctx, X, 16, 0, None, 16), _lib.E_ARG, "null")
    _err(lib, lib.aeth_vec_levels(ctx, X, 16, 0, LV, 15), _lib.E_LEN, "same length")
    _err(lib, lib.aeth_vec_levels(ctx, X, 16, 0, LV, 17), _lib.E_LEN, "same length")
    for kind in (-1, 3, 99):
        _err(lib, lib.aeth_vec_levels(ctx, X, 16, kind, LV, 16), _lib.E_ARG, "level kind")
    _err(lib, lib.aeth_vec_levels(ctx, C.c_void_p(0x10004), 16, 0, LV, 16), _lib.E_ALIGN, "aligned")
    _err(lib, lib.aeth_vec_levels(ctx, X, 16, 0, C.c_void_p(0x90002), 16), _lib.E_ALIGN, "aligned")
    # the output inside, at the start of, and straddling the end of the input: refused; touching ranges are fine
    for lv in (0x10000, 0x10040, 0x10000 + 16 * 8 - 4, 0x10000 - 16 * 4 + 4):
        _err(lib, lib.aeth_vec_levels(ctx, X, 16, 0, C.c_void_p(lv), 16), _lib.E_ARG, "overlap")
    # an empty vector is no error and no launch (the element-wise calls behave the same)
    assert lib.aeth_vec_levels(ctx, X, 0, 0, LV, 0) == _lib.OK
    assert lib.aeth_vec_levels(ctx, None, 0, 2, None, 0) == _lib.OK


def test_fft_levels_arguments(lib):
    _err(lib, lib.aeth_fft_exec_levels(None, X, 2048, 1, 1, 0, 0.0, 0, 0, LV, 2048), _lib.E_ARG, "plan", "null")
    with pytest.raises(_lib.AetherError):
        _lib.check(lib.aeth_fft_exec_levels(None, None, 0, 0, 1, 0, 0.0, 1, 1, None, 0))


def test_python_mirror_has_the_new_surface():
    import aether_primitives_amd as ap
    assert (ap.LEVEL_NORM, ap.LEVEL_DB, ap.LEVEL_POWER_DB) == (0, 1, 2)
    for cls, names in ((ap.DeviceVec, ("stats", "levels")), (ap.HostVec, ("stats",)), (ap.HipFft, ("levels",)),
                       (ap.DeviceF32, ("to_host", "slice"))):
        for name in names:
            assert callable(getattr(cls, name)), (cls, name)
