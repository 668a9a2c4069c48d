"""CPU: the averaged-spectra entry points refuse null handles, null contexts and bad arguments with the status
include/aether_hip.h names, before any device work (tests/test_chan_args.py does the same for the filter bank)."""
import ctypes as C

import pytest

from aether_primitives_amd import _lib

NEW = ("aeth_vec_frame_sums", "aeth_chan_exec_sums", "aeth_chan_sums_chunk", "aeth_chan_sums_fused", "aeth_vec_sum_levels")
A = C.c_void_p(0x100000)             # never dereferenced: 16-byte aligned "device" addresses, 1 MiB apart
B = C.c_void_p(0x200000)
D = C.c_void_p(0x300000)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


@pytest.fixture(scope="module")
def fake_ctx():
    """memory that stands in for a context: every refusal below comes before the context is looked at"""
    buf = (C.c_char * 4096)()
    return C.c_void_p(C.addressof(buf)), buf


def err(lib, rc, code, *words):
    msg = lib.aeth_last_error().decode()
    assert rc == code, (rc, msg)
    assert all(w in msg for w in words), msg


def test_the_ctypes_table_covers_the_entries(lib):
    for name in NEW:
        assert name in _lib.PROTOTYPES and hasattr(lib, name), name


def test_null_handles_and_null_contexts(lib):
    err(lib, lib.aeth_vec_frame_sums(None, A, 64, 8, 0, 4, B, D, 8), _lib.E_ARG, "ctx", "null")
    err(lib, lib.aeth_chan_exec_sums(None, None, A, 64, 0, 1, 0, 0.0, 0, 0, 0, B, D, 8), _lib.E_ARG, "chan", "null")
    err(lib, lib.aeth_vec_sum_levels(None, A, 8, 1.0, 0, B), _lib.E_ARG, "ctx", "null")
    assert lib.aeth_chan_sums_chunk(None) == 0 and lib.aeth_chan_sums_fused(None) == 0


def test_frame_sums_refusals_in_order(lib, fake_ctx):
    ctx = fake_ctx[0]

    def call(frames=A, n=64, length=8, block=0, chunk=4, s=B, m=D, n_out=8):
        return lib.aeth_vec_frame_sums(ctx, frames, n, length, block, chunk, s, m, n_out)

    err(lib, call(frames=None), _lib.E_ARG, "frames", "null")
    err(lib, call(s=None, m=None), _lib.E_ARG, "both output planes are null")
    err(lib, call(n=0), _lib.E_LEN, "0 samples")
    err(lib, call(length=0), _lib.E_LEN, "frames of 0")
    err(lib, call(n=65), _lib.E_LEN, "65 samples", "frame length 8")
    err(lib, call(chunk=0), _lib.E_LEN, "chunk of 0")
    err(lib, call(n_out=9), _lib.E_LEN, "hold 9", "1 rows x 8")
    err(lib, call(block=3, n_out=16), _lib.E_LEN, "hold 16", "3 rows x 8")          # 8 frames in rows of 3
    err(lib, call(frames=C.c_void_p(0x100004)), _lib.E_ALIGN, "0x100004")
    err(lib, call(s=C.c_void_p(0x200004)), _lib.E_ALIGN, "0x200004")
    err(lib, call(m=C.c_void_p(0x300002)), _lib.E_ALIGN, "0x300002")
    err(lib, call(s=C.c_void_p(0x100000 + 64 * 8 - 8)), _lib.E_ARG, "overlaps the input")
    err(lib, call(m=C.c_void_p(0x100000 - 8)), _lib.E_ARG, "overlaps the input")
    err(lib, call(m=C.c_void_p(0x200000 + 56)), _lib.E_ARG, "overlaps max_dev")
    # null before lengths, lengths before alignment, alignment before overlap
    err(lib, call(frames=None, n=0), _lib.E_ARG, "null")
    err(lib, call(n=65, frames=C.c_void_p(0x100004)), _lib.E_LEN, "65 samples")
    err(lib, call(frames=C.c_void_p(0x200004)), _lib.E_ALIGN, "0x200004")


def test_sum_levels_refusals(lib, fake_ctx):
    ctx = fake_ctx[0]
    err(lib, lib.aeth_vec_sum_levels(ctx, A, 8, 1.0, 3, B), _lib.E_ARG, "level kind 3")
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        err(lib, lib.aeth_vec_sum_levels(ctx, A, 8, bad, 0, B), _lib.E_ARG, "count")
    assert lib.aeth_vec_sum_levels(ctx, None, 0, 1.0, 0, None) == _lib.OK           # nothing to do
    err(lib, lib.aeth_vec_sum_levels(ctx, None, 8, 1.0, 0, B), _lib.E_ARG, "null")
    err(lib, lib.aeth_vec_sum_levels(ctx, A, 8, 1.0, 0, None), _lib.E_ARG, "null")
    err(lib, lib.aeth_vec_sum_levels(ctx, C.c_void_p(0x100004), 8, 1.0, 0, B), _lib.E_ALIGN, "0x100004")
    err(lib, lib.aeth_vec_sum_levels(ctx, A, 8, 1.0, 0, C.c_void_p(0x200002)), _lib.E_ALIGN, "0x200002")
    err(lib, lib.aeth_vec_sum_levels(ctx, A, 8, 1.0, 0, C.c_void_p(0x100000 + 60)), _lib.E_ARG, "overlaps")


def test_python_mirror_has_the_new_surface():
    import aether_primitives_amd as ap
    for name in ("sums", "sums_chunk", "sums_fused"):
        assert hasattr(ap.Channelizer, name), name
    assert hasattr(ap.Context, "frame_sums") and hasattr(ap.Context, "sum_levels") and ap.DeviceF64 is not None
