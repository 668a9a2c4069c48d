"""CPU: the turbo kernels (csrc/aeth_turbo.hip) are in the library's gfx950 code object -- the encoder once, the decoder
once per built S = 4, 8, 16 states -- without spills or scratch.  As built the decoders take 65, 78 and 110 VGPRs and the
encoder 13.  A decoder workgroup may have 1024 lanes (one per window), four waves on each SIMD, so the step of the
occupancy table that every decoder must stay within is 128 registers; S = 4 and 8 would also fit the 96-register step
(five waves per SIMD), which the LDS of a large frame does not let them reach anyway.  All of a kernel's LDS is dynamic
(aeth_turbo_lds_bytes): the static size is 0.  For the LTE code at K = 6144 with windows of 32 steps a workgroup is one
codeword on 192 lanes and 49180 bytes, so three workgroups, nine waves, share a CU of 160 KiB.

Registers, spills and scratch come from the `kernels` fixture of tests/test_kernel_resources.py; the static LDS is read
from the code object's notes here, one kernel's record at a time.  Only the resource notes are read."""
import os
import re
import shutil
import subprocess

import pytest

from test_kernel_resources import LIB, LLVM, kernels          # noqa: F401  (the module-scoped fixture that reads the code objects)

VGPR_BOUND = 128
LDS_PER_CU = 160 * 1024
DECODERS = ("turbo_decode_kernelILi4E", "turbo_decode_kernelILi8E", "turbo_decode_kernelILi16E")


@pytest.fixture(scope="module")
def lds_bytes(kernels, tmp_path_factory):                      # noqa: F811  (after `kernels`: it skips when the tools are missing)
    """{kernel name: .group_segment_fixed_size} of the code objects that hold a turbo kernel"""
    d = tmp_path_factory.mktemp("co_turbo")
    so = shutil.copy(LIB, d / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    out = {}
    for f in sorted(os.listdir(d)):
        if "gfx950" not in f or b"turbo_decode_kernel" not in open(d / f, "rb").read():
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(d / f)], check=True, capture_output=True, text=True).stdout
        for rec in re.split(r"\n\s+- \.", notes):              # one list item per kernel
            name = re.search(r"\.name:\s+(\S+)", rec)
            lds = re.search(r"group_segment_fixed_size:\s+(\d+)", rec)
            if name and lds:
                out[name.group(1)] = int(lds.group(1))
    return out


@pytest.mark.parametrize("name", ("turbo_encode_kernel",) + DECODERS)
def test_kernel_exists_without_spills_and_static_lds(kernels, lds_bytes, name):          # noqa: F811
    got = {k: v for k, v in kernels.items() if name in k}
    assert len(got) == 1, (name, sorted(got))
    for k, v in got.items():
        assert not v.get("vgpr_spill_count", 0) and not v.get("sgpr_spill_count", 0), (k, v)
        assert not v.get("private_segment_fixed_size", 0), (k, v)
        assert 0 < v["vgpr_count"] <= VGPR_BOUND, (k, v)
        assert k in lds_bytes, (k, sorted(lds_bytes))
        assert lds_bytes[k] == 0, (k, lds_bytes[k])
        print(k, v["vgpr_count"], v.get("sgpr_count"), lds_bytes[k])


def test_no_other_build_is_in_the_library(kernels):          # noqa: F811
    assert len([k for k in kernels if "turbo_decode_kernel" in k]) == 3
    assert len([k for k in kernels if "turbo_encode_kernel" in k]) == 1


def lds_of(K, nu, W):
    """aeth_turbo_group and aeth_turbo_lds_bytes as aeth_turbo_core.h computes them"""
    pad4 = lambda v: (v + 3) & ~3                             # noqa: E731
    per = pad4(3 * K + 4 * nu) + pad4(K) + pad4(4 * K)        # the frame as it came, interleaved systematics, a1 and a2 as int16
    windows = (K - 1) // W + 1
    G = max(1, min(256 // windows, (48 * 1024) // per, 64))
    return windows, G, G * per + 8 * G + 8


@pytest.mark.parametrize("K,nu,W,windows,G,lds,per_cu", ((6144, 3, 32, 192, 1, 49180, 3), (512, 3, 32, 16, 11, 45284, 3), (40, 3, 40, 1, 64, 21768, 7),
                                                         (8192, 4, 8, 1024, 1, 65568, 2)))
def test_workgroups_per_cu_the_lds_allows(K, nu, W, windows, G, lds, per_cu):
    assert lds_of(K, nu, W) == (windows, G, lds)
    assert G * windows <= 1024 and lds <= LDS_PER_CU
    assert LDS_PER_CU // lds == per_cu


def test_lds_bytes_through_the_library_for_6144_by_32():
    """the getter's arithmetic on an object that is never followed past its own fields"""
    import ctypes as C
    from aether_primitives_amd import _lib
    from test_turbo_args import FakeTurbo
    lib = _lib.load()
    obj = FakeTurbo(0, 6144, 3 * 6144 + 12, 4, 8, 32, 32, 192, 1, 49164, 1, 32 * 8 * 192, (C.c_uint32 * 3)(4, 0o13, 0o15))
    assert lib.aeth_turbo_lds_bytes(C.byref(obj)) == 49180 and LDS_PER_CU // 49180 == 3
    assert lib.aeth_turbo_group(C.byref(obj)) * lib.aeth_turbo_windows(C.byref(obj)) == 192       # three waves
