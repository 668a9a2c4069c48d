"""CPU: the polar kernels (csrc/aeth_polar.hip) are in the library's gfx950 code object -- the encoder once, the decoder
once per built T = 4, 8, 16 lanes per codeword -- without spills or scratch.  As built the decoders take 55, 56 and 64
VGPRs and the encoder 20: all within the 64-register step of the occupancy table, eight waves per SIMD as far as
registers go.  What the LDS allows is less and is the design's trade: a decoder workgroup is one wave on
aeth_polar_lds_bytes of dynamic LDS -- at n = 10, 36992 bytes with T = 4 (four waves per CU of 160 KiB, one per SIMD),
18560 with T = 8 (eight, two per SIMD) and 9344 with T = 16 (seventeen, four per SIMD).  All of a kernel's LDS is dynamic:
the static size is 0 for the decoders, and the encoder uses none.

Registers, spills and scratch come from the `kernels` fixture of tests/test_kernel_resources.py; the static LDS is read
from the code object's notes here, one kernel's record at a time.  Only the resource notes are read."""
import os
import re
import shutil
import subprocess

import pytest

from test_kernel_resources import LIB, LLVM, kernels          # noqa: F401  (the module-scoped fixture that reads the code objects)

VGPR_BOUND = 64
LDS_PER_CU = 160 * 1024


@pytest.fixture(scope="module")
def lds_bytes(kernels, tmp_path_factory):                      # noqa: F811  (after `kernels`: it skips when the tools are missing)
    """{kernel name: .group_segment_fixed_size} of the code objects that hold a polar kernel"""
    d = tmp_path_factory.mktemp("co_polar")
    so = shutil.copy(LIB, d / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    out = {}
    for f in sorted(os.listdir(d)):
        if "gfx950" not in f or b"polar_decode_kernel" not in open(d / f, "rb").read():
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(d / f)], check=True, capture_output=True, text=True).stdout
        for rec in re.split(r"\n\s+- \.", notes):              # one list item per kernel
            name = re.search(r"\.name:\s+(\S+)", rec)
            lds = re.search(r"group_segment_fixed_size:\s+(\d+)", rec)
            if name and lds:
                out[name.group(1)] = int(lds.group(1))
    return out


@pytest.mark.parametrize("name", ("polar_encode_kernel", "polar_decode_kernelILi4E", "polar_decode_kernelILi8E", "polar_decode_kernelILi16E"))
def test_kernel_exists_without_spills_and_static_lds(kernels, lds_bytes, name):          # noqa: F811
    got = {k: v for k, v in kernels.items() if name in k}
    assert len(got) == 1, (name, sorted(got))
    for k, v in got.items():
        assert not v.get("vgpr_spill_count", 0) and not v.get("sgpr_spill_count", 0), (k, v)
        assert not v.get("private_segment_fixed_size", 0), (k, v)
        assert 0 < v["vgpr_count"] <= VGPR_BOUND, (k, v)
        assert k in lds_bytes, (k, sorted(lds_bytes))
        assert lds_bytes[k] == 0, (k, lds_bytes[k])
        print(k, v["vgpr_count"], lds_bytes[k])


def test_no_other_decoder_build_is_in_the_library(kernels):   # noqa: F811
    assert len([k for k in kernels if "polar_decode_kernel" in k]) == 3
    assert len([k for k in kernels if "polar_encode_kernel" in k]) == 1


@pytest.mark.parametrize("T,lds,waves", ((4, 36992, 4), (8, 18560, 8), (16, 9344, 17)))
def test_waves_per_cu_the_lds_allows_at_n_10(T, lds, waves):
    """the decoder's state per codeword at n = 10: levels of 2 T .. N / 2 int16 values, two packed bit arrays of N bits,
    padded to 2 T modulo 128 bytes; 64 / T codewords per wave"""
    N = 1024
    raw = 2 * (N - 2 * T) + 2 * (N // 8)
    stride = raw + (2 * T - raw) % 128
    assert stride % 128 == 2 * T and (64 // T) * stride == lds
    assert min(LDS_PER_CU // lds, 32) == waves
