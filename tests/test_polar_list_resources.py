"""CPU: the list decoder's kernels (csrc/aeth_polar.hip) are in the library's gfx950 code object -- polar_list_kernel once
per built (T lanes per path, L paths): T = 4, 8, 16 x L = 1, 2, 4, 8 with T L <= 64, eleven in all, and the pick once --
without spills or scratch, and all of a list kernel's LDS is dynamic (static size 0).

What the LDS allows at n = 10, a workgroup being one wave on 64 / T path states of aeth_polar_list_lds_bytes in all: with
T = 16 (L = 1, 2, 4) 8848 bytes, 18 waves per CU of 160 KiB, so up to five per SIMD, which needs at most 512 / 5 -> 96
VGPRs; with T = 8 (L = 8) 17568 bytes, 9 waves per CU, three per SIMD, 512 / 3 -> 168 VGPRs.  As built the kernels take 36
to 73 VGPRs (T = 16: 40, 58, 55 for L = 1, 2, 4; T = 8, L = 8: 67; the largest, 73, is T = 4, L = 8, which only n = 3
reaches), so registers never bind before the LDS does; every instance is held to the 96 of the tighter step.  The counts
are printed.

Registers, spills and scratch come from the `kernels` fixture of tests/test_kernel_resources.py; the static LDS is read
from the code object's notes here.  Only the resource notes are read."""
import os
import re
import shutil
import subprocess

import pytest

from test_kernel_resources import LIB, LLVM, kernels          # noqa: F401  (the module-scoped fixture that reads the code objects)

BUILT = tuple((T, L) for T in (4, 8, 16) for L in (1, 2, 4, 8) if T * L <= 64)
LDS_PER_CU = 160 * 1024
VGPR_BOUND = 96


def lanes_of(n, L):
    T = 16
    while T > 4 and (T * L > 64 or 2 * T > (1 << n)):
        T //= 2
    return T


def lds_of(n, L):
    """aeth_polar_list_lds_bytes: per path the levels of 2 T .. N / 2 int16 values and N packed bits, padded to 2 T modulo
    128, and one survivor word; 64 / T paths per wave"""
    T, N = lanes_of(n, L), 1 << n
    raw = 2 * (N - 2 * T) + 4 * max(N // 32, 1)
    stride = raw + (2 * T - raw) % 128
    assert stride % 128 == 2 * T
    return (64 // T) * (stride + 4)


@pytest.fixture(scope="module")
def lds_bytes(kernels, tmp_path_factory):                      # noqa: F811  (after `kernels`: it skips when the tools are missing)
    """{kernel name: .group_segment_fixed_size} of the code objects that hold a list kernel"""
    d = tmp_path_factory.mktemp("co_polar_list")
    so = shutil.copy(LIB, d / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    out = {}
    for f in sorted(os.listdir(d)):
        if "gfx950" not in f or b"polar_list_kernel" not in open(d / f, "rb").read():
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(d / f)], check=True, capture_output=True, text=True).stdout
        for rec in re.split(r"\n\s+- \.", notes):              # one list item per kernel
            name = re.search(r"\.name:\s+(\S+)", rec)
            lds = re.search(r"group_segment_fixed_size:\s+(\d+)", rec)
            if name and lds:
                out[name.group(1)] = int(lds.group(1))
    return out


@pytest.mark.parametrize("T,L", BUILT)
def test_instance_exists_without_spills_and_static_lds(kernels, lds_bytes, T, L):          # noqa: F811
    name = f"polar_list_kernelILi{T}ELi{L}EE"
    got = {k: v for k, v in kernels.items() if name in k}
    assert len(got) == 1, (name, sorted(got))
    for k, v in got.items():
        assert not v.get("vgpr_spill_count", 0) and not v.get("sgpr_spill_count", 0), (k, v)
        assert not v.get("private_segment_fixed_size", 0), (k, v)
        print(k, "VGPRs", v["vgpr_count"], "static LDS", lds_bytes.get(k))
        assert 0 < v["vgpr_count"] <= VGPR_BOUND, (k, v)
        assert lds_bytes[k] == 0, (k, lds_bytes[k])


def test_no_other_list_build_and_one_pick_are_in_the_library(kernels):   # noqa: F811
    assert len([k for k in kernels if "polar_list_kernel" in k]) == len(BUILT) == 11
    pick = {k: v for k, v in kernels.items() if "polar_pick_kernel" in k}
    assert len(pick) == 1
    for v in pick.values():
        assert not v.get("vgpr_spill_count", 0) and not v.get("private_segment_fixed_size", 0) and v["vgpr_count"] <= 64


@pytest.mark.parametrize("L,T,lds,per_simd,step", ((1, 16, 8848, 5, 96), (2, 16, 8848, 5, 96), (4, 16, 8848, 5, 96), (8, 8, 17568, 3, 168)))
def test_the_register_step_the_lds_needs_at_n_10(kernels, L, T, lds, per_simd, step):          # noqa: F811
    assert lanes_of(10, L) == T and lds_of(10, L) == lds <= 65536
    waves = min(LDS_PER_CU // lds, 32)
    assert -(-waves // 4) == per_simd and 512 // per_simd // 8 * 8 == step
    (v,) = [v for k, v in kernels.items() if f"polar_list_kernelILi{T}ELi{L}EE" in k]
    assert v["vgpr_count"] <= step, (T, L, v["vgpr_count"], step)


@pytest.mark.parametrize("n", range(3, 11))
def test_a_workgroup_stays_within_64_kib(n):
    for L in (1, 2, 4, 8):
        assert (lanes_of(n, L), L) in BUILT and lds_of(n, L) <= 65536
