"""CPU: the rate-matching kernels (csrc/aeth_remap.hip) are in the library's gfx950 code object on both routes under both
cache policies, without spills or scratch and within 128 VGPRs (four waves per SIMD: the tile launch asks for four
workgroups per CU); the tile kernel's static LDS is the 32 KiB budget the route is chosen by (five workgroups share a CU's
160 KiB), the gather kernel uses none.

Registers, spills and scratch come from the `kernels` fixture of tests/test_kernel_resources.py; the static LDS is read
from the code object's notes here, one kernel's record at a time (the notes list .group_segment_fixed_size in front of
.name, so that fixture files it under the kernel listed before).  Only the resource notes are read."""
import os
import re
import shutil
import subprocess

import pytest

from test_kernel_resources import LIB, LLVM, kernels          # noqa: F401  (the module-scoped fixture that reads the code objects)

LDS_BUDGET = 32768


@pytest.fixture(scope="module")
def lds_bytes(kernels, tmp_path_factory):                      # noqa: F811  (after `kernels`: it skips when the tools are missing)
    """{kernel name: .group_segment_fixed_size} of the code objects that hold a rate-matching kernel"""
    d = tmp_path_factory.mktemp("co_remap")
    so = shutil.copy(LIB, d / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    out = {}
    for f in sorted(os.listdir(d)):
        if "gfx950" not in f or b"remap_tile_kernel" not in open(d / f, "rb").read():
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(d / f)], check=True, capture_output=True, text=True).stdout
        for rec in re.split(r"\n\s+- \.", notes):              # one list item per kernel
            name = re.search(r"\.name:\s+(\S+)", rec)
            lds = re.search(r"group_segment_fixed_size:\s+(\d+)", rec)
            if name and lds:
                out[name.group(1)] = int(lds.group(1))
    return out


def variants(kernels, lds_bytes, name):                        # noqa: F811
    found = {k: v for k, v in kernels.items() if name in k}
    have = {int(re.search(name + r"ILb([01])E", k).group(1)) for k in found}
    assert len(found) == 2 and have == {0, 1}, sorted(found)
    for k, v in found.items():
        assert not v.get("vgpr_spill_count", 0) and not v.get("sgpr_spill_count", 0), (k, v)
        assert not v.get("private_segment_fixed_size", 0), (k, v)
        assert 0 < v["vgpr_count"] <= 128, (k, v)
        assert k in lds_bytes, (k, sorted(lds_bytes))
    print({k: (v["vgpr_count"], lds_bytes[k]) for k, v in sorted(found.items())})
    return found


def test_tile_route_exists_under_both_cache_policies_within_the_lds_budget(kernels, lds_bytes):       # noqa: F811
    for k in variants(kernels, lds_bytes, "remap_tile_kernel"):
        assert 0 < lds_bytes[k] <= LDS_BUDGET, (k, lds_bytes[k])


def test_gather_route_exists_under_both_cache_policies_without_lds(kernels, lds_bytes):               # noqa: F811
    for k in variants(kernels, lds_bytes, "remap_gather_kernel"):
        assert lds_bytes[k] == 0, (k, lds_bytes[k])
