"""CPU: the moving-window kernels (csrc/aeth_mov.hip) are in the library's gfx950 code object in every template
combination -- the lag kind with each of the seven plane sets and the search, the power kind with the three plane sets
without p and the search, each under both cache policies; the fold kernel -- without spills or scratch, within 128 VGPRs
(four waves per SIMD, as for the estimators) and 80 KiB of LDS (static; the kernels ask for no dynamic LDS), so that two
workgroups fit in a CU's 160 KiB.

Registers, spills and scratch come from the `kernels` fixture of tests/test_kernel_resources.py; the static LDS is read
from the code object's notes here, one kernel's record at a time.  Only the resource notes are read."""
import os
import re
import shutil
import subprocess

import pytest

from test_kernel_resources import LIB, LLVM, kernels          # noqa: F401  (the module-scoped fixture that reads the code objects)

LAG, POWER = 0, 1
OUTS = {LAG: (1, 2, 3, 4, 5, 6, 7, 8), POWER: (2, 4, 6, 8)}    # bit 0: p, bit 1: r, bit 2: m; 8: the search
LDS_LIMIT = 80 * 1024


@pytest.fixture(scope="module")
def lds_bytes(kernels, tmp_path_factory):                      # noqa: F811  (after `kernels`: it skips when the tools are missing)
    """{kernel name: .group_segment_fixed_size} of the code objects that hold a moving-window kernel"""
    d = tmp_path_factory.mktemp("co_mov")
    so = shutil.copy(LIB, d / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    out = {}
    for f in sorted(os.listdir(d)):
        if "gfx950" not in f or b"mov_kernel" not in open(d / f, "rb").read():
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(d / f)], check=True, capture_output=True, text=True).stdout
        for rec in re.split(r"\n\s+- \.", notes):              # one list item per kernel
            name = re.search(r"\.name:\s+(\S+)", rec)
            lds = re.search(r"group_segment_fixed_size:\s+(\d+)", rec)
            if name and lds:
                out[name.group(1)] = int(lds.group(1))
    return out


def within_limits(found, lds_bytes):
    for k, v in found.items():
        assert not v.get("vgpr_spill_count", 0) and not v.get("sgpr_spill_count", 0), (k, v)
        assert not v.get("private_segment_fixed_size", 0), (k, v)
        assert 0 < v["vgpr_count"] <= 128, (k, v)
        assert k in lds_bytes, (k, sorted(lds_bytes))
        assert lds_bytes[k] <= LDS_LIMIT, (k, lds_bytes[k])
    print({k: (v["vgpr_count"], lds_bytes[k]) for k, v in sorted(found.items())})


def test_window_kernel_exists_in_every_combination_within_its_limits(kernels, lds_bytes):          # noqa: F811
    found = {k: v for k, v in kernels.items() if "mov_kernel" in k}
    # mangled template arguments: ILi<KIND>ELb<NT>ELi<OUT>EE
    have = {tuple(int(g) for g in re.search(r"mov_kernelILi(\d)ELb([01])ELi(\d)EE", k).groups()) for k in found}
    assert have == {(kind, nt, out) for kind in (LAG, POWER) for nt in (0, 1) for out in OUTS[kind]}, sorted(have)
    assert len(found) == 24, sorted(found)
    within_limits(found, lds_bytes)


def test_fold_kernel_is_within_its_limits(kernels, lds_bytes):                                     # noqa: F811
    found = {k: v for k, v in kernels.items() if "mov_fold_kernel" in k}
    assert len(found) == 1, sorted(found)
    within_limits(found, lds_bytes)
