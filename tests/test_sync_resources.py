"""CPU: the estimators' kernels (csrc/aeth_sync.hip) are in the library's gfx950 code object in every template
combination -- the line kernel for five kinds, both cache policies, with and without the phasor; the lag kernel for four
powers and both cache policies; the fold kernel -- without spills or scratch, within 128 VGPRs (four waves per SIMD) and
4 KiB of static LDS.

Registers, spills and scratch come from the `kernels` fixture of tests/test_kernel_resources.py; the static LDS is read
from the code object's notes here, one kernel's record at a time (tests/test_resamp_resources.py says why).  Only the
resource notes are read."""
import os
import re
import shutil
import subprocess

import pytest

from test_kernel_resources import LIB, LLVM, kernels          # noqa: F401  (the module-scoped fixture that reads the code objects)

KINDS = (0, 1, 2, 4, 8)
POWERS = (1, 2, 4, 8)


@pytest.fixture(scope="module")
def lds_bytes(kernels, tmp_path_factory):                      # noqa: F811  (after `kernels`: it skips when the tools are missing)
    """{kernel name: .group_segment_fixed_size} of the code objects that hold an estimator kernel"""
    d = tmp_path_factory.mktemp("co_sync")
    so = shutil.copy(LIB, d / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    out = {}
    for f in sorted(os.listdir(d)):
        if "gfx950" not in f or b"sync_line_kernel" not in open(d / f, "rb").read():
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
        assert lds_bytes[k] <= 4096, (k, lds_bytes[k])
    print({k: (v["vgpr_count"], lds_bytes[k]) for k, v in sorted(found.items())})


def test_line_kernel_exists_in_every_combination_within_its_limits(kernels, lds_bytes):           # noqa: F811
    found = {k: v for k, v in kernels.items() if "sync_line_kernel" in k}
    # mangled template arguments: ILi<KIND>ELb<NT>ELb<ZERO>EE
    have = {tuple(int(g) for g in re.search(r"sync_line_kernelILi(\d)ELb([01])ELb([01])EE", k).groups()) for k in found}
    assert have == {(kind, nt, zero) for kind in KINDS for nt in (0, 1) for zero in (0, 1)}, sorted(have)
    assert len(found) == 20, sorted(found)
    within_limits(found, lds_bytes)


def test_lag_kernel_exists_in_every_combination_within_its_limits(kernels, lds_bytes):            # noqa: F811
    found = {k: v for k, v in kernels.items() if "sync_lag_kernel" in k}
    have = {tuple(int(g) for g in re.search(r"sync_lag_kernelILi(\d)ELb([01])EE", k).groups()) for k in found}
    assert have == {(m, nt) for m in POWERS for nt in (0, 1)}, sorted(have)
    assert len(found) == 8, sorted(found)
    within_limits(found, lds_bytes)


def test_fold_kernel_is_within_its_limits(kernels, lds_bytes):                                    # noqa: F811
    found = {k: v for k, v in kernels.items() if "sync_fold_kernel" in k}
    assert len(found) == 1, sorted(found)
    within_limits(found, lds_bytes)
