"""CPU: the resampler's kernels (csrc/aeth_resamp.hip) are in the library's gfx950 code object, in both cache policies
and with and without the up == 1 flag, without spills or scratch, within the 128 VGPRs that __launch_bounds__(256, 4)
promises and within 40 KiB of static LDS: four workgroups in a CU's 160 KiB.

Registers, spills and scratch come from the `kernels` fixture of tests/test_kernel_resources.py.  The static LDS does not:
a code object's notes list .group_segment_fixed_size IN FRONT OF .name, so that fixture files it under the kernel listed
before (and drops it for the first kernel of a code object).  `lds_bytes` below reads the same notes once more and keeps
every field of one kernel's record together."""
import os
import re
import shutil
import subprocess

import pytest

from test_kernel_resources import LIB, LLVM, kernels          # noqa: F401  (the module-scoped fixture that reads the code objects)

NAMES = ("resamp_staged_kernel", "resamp_direct_kernel")


@pytest.fixture(scope="module")
def lds_bytes(kernels, tmp_path_factory):                      # noqa: F811  (after `kernels`: it skips when the tools are missing)
    """{kernel name: .group_segment_fixed_size} of the code objects that hold a resampler kernel"""
    d = tmp_path_factory.mktemp("co_resamp")
    so = shutil.copy(LIB, d / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    out = {}
    for f in sorted(os.listdir(d)):
        if "gfx950" not in f or b"resamp_" not in open(d / f, "rb").read():
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(d / f)], check=True, capture_output=True, text=True).stdout
        for rec in re.split(r"\n\s+- \.", notes):              # one list item per kernel
            name = re.search(r"\.name:\s+(\S+)", rec)
            lds = re.search(r"group_segment_fixed_size:\s+(\d+)", rec)
            if name and lds:
                out[name.group(1)] = int(lds.group(1))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_resampler_kernels_exist_within_four_workgroups_per_cu(kernels, lds_bytes, name):           # noqa: F811
    found = {k: v for k, v in kernels.items() if name in k}
    assert len(found) == 4, (name, sorted(found))
    # mangled template arguments: ILb<U1>ELb<NT>E
    have = {tuple(int(g) for g in re.search(name + r"ILb([01])ELb([01])E", k).groups()) for k in found}
    assert have == {(u1, nt) for u1 in (0, 1) for nt in (0, 1)}, sorted(have)
    for k, v in found.items():
        assert not v.get("vgpr_spill_count", 0) and not v.get("sgpr_spill_count", 0), (k, v)
        assert not v.get("private_segment_fixed_size", 0), (k, v)
        assert 0 < v["vgpr_count"] <= 128, (k, v)
        assert k in lds_bytes, (k, sorted(lds_bytes))
        assert lds_bytes[k] <= 40 * 1024, (k, lds_bytes[k])
        assert (lds_bytes[k] > 0) == (name == "resamp_staged_kernel"), (k, lds_bytes[k])      # only the staged route stages
    print({k: (v["vgpr_count"], lds_bytes[k]) for k, v in sorted(found.items())})
