"""CPU: the arbitrary-ratio resampler's kernels (csrc/aeth_arb.hip) are in the library's gfx950 code object, on both
routes, with the tap table in memory and in LDS, and in both cache policies, without spills or scratch, within the 128 VGPRs that __launch_bounds__(256, 4)
promises and within 40 KiB of static LDS: four workgroups in a CU's 160 KiB.

Registers, spills and scratch come from the `kernels` fixture of tests/test_kernel_resources.py; the static LDS is read
from the code object's notes as tests/test_resamp_resources.py reads it (one record per kernel, every field of the record
kept together)."""
import os
import re
import shutil
import subprocess

import pytest

from test_kernel_resources import LIB, LLVM, kernels          # noqa: F401  (the module-scoped fixture that reads the code objects)

NAMES = ("arb_staged_kernel", "arb_direct_kernel")


@pytest.fixture(scope="module")
def lds_bytes(kernels, tmp_path_factory):                      # noqa: F811  (after `kernels`: it skips when the tools are missing)
    """{kernel name: .group_segment_fixed_size} of the code objects that hold one of these kernels"""
    d = tmp_path_factory.mktemp("co_arb")
    so = shutil.copy(LIB, d / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    out = {}
    for f in sorted(os.listdir(d)):
        if "gfx950" not in f or b"arb_staged_kernel" not in open(d / f, "rb").read():
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(d / f)], check=True, capture_output=True, text=True).stdout
        for rec in re.split(r"\n\s+- \.", notes):              # one list item per kernel
            name = re.search(r"\.name:\s+(\S+)", rec)
            lds = re.search(r"group_segment_fixed_size:\s+(\d+)", rec)
            if name and lds:
                out[name.group(1)] = int(lds.group(1))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_arb_kernels_exist_within_four_workgroups_per_cu(kernels, lds_bytes, name):           # noqa: F811
    found = {k: v for k, v in kernels.items() if name in k}
    staged = name == "arb_staged_kernel"
    assert len(found) == (4 if staged else 2), (name, sorted(found))
    # mangled template arguments: ILb<NT>ELb<TAB>E on the staged route, ILb<NT>E on the direct one
    have = {tuple(int(g) for g in re.search(name + (r"ILb([01])ELb([01])E" if staged else r"ILb([01])E"), k).groups()) for k in found}
    assert have == ({(nt, tab) for nt in (0, 1) for tab in (0, 1)} if staged else {(0,), (1,)}), sorted(have)
    for k, v in found.items():
        assert not v.get("vgpr_spill_count", 0) and not v.get("sgpr_spill_count", 0), (k, v)
        assert not v.get("private_segment_fixed_size", 0), (k, v)
        assert 0 < v["vgpr_count"] <= 128, (k, v)
        assert k in lds_bytes, (k, sorted(lds_bytes))
        assert lds_bytes[k] <= 40 * 1024, (k, lds_bytes[k])
        assert (lds_bytes[k] > 0) == staged, (k, lds_bytes[k])                                # only the staged route stages
    print({k: (v["vgpr_count"], lds_bytes[k]) for k, v in sorted(found.items())})
