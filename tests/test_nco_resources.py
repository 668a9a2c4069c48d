"""CPU: the oscillator's kernels (csrc/aeth_nco.hip) are in the library's gfx950 code object in every template
combination -- 16- and 8-byte lanes, both cache policies, with and without the chirp term -- without spills, scratch or
LDS and within 64 VGPRs.

Registers, spills and scratch come from the `kernels` fixture of tests/test_kernel_resources.py; the static LDS is read
from the code object's notes here, one kernel's record at a time (tests/test_resamp_resources.py says why)."""
import os
import re
import shutil
import subprocess

import pytest

from test_kernel_resources import LIB, LLVM, kernels          # noqa: F401  (the module-scoped fixture that reads the code objects)

NAMES = ("nco_mix_kernel", "nco_tone_kernel")


@pytest.fixture(scope="module")
def lds_bytes(kernels, tmp_path_factory):                      # noqa: F811  (after `kernels`: it skips when the tools are missing)
    """{kernel name: .group_segment_fixed_size} of the code objects that hold an oscillator kernel"""
    d = tmp_path_factory.mktemp("co_nco")
    so = shutil.copy(LIB, d / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    out = {}
    for f in sorted(os.listdir(d)):
        if "gfx950" not in f or b"nco_mix_kernel" not in open(d / f, "rb").read():
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(d / f)], check=True, capture_output=True, text=True).stdout
        for rec in re.split(r"\n\s+- \.", notes):              # one list item per kernel
            name = re.search(r"\.name:\s+(\S+)", rec)
            lds = re.search(r"group_segment_fixed_size:\s+(\d+)", rec)
            if name and lds:
                out[name.group(1)] = int(lds.group(1))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_oscillator_kernels_exist_in_every_combination_within_their_limits(kernels, lds_bytes, name):           # noqa: F811
    found = {k: v for k, v in kernels.items() if name in k}
    assert len(found) == 8, (name, sorted(found))
    # mangled template arguments: I15HIP_vector_typeIfLj<lanes>EELb<NT>ELb<RATE>E
    have = {tuple(int(g) for g in re.search(name + r"I15HIP_vector_typeIfLj([24])EELb([01])ELb([01])E", k).groups()) for k in found}
    assert have == {(v, nt, rate) for v in (2, 4) for nt in (0, 1) for rate in (0, 1)}, sorted(have)
    for k, v in found.items():
        assert not v.get("vgpr_spill_count", 0) and not v.get("sgpr_spill_count", 0), (k, v)
        assert not v.get("private_segment_fixed_size", 0), (k, v)
        assert 0 < v["vgpr_count"] <= 64, (k, v)
        assert k in lds_bytes, (k, sorted(lds_bytes))
        assert lds_bytes[k] == 0, (k, lds_bytes[k])
    print({k: v["vgpr_count"] for k, v in sorted(found.items())})
