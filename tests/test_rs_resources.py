"""CPU: the Reed-Solomon kernels (csrc/aeth_rs.hip) are in the library's gfx950 code object, once each, without spills or
scratch and within 64 VGPRs (eight waves per SIMD as far as registers go).  The design's static LDS budget: the decoder
keeps the antilog table twice over (512 bytes), the log table (256) and the four records of the summary's workgroup fold
(64) beside the dynamic arrays that aeth_rs_lds_bytes reports; the summary kernel keeps the four records; the encoder
works in registers only.

Registers, spills and scratch come from the `kernels` fixture of tests/test_kernel_resources.py; the static LDS is read
from the code object's notes here, one kernel's record at a time.  Only the resource notes are read."""
import os
import re
import shutil
import subprocess

import pytest

from test_kernel_resources import LIB, LLVM, kernels          # noqa: F401  (the module-scoped fixture that reads the code objects)

VGPR_BOUND = 64


@pytest.fixture(scope="module")
def lds_bytes(kernels, tmp_path_factory):                      # noqa: F811  (after `kernels`: it skips when the tools are missing)
    """{kernel name: .group_segment_fixed_size} of the code objects that hold an RS kernel"""
    d = tmp_path_factory.mktemp("co_rs")
    so = shutil.copy(LIB, d / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    out = {}
    for f in sorted(os.listdir(d)):
        if "gfx950" not in f or b"rs_decode_kernel" not in open(d / f, "rb").read():
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(d / f)], check=True, capture_output=True, text=True).stdout
        for rec in re.split(r"\n\s+- \.", notes):              # one list item per kernel
            name = re.search(r"\.name:\s+(\S+)", rec)
            lds = re.search(r"group_segment_fixed_size:\s+(\d+)", rec)
            if name and lds:
                out[name.group(1)] = int(lds.group(1))
    return out


@pytest.mark.parametrize("name,lds", (("rs_decode_kernel", 512 + 256 + 64), ("rs_encode_kernel", 0), ("rs_summary_kernel", 64)))
def test_kernel_exists_without_spills_within_its_lds_budget(kernels, lds_bytes, name, lds):          # noqa: F811
    got = {k: v for k, v in kernels.items() if name in k}
    assert len(got) == 1, (name, sorted(got))
    for k, v in got.items():
        assert not v.get("vgpr_spill_count", 0) and not v.get("sgpr_spill_count", 0), (k, v)
        assert not v.get("private_segment_fixed_size", 0), (k, v)
        assert 0 < v["vgpr_count"] <= VGPR_BOUND, (k, v)
        assert k in lds_bytes, (k, sorted(lds_bytes))
        assert lds_bytes[k] == lds, (k, lds_bytes[k])
        print(k, v["vgpr_count"], lds_bytes[k])
