"""CPU: the frame-check kernels (csrc/aeth_crc.hip) are in the library's gfx950 code object -- the frames route, the long
route's chunk and store launches and both packing kernels under both cache policies, the long route's combine launch and
the summary fold once each -- without spills or scratch and within 128 VGPRs (four waves per SIMD).  The design's static
LDS budget is four fold records per workgroup: 64 bytes where a summary is folded, 32 in the combine launch, none in the
kernels that fold nothing.

Registers, spills and scratch come from the `kernels` fixture of tests/test_kernel_resources.py; the static LDS is read
from the code object's notes here, one kernel's record at a time.  Only the resource notes are read."""
import os
import re
import shutil
import subprocess

import pytest

from test_kernel_resources import LIB, LLVM, kernels          # noqa: F401  (the module-scoped fixture that reads the code objects)

LDS_RECORDS = 4 * 16


@pytest.fixture(scope="module")
def lds_bytes(kernels, tmp_path_factory):                      # noqa: F811  (after `kernels`: it skips when the tools are missing)
    """{kernel name: .group_segment_fixed_size} of the code objects that hold a frame-check kernel"""
    d = tmp_path_factory.mktemp("co_crc")
    so = shutil.copy(LIB, d / "lib.so")
    subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", so], check=True, capture_output=True, cwd=d)
    out = {}
    for f in sorted(os.listdir(d)):
        if "gfx950" not in f or b"crc_frames_kernel" not in open(d / f, "rb").read():
            continue
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", str(d / f)], check=True, capture_output=True, text=True).stdout
        for rec in re.split(r"\n\s+- \.", notes):              # one list item per kernel
            name = re.search(r"\.name:\s+(\S+)", rec)
            lds = re.search(r"group_segment_fixed_size:\s+(\d+)", rec)
            if name and lds:
                out[name.group(1)] = int(lds.group(1))
    return out


def found(kernels, lds_bytes, name, count):                    # noqa: F811
    got = {k: v for k, v in kernels.items() if name in k}
    assert len(got) == count, (name, sorted(got))
    if count == 2:
        assert {int(re.search(name + r"ILb([01])E", k).group(1)) for k in got} == {0, 1}, sorted(got)
    for k, v in got.items():
        assert not v.get("vgpr_spill_count", 0) and not v.get("sgpr_spill_count", 0), (k, v)
        assert not v.get("private_segment_fixed_size", 0), (k, v)
        assert 0 < v["vgpr_count"] <= 128, (k, v)
        assert k in lds_bytes, (k, sorted(lds_bytes))
    print({k: (v["vgpr_count"], lds_bytes[k]) for k, v in sorted(got.items())})
    return got


@pytest.mark.parametrize("name,count,lds", (("crc_frames_kernel", 2, LDS_RECORDS), ("crc_long_kernel", 2, 0), ("crc_store_kernel", 2, LDS_RECORDS),
                                            ("crc_combine_kernel", 1, 32), ("crc_summary_kernel", 1, LDS_RECORDS),
                                            ("bits_pack_kernel", 2, 0), ("bits_unpack_kernel", 2, 0)))
def test_kernel_exists_without_spills_within_its_lds_budget(kernels, lds_bytes, name, count, lds):          # noqa: F811
    for k in found(kernels, lds_bytes, name, count):
        assert lds_bytes[k] == lds, (k, lds_bytes[k])
