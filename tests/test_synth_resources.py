"""CPU: the overlap-add kernels of the synthesis bank (csrc/aeth_synth.hip) are in the library's gfx950 code object, in
both cache policies, without spills or scratch and within 128 VGPRs: the budget of the analysis bank
(tests/test_chan_resources.py), four waves per SIMD."""
import re

import pytest

from test_kernel_resources import kernels          # noqa: F401  (the module-scoped fixture that reads the code objects)

NAMES = ("synth_ring_kernel", "synth_gen_kernel")


@pytest.mark.parametrize("name", NAMES)
def test_unfold_kernels_exist_within_four_waves_per_simd(kernels, name):           # noqa: F811
    found = {k: v for k, v in kernels.items() if name in k}
    # the general kernel: plain and non-temporal accesses; the ring kernel: that times K = 2 .. 8 and one or two offsets
    assert len(found) == (2 if name == "synth_gen_kernel" else 28), (name, sorted(found))
    for k, v in found.items():
        assert not v.get("vgpr_spill_count", 0) and not v.get("sgpr_spill_count", 0), (k, v)
        assert not v.get("private_segment_fixed_size", 0), (k, v)
        assert 0 < v["vgpr_count"] <= 128, (k, v)
    print({k: v["vgpr_count"] for k, v in sorted(found.items())})


def test_the_ring_is_built_for_every_depth_width_and_cache_policy(kernels):     # noqa: F811
    """mangled template arguments: ILi<K>ELi<CW>ELb<NT>E"""
    have = set()
    for k in kernels:
        m = re.search(r"synth_ring_kernelILi(\d+)ELi(\d+)ELb([01])E", k)
        if m:
            have.add(tuple(int(g) for g in m.groups()))
    assert have == {(K, cw, nt) for K in range(2, 9) for cw in (1, 2) for nt in (0, 1)}, sorted(have)
    gen = {re.search(r"synth_gen_kernelILb([01])E", k).group(1) for k in kernels if "synth_gen_kernel" in k}
    assert gen == {"0", "1"}
