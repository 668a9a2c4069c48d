"""CPU: the fold kernels of the filter bank (csrc/aeth_chan.hip) are in the library's gfx950 code object, in both cache
policies, without spills or scratch and within 128 VGPRs.  A lane of either kernel is one load -> store chain, hidden by
the other waves of its SIMD, so the budget is four waves per SIMD."""
import pytest

from test_kernel_resources import kernels          # noqa: F401  (the module-scoped fixture that reads the code objects)

NAMES = ("chan_ring_kernel", "chan_gen_kernel")


@pytest.mark.parametrize("name", NAMES)
def test_fold_kernels_exist_within_four_waves_per_simd(kernels, name):           # noqa: F811
    found = {k: v for k, v in kernels.items() if name in k}
    # the general kernel: plain and non-temporal stores; the ring kernel: that times P = 1 .. 8 and one or two columns
    assert len(found) >= (2 if name == "chan_gen_kernel" else 32), (name, sorted(found))
    for k, v in found.items():
        assert not v.get("vgpr_spill_count", 0) and not v.get("sgpr_spill_count", 0), (k, v)
        assert not v.get("private_segment_fixed_size", 0), (k, v)
        assert 0 < v["vgpr_count"] <= 128, (k, v)
    print({k: v["vgpr_count"] for k, v in sorted(found.items())})
