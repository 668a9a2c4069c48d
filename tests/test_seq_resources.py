"""CPU: the four sequence kernels (csrc/aeth_sequence.hip) are in the library's gfx950 code object, in both cache
policies, without spills or scratch and within 64 VGPRs.  The generator is one dependent chain per wave (ballot ->
window -> ballot), hidden only by other waves, so the budget is eight waves per SIMD."""
import pytest

from test_kernel_resources import kernels          # noqa: F401  (the module-scoped fixture that reads the code objects)

NAMES = ("seq_bits_kernel", "seq_scramble_kernel", "seq_chips_kernel", "seq_spread_kernel")


@pytest.mark.parametrize("name", NAMES)
def test_sequence_kernels_exist_within_eight_waves_per_simd(kernels, name):      # noqa: F811
    found = {k: v for k, v in kernels.items() if name in k}
    assert len(found) >= 2, (name, sorted(found))                                # plain and non-temporal stores
    for k, v in found.items():
        assert not v.get("vgpr_spill_count", 0) and not v.get("sgpr_spill_count", 0), (k, v)
        assert not v.get("private_segment_fixed_size", 0), (k, v)
        assert 0 < v["vgpr_count"] <= 64, (k, v)
    print({k: v["vgpr_count"] for k, v in sorted(found.items())})

