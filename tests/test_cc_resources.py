"""CPU: the convolutional-code kernels (csrc/aeth_cc.hip) and the soft demodulator (csrc/aeth_modulation.hip) are in the
library's gfx950 code object in every template combination the dispatchers can select -- the decoder for k = 3 .. 7, the
encoder for n = 2 .. 4, the demodulator for 1 .. 8 bits per symbol under both cache policies -- without spills or
scratch, and the decoder within 64 VGPRs (eight waves per SIMD: the serial traceback of one wave hides behind the
forward passes of the others).

Registers, spills and scratch come from the `kernels` fixture of tests/test_kernel_resources.py."""
import re

from test_kernel_resources import kernels          # noqa: F401  (the module-scoped fixture that reads the code objects)


def clean(found):
    for k, v in found.items():
        assert not v.get("vgpr_spill_count", 0) and not v.get("sgpr_spill_count", 0), (k, v)
        assert not v.get("private_segment_fixed_size", 0), (k, v)
        assert v["vgpr_count"] > 0, (k, v)


def test_decoder_exists_for_every_constraint_length_within_64_vgprs(kernels):           # noqa: F811
    found = {k: v for k, v in kernels.items() if "cc_decode_kernel" in k}
    have = {int(re.search(r"cc_decode_kernelILi(\d+)E", k).group(1)) for k in found}
    assert len(found) == 5 and have == {3, 4, 5, 6, 7}, sorted(found)
    clean(found)
    for k, v in found.items():
        assert v["vgpr_count"] <= 64, (k, v)
    print({k: v["vgpr_count"] for k, v in sorted(found.items())})


def test_encoder_exists_for_every_rate(kernels):                                          # noqa: F811
    found = {k: v for k, v in kernels.items() if "cc_encode_kernel" in k}
    have = {int(re.search(r"cc_encode_kernelILi(\d+)E", k).group(1)) for k in found}
    assert len(found) == 3 and have == {2, 3, 4}, sorted(found)
    clean(found)


def test_soft_demodulator_exists_for_every_table_size_and_cache_policy(kernels):          # noqa: F811
    found = {k: v for k, v in kernels.items() if "demod_soft_kernel" in k}
    have = {tuple(int(g) for g in re.search(r"demod_soft_kernelILi(\d+)ELb([01])E", k).groups()) for k in found}
    assert len(found) == 16 and have == {(b, nt) for b in range(1, 9) for nt in (0, 1)}, sorted(found)
    clean(found)
