"""CPU: the kernels behind aeth_vec_stats, aeth_vec_levels and aeth_fft_exec_levels are in the built library, for every
level kind and cache policy, and none of them spills or uses scratch (the f64 logarithm of the dB kinds included); the
transforms that store levels keep the occupancy of the ones that store the spectrum."""
import re

from test_kernel_resources import kernels          # noqa: F401  (the module-scoped fixture that reads the code objects)


def _clean(v):
    return not v.get("vgpr_spill_count", 0) and not v.get("private_segment_fixed_size", 0)


def test_stats_and_levels_kernels_are_built_without_scratch(kernels):      # noqa: F811
    for pat, count in ((r"stats_partial_kernelILb[01]E", 2), (r"stats_final_kernel", 1), (r"levels_kernelILi[012]ELb[01]E", 6)):
        found = {k: v for k, v in kernels.items() if re.search(pat, k)}
        assert len(found) == count, (pat, sorted(found))
        assert all(_clean(v) for v in found.values()), found
    # 16 loads of 16 bytes in flight per lane and the f64 accumulators: still four waves per SIMD
    assert max(v["vgpr_count"] for k, v in kernels.items() if "stats_partial_kernel" in k) <= 128


def test_level_storing_transforms_keep_their_occupancy(kernels):           # noqa: F811
    """fft_pow2_kernel / fft_pow2_stream_kernel with a level store kind (last template argument 0, 1, 2; -1 is the
    spectrum): every length 2 ... 4096, both signs, both cache policies; no scratch, and the one-frame-per-workgroup
    builds at two waves per SIMD (256 VGPRs) like the ones that store the spectrum"""
    lv = {k: v for k, v in kernels.items() if re.search(r"fft_pow2(_stream)?_kernelI.*Lb[01]ELi[012]EEEv", k)}
    plain = {k: v for k, v in kernels.items() if re.search(r"fft_pow2(_stream)?_kernelI.*Lb[01]ELin1EEEv", k)}
    assert plain, "the spectrum-storing builds carry the store kind -1"
    for n in (2, 4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096):
        mine = [k for k in lv if f"CfgILi{n}E" in k]
        assert len(mine) >= 12, (n, len(mine))                     # 2 signs x 2 cache policies x 3 kinds (x 2 kernels from 512 up)
    assert not [k for k in lv if "CfgILi8192E" in k]                 # 8192 runs the ragged kernel and the two-step path
    assert all(_clean(v) for v in lv.values()), {k: v for k, v in lv.items() if not _clean(v)}
    assert max(v["vgpr_count"] for k, v in lv.items() if "stream_kernel" in k) <= 256
