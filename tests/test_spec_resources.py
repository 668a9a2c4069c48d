"""CPU: the averaged-spectra kernels in the built library's gfx950 code object (the `kernels` fixture of
tests/test_kernel_resources.py): the fused kernel exists for every length x sign x planes x cache policy it is
dispatched for, nothing spills or uses scratch, and the register budgets are what the occupancy was planned for."""
import re

from test_kernel_resources import kernels          # noqa: F401  (the fixture)

FUSED_LENGTHS = (512, 1024, 2048, 4096)


def waves_per_simd(vgprs):
    """512 registers per lane of a SIMD, allocated in blocks of 8"""
    return max(1, min(8, 512 // (-(-vgprs // 8) * 8)))


def named(kernels, word):                          # noqa: F811
    return {k: v for k, v in kernels.items() if word in k}


def clean(v):
    return not (v.get("vgpr_spill_count", 0) or v.get("sgpr_spill_count", 0) or v.get("private_segment_fixed_size", 0))


def test_fused_kernel_is_there_for_every_dispatch_and_spills_nothing(kernels):       # noqa: F811
    fused = named(kernels, "spec_fused_kernel")
    plain = named(kernels, "fft_pow2_stream_kernel")
    assert len(fused) == len(FUSED_LENGTHS) * 2 * 3 * 2, sorted(fused)
    for n in FUSED_LENGTHS:
        ref = [v["vgpr_count"] for k, v in plain.items() if f"CfgILi{n}E" in k]
        for sign in ("Li1E", "Lin1E"):
            for planes in (1, 2, 3):
                for nt in (0, 1):
                    pat = rf"spec_fused_kernel.*CfgILi{n}E\w*?EE{sign}Li{planes}ELb{nt}EEEv"
                    hit = [k for k in fused if re.search(pat, k)]
                    assert len(hit) == 1, (n, sign, planes, nt, hit)
                    v = fused[hit[0]]
                    assert clean(v), (hit[0], v)
                    print(f"spec_fused N={n} sign={sign} planes={planes} nt={nt}: {v['vgpr_count']} VGPRs, "
                          f"{waves_per_simd(v['vgpr_count'])} waves per SIMD, LDS {v.get('group_segment_fixed_size', 0)} B; "
                          f"plain transform {min(ref)}..{max(ref)} VGPRs, {waves_per_simd(max(ref))} waves per SIMD")
                    # two waves per SIMD hide the exchanges: the budget the prefetch was decided by
                    assert v["vgpr_count"] <= 256, (hit[0], v["vgpr_count"])


def test_reduction_kernels_are_lean(kernels):                                         # noqa: F811
    sums = {k: v for k, v in named(kernels, "frame_sums_kernel").items()}
    fold = named(kernels, "frame_sums_fold_kernel")
    head = named(kernels, "spec_head_kernel")
    lev = named(kernels, "sum_levels_kernel")
    assert len(sums) == 2 * 3 * 2 and len(fold) == 1 and len(head) == 1 and len(lev) == 3
    for k, v in {**sums, **fold, **head, **lev}.items():
        assert clean(v), (k, v)
        assert v["vgpr_count"] <= 128, (k, v["vgpr_count"])
