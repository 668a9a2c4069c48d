"""CPU: the builds of the fused FFT*H*IFFT kernel behind aeth_corr_exec_levels and aeth_corr_search are in the library --
every length with store variants (1024, 2048, 4096), both cache policies, every level kind include/aether_hip.h calls one
pass (all three) -- within the register budget of two waves per SIMD, without spills or scratch; and so are the two small
kernels that fold the waves' peak records."""
import re

from test_kernel_resources import kernels          # noqa: F401  (the module-scoped fixture that reads the code objects)

# kernel variant bits (csrc/aeth_fir_kernel.h)
V_LEVEL, V_LV_DB, V_LV_POWER_DB, V_PEAK = 1 << 19, 1 << 20, 1 << 21, 1 << 22
ONE_PASS_KINDS = {"NORM": 0, "DB": V_LV_DB, "POWER_DB": V_LV_POWER_DB}
LENGTHS = (1024, 2048, 4096)


def _clean(v):
    return not v.get("vgpr_spill_count", 0) and not v.get("sgpr_spill_count", 0) and not v.get("private_segment_fixed_size", 0)


def _fmi(kernels):                                  # noqa: F811
    """(N, non-temporal, VAR) -> resources, for every fmi_kernel build"""
    out = {}
    for k, v in kernels.items():
        m = re.search(r"fmi_kernelINS_4fftk3CfgILi(\d+)E.*?EEELb[01]ELi\d+ELb([01])ELb[01]ELi(\d+)EEEv", k)
        if m:
            out[(int(m.group(1)), int(m.group(2)), int(m.group(3)))] = v
    return out


def test_level_and_peak_builds_exist_within_the_register_budget(kernels):      # noqa: F811
    fmi = _fmi(kernels)
    assert len(fmi) >= 40
    mine = {}
    for n in LENGTHS:
        for nt in (0, 1):
            want = {"PEAK": V_PEAK, **{f"LEVEL_{k}": V_LEVEL | bits for k, bits in ONE_PASS_KINDS.items()}}
            for what, bits in want.items():
                mask = V_LEVEL | V_LV_DB | V_LV_POWER_DB | V_PEAK
                found = {key: v for key, v in fmi.items() if key[0] == n and key[1] == nt and (key[2] & mask) == bits}
                assert len(found) == 1, (n, nt, what, sorted(found))
                mine.update(found)
    assert len(mine) == 24
    # nothing else carries the new bits (no length without store variants, no scaled build)
    assert {k for k in fmi if k[2] & (V_LEVEL | V_PEAK)} == set(mine)
    bad = {k: v for k, v in mine.items() if not _clean(v)}
    assert not bad, f"level / peak builds with spills or scratch: {bad}"
    over = {k: v["vgpr_count"] for k, v in mine.items() if v["vgpr_count"] > 256}
    assert not over, f"level / peak builds above 256 VGPRs (one wave per SIMD): {over}"
    print({k: v["vgpr_count"] for k, v in sorted(mine.items())})


def test_fold_kernels_are_present_and_clean(kernels):                          # noqa: F811
    for name in ("corr_fold_kernel", "corr_best_kernel"):
        found = {k: v for k, v in kernels.items() if name in k}
        assert len(found) == 1, (name, sorted(found))
        v = next(iter(found.values()))
        assert _clean(v) and v["vgpr_count"] <= 64, (name, v)
