"""CPU: the OFDM kernels (csrc/aeth_ofdm.hip) are in the library's gfx950 code object -- the fused kernel for all seven
lengths in every combination of direction, equaliser and cache policy; the strip, pick, place, prefix and estimate
kernels -- without spills or scratch, and each fused kernel within the register count that keeps the occupancy of the
plain transform of the same length.

The plain transform of a length is the kernel launch_pow2 (csrc/aeth_fft.hip) launches for it: fft_pow2_stream_kernel where
a workgroup is one frame (N >= 512), fft_pow2_kernel otherwise, for the same sign and cache policy.  Its VGPR count is read
from the same fixture; the allowance is the largest count with the same number of waves per SIMD (registers are handed out
in blocks of 8 from 512 per SIMD lane, at most 8 waves), not a number written down here.  Only the resource notes are read."""
import re

from test_kernel_resources import kernels          # noqa: F401  (the module-scoped fixture that reads the code objects)

LENGTHS = (64, 128, 256, 512, 1024, 2048, 4096)
DEMOD, MOD = 0, 1


def waves_per_simd(vgprs):
    return min(8, 512 // (-(-vgprs // 8) * 8))


def fused(kernels):                                 # noqa: F811
    """{(N, dir, eq, nt): record}; mangled template arguments: ...3CfgILi<N>E...EELi<DIR>ELb<EQ>ELb<NT>EEEv"""
    out = {}
    for k, v in kernels.items():
        if "ofdm_fused_kernel" not in k:
            continue
        m = re.search(r"3CfgILi(\d+)E\w*?EELi([01])ELb([01])ELb([01])EEEv", k)
        assert m, k
        out[tuple(int(g) for g in m.groups())] = v
    return out


def plain(kernels, n, sign, nt):                    # noqa: F811
    name = "fft_pow2_stream_kernel" if n >= 512 else "fft_pow2_kernel"
    sgn = "Li1E" if sign > 0 else "Lin1E"
    hits = {k: v for k, v in kernels.items()
            if re.search(name + r"IN\w*?3CfgILi%dE\w*?EE%sLb%dELin1EEEv" % (n, sgn, nt), k)}
    assert len(hits) == 1, (n, sign, nt, sorted(hits))
    return next(iter(hits.values()))


def test_fused_kernel_exists_in_every_combination(kernels):                                      # noqa: F811
    have = set(fused(kernels))
    want = {(n, DEMOD, eq, nt) for n in LENGTHS for eq in (0, 1) for nt in (0, 1)} | {(n, MOD, 0, nt) for n in LENGTHS for nt in (0, 1)}
    assert have == want, sorted(have ^ want)


def test_fused_kernels_do_not_spill(kernels):                                                    # noqa: F811
    for key, v in fused(kernels).items():
        assert not v.get("vgpr_spill_count", 0) and not v.get("sgpr_spill_count", 0), (key, v)
        assert not v.get("private_segment_fixed_size", 0), (key, v)


def test_fused_kernels_keep_the_occupancy_of_the_plain_transform(kernels):                       # noqa: F811
    report = {}
    for (n, d, eq, nt), v in sorted(fused(kernels).items()):
        ref = plain(kernels, n, +1 if d == DEMOD else -1, nt)
        w_ref, w = waves_per_simd(ref["vgpr_count"]), waves_per_simd(v["vgpr_count"])
        report[(n, d, eq, nt)] = (v["vgpr_count"], ref["vgpr_count"], w, w_ref)
    print(report)
    worse = {k: r for k, r in report.items() if r[2] < r[3]}
    assert not worse, f"(N, dir, eq, nt): (vgprs, plain transform's, waves, plain transform's) {worse}"


def test_copy_and_estimate_kernels_are_present_without_spills(kernels):                          # noqa: F811
    for name, count in (("ofdm_strip_kernel", 1), ("ofdm_pick_kernel", 2), ("ofdm_place_kernel", 1), ("ofdm_prefix_kernel", 1),
                        ("ofdm_estimate_kernel", 1)):
        found = {k: v for k, v in kernels.items() if name in k}
        assert len(found) == count, (name, sorted(found))
        for k, v in found.items():
            assert not v.get("vgpr_spill_count", 0) and not v.get("sgpr_spill_count", 0) and not v.get("private_segment_fixed_size", 0), (k, v)
            assert 0 < v["vgpr_count"] <= 128, (k, v)
