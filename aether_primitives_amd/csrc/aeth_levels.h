// aeth_levels.h -- the definitions behind aeth_vec_stats, aeth_vec_levels and aeth_fft_exec_levels.  Every kernel
// that produces a norm or a level includes this header and nothing else computes one, so that a translation unit built
// with -ffp-contract=fast (aeth_fft.hip) and one built with -ffp-contract=off (aeth_stats.hip) give the same bits.
//
// For a sample c = (re, im):
//   q(c)    = (double)re * re + (double)im * im.  Both products are exact in f64 (24-bit significands), so the value
//             is ONE rounding of the true |c|^2 and fma(re, re, im * im) gives the same bits: contraction cannot
//             change it.  No finite f32 input overflows or underflows it.
//   norm(c) = (float)sqrt(q(c)), f64 sqrt being correctly rounded.  This is Complex::norm() = hypot (util/plot.rs:65,127)
//             without hypot's platform dependence; it may differ from a correctly rounded hypotf by double rounding in
//             rare cases, which is why this definition, not libm, is the contract.
//   level kinds (include/aether_hip.h):
//     AETH_LEVEL_NORM      norm(c)
//     AETH_LEVEL_DB        (float)(10.0 * log10((double)norm(c))): the reference's literal DB::from(c.norm()).db()
//                          (util/mod.rs:26-34).  NOTE: 10 * log10 of an AMPLITUDE -- the reference's quirk (a power level
//                          of an amplitude would be 20 * log10), reproduced as the default like its other quirks.
//     AETH_LEVEL_POWER_DB  (float)(10.0 * log10(q(c))): the corrected form, the power in dB.
//   norm = 0 gives -inf, a NaN component gives NaN, as Rust's f64::log10 does.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/aether_hip.h"

namespace aeth {

__device__ __forceinline__ double level_q(float re, float im)
{
#pragma clang fp contract(off)
    const double a = (double)re, b = (double)im;
    return a * a + b * b;
}

__device__ __forceinline__ float level_norm_of_q(double q)
{
    return (float)__builtin_sqrt(q);
}

template <int KIND>
__device__ __forceinline__ float level_of(float re, float im)
{
#pragma clang fp contract(off)
    const double q = level_q(re, im);
    if constexpr (KIND == AETH_LEVEL_NORM) return level_norm_of_q(q);
    else if constexpr (KIND == AETH_LEVEL_DB) return (float)(10.0 * log10((double)level_norm_of_q(q)));
    else return (float)(10.0 * log10(q));
}

inline bool level_kind_ok(int kind) { return kind >= AETH_LEVEL_NORM && kind <= AETH_LEVEL_POWER_DB; }

}  // namespace aeth
