// aeth_nco_core.h -- the oscillator's word arithmetic and the phasor of a word (no body in the reference; the definition
// is in include/aether_hip.h, aeth_nco_*).  One text for the host entry points (aeth_nco_word_at, aeth_nco_phasor) and
// for the kernels of aeth_nco.hip: what the host answers for one word is what every lane computes.
//
// The phase is a 64-bit fraction of a turn.  Its arithmetic is unsigned wrap-around, so it is exact at every stream
// position: w(n) = phase + n step + T(n) rate with T(n) = n (n - 1) / 2.  Moving the origin by m samples keeps the form
// (`advance`): T(m + j) = T(m) + T(j) + m j, hence w(m + j) = w(m) + j (step + m rate) + T(j) rate.  The launch moves
// the origin to its first sample on the host, a workgroup moves it to its tile with scalar arithmetic, and a lane is left
// with a j below 512.
// The phasor is f32, every operation rounded on its own: compile with -ffp-contract=off (the Makefile's EXACT).
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AETH_NCO_HD __host__ __device__ __forceinline__
#else
#define AETH_NCO_HD inline
#endif

namespace aeth {
namespace nco {

struct Words { uint64_t phase, step, rate; };
struct Phasor { float c, d; };                         // cos and sin of the word's angle

// T(n) = n (n - 1) / 2 modulo 2^64: the even factor is halved before the product, so nothing is lost
AETH_NCO_HD uint64_t tri(uint64_t n) { return (n & 1u) ? n * ((n - 1u) >> 1) : (n >> 1) * (n - 1u); }

AETH_NCO_HD uint64_t word_at(const Words &w, uint64_t n) { return w.phase + n * w.step + tri(n) * w.rate; }

// the same oscillator counted from sample m: advance(w, m) at j is w at m + j
AETH_NCO_HD Words advance(const Words &w, uint64_t m) { return Words{word_at(w, m), w.step + m * w.rate, w.rate}; }

constexpr float kTurn = 0x1.921fb6p-30f;               // f32 nearest 2 pi / 2^32
constexpr float kS1 = -0x1.555546p-3f, kS2 = 0x1.11073cp-7f, kS3 = -0x1.9943f2p-13f;      // sin on [-pi/4, pi/4]
constexpr float kC1 = 0x1.55554ap-5f, kC2 = -0x1.6c0c34p-10f, kC3 = 0x1.99eb9cp-16f;      // cos on [-pi/4, pi/4]

AETH_NCO_HD Phasor phasor(uint64_t w)
{
    const uint32_t t = (uint32_t)(w >> 32);
    const uint32_t k = ((t + 0x20000000u) >> 30) & 3u;             // nearest quarter turn
    const int32_t r = (int32_t)(t - (k << 30));                    // -2^29 <= r < 2^29
    const float a = (float)r * kTurn;
    const float s = a * a;
    const float ps = (kS3 * s + kS2) * s + kS1;
    const float sn = (a * s) * ps + a;
    const float pc = (kC3 * s + kC2) * s + kC1;
    const float cs = (1.0f - 0.5f * s) + (s * s) * pc;
    // (cs, sn), (-sn, cs), (-cs, -sn), (sn, -cs) for k = 0, 1, 2, 3
    const float c0 = (k & 1u) ? sn : cs, d0 = (k & 1u) ? cs : sn;
    return Phasor{((k + 1u) & 2u) ? -c0 : c0, (k & 2u) ? -d0 : d0};
}

// aeth_vec_mul's expression (aeth_vecops.hip, OP_MUL) with the phasor as the second operand
AETH_NCO_HD void mix(float xr, float xi, Phasor p, float &re, float &im)
{
    re = xr * p.c - xi * p.d;
    im = xr * p.d + xi * p.c;
}

}  // namespace nco
}  // namespace aeth
