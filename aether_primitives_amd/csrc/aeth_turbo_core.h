// aeth_turbo_core.h -- the host algebra of a turbo code in plain C++ (not installed): the checks on a constituent code, a
// frame and an interleaver of include/aether_hip.h (aeth_turbo_*), the two masks the kernels read a trellis from, the
// quadratic permutation polynomial, the catalogue of named codes and the geometry of a decoder workgroup.
// aeth_turbo_qpp and aeth_turbo_named run it with no context, so the algebra is testable without a device.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#include "aeth_internal.h"

namespace aeth {
namespace turbo {

constexpr uint32_t kMinK = 3, kMaxK = 5;              // constraint length
constexpr uint32_t kMinBits = 8, kMaxBits = 8192;     // information bits of a frame
constexpr uint32_t kMaxWarm = 8192, kMaxWindows = 1024, kMaxIter = 64;
constexpr uint32_t kLanes = 256;                      // lanes a workgroup aims at: G = kLanes / windows codewords, at least one
constexpr uint32_t kMaxGroup = 64;
constexpr size_t kLdsGroup = 48 * 1024;               // ... as far as their LDS stays within this
constexpr size_t kStoreBudget = (size_t)128 << 20;    // device memory an object spends on alpha stores at the most

inline uint32_t parity(uint32_t v) { return (uint32_t)__builtin_popcount(v) & 1u; }

// A trellis as the kernels read it.  With a = u ^ fbp(s) the step is s' = (a << (nu - 1)) | (s >> 1) whatever the
// polynomials are, so the branches are indexed by a at compile time and the polynomials enter as two masks of S bits:
// bit s of fbm is parity(s & fb & (S - 1)) (u = a ^ that bit), bit s of ffm is parity(s & ff & (S - 1))
// (z = (a & ffmsb) ^ that bit).
struct Trellis {
    uint32_t fbm, ffm, ffmsb;
};

inline Trellis trellis_of(const aeth_turbo_code &c)
{
    const uint32_t S = 1u << (c.k - 1);
    Trellis t{0, 0, (c.ff >> (c.k - 1)) & 1u};
    for (uint32_t s = 0; s < S; s++) {
        t.fbm |= parity(s & c.fb & (S - 1)) << s;
        t.ffm |= parity(s & c.ff & (S - 1)) << s;
    }
    return t;
}

inline int check_code(const aeth_turbo_code *c)
{
    AETH_REQUIRE(c, AETH_E_ARG, "code is null");
    AETH_REQUIRE(c->k >= kMinK && c->k <= kMaxK, AETH_E_UNSUPPORTED, "k = %u outside %u .. %u", c->k, kMinK, kMaxK);
    const uint32_t top = 1u << (c->k - 1);
    AETH_REQUIRE(c->fb < 2 * top && (c->fb & top) && (c->fb & 1u), AETH_E_ARG, "fb = 0%o: bits %u and 0 must be set and none above", c->fb,
                 c->k - 1);
    AETH_REQUIRE(c->ff < 2 * top && (c->ff & 1u), AETH_E_ARG, "ff = 0%o: bit 0 must be set and none above bit %u", c->ff, c->k - 1);
    return AETH_OK;
}

inline int check_bits(uint32_t K)
{
    AETH_REQUIRE(K >= kMinBits && K <= kMaxBits, AETH_E_ARG, "K = %u outside %u .. %u", K, kMinBits, kMaxBits);
    return AETH_OK;
}

// pi[0 .. K) is a permutation of 0 .. K - 1; the refusal names the index and the value
inline int check_permutation(const uint32_t *pi, uint32_t K)
{
    std::vector<int32_t> at(K, -1);
    for (uint32_t i = 0; i < K; i++) {
        AETH_REQUIRE(pi[i] < K, AETH_E_ARG, "pi[%u] = %u is not below K = %u", i, pi[i], K);
        AETH_REQUIRE(at[pi[i]] < 0, AETH_E_ARG, "pi[%u] = %u repeats pi[%d]", i, pi[i], at[pi[i]]);
        at[pi[i]] = (int32_t)i;
    }
    return AETH_OK;
}

inline void qpp(uint32_t K, uint32_t f1, uint32_t f2, std::vector<uint32_t> &pi)
{
    pi.resize(K);
    for (uint64_t i = 0; i < K; i++) pi[i] = (uint32_t)(((uint64_t)f1 * i + (uint64_t)f2 * i * i) % K);   // below 2^59
}

struct Named {
    const char *name;
    aeth_turbo_code code;
};
constexpr Named kNamed[] = {{"lte", {4, 013, 015}}, {"ccsds", {5, 023, 033}}, {"k3", {3, 07, 05}}};

// ---- the decoder workgroup.  A lane owns a window, a workgroup G codewords.  LDS per codeword: the N soft values as they
// came, the K systematic values in interleaved order, and the two a-priori arrays as int16 (value << 1 | hard decision).
constexpr uint32_t pad4(uint32_t v) { return (v + 3u) & ~3u; }
inline uint32_t frame_of(uint32_t K, uint32_t nu) { return 3 * K + 4 * nu; }
inline uint32_t lds_per_codeword(uint32_t K, uint32_t nu) { return pad4(frame_of(K, nu)) + pad4(K) + pad4(4 * K); }
inline uint32_t windows_of(uint32_t K, uint32_t W) { return (K - 1) / W + 1; }
inline uint32_t group_of(uint32_t K, uint32_t nu, uint32_t windows)
{
    const uint32_t by_lanes = kLanes / windows, by_lds = (uint32_t)(kLdsGroup / lds_per_codeword(K, nu));
    return std::max(1u, std::min({by_lanes, by_lds, kMaxGroup}));
}
// dynamic LDS of a workgroup: G codewords, then two disagreement counters per codeword and two words for the group
inline size_t lds_bytes(uint32_t K, uint32_t nu, uint32_t G) { return (size_t)G * lds_per_codeword(K, nu) + (size_t)G * 8 + 8; }
// int32 values of one workgroup's alpha store: [step of the window][lane][state]
inline size_t store_words(uint32_t K, uint32_t W, uint32_t S, uint32_t G, uint32_t windows) { return (size_t)std::min(W, K) * S * G * windows; }

}  // namespace turbo
}  // namespace aeth
