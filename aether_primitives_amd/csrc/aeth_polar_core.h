// aeth_polar_core.h -- the host algebra of a polar code in plain C++ (not installed): the integer polarization weights
// and the reliability order of include/aether_hip.h (aeth_polar_*), the checks on a mask, and the two tables the kernels
// read: the encoder's position table and the decoder's schedule of node visits.  aeth_polar_rank and aeth_polar_mask run
// it with no context, so the algebra is testable without a device.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "aeth_internal.h"

namespace aeth {
namespace polar {

constexpr uint32_t kMinN = 3, kMaxN = 10;
constexpr uint64_t kQ[4] = {4294967296ull, 5107605667ull, 6074001000ull, 7223245206ull};    // round(2^(r/4) 2^32)

inline int check_n(uint32_t n)
{
    AETH_REQUIRE(n >= kMinN && n <= kMaxN, AETH_E_UNSUPPORTED, "n = %u outside %u .. %u", n, kMinN, kMaxN);
    return AETH_OK;
}

inline uint64_t weight(uint32_t i)
{
    uint64_t w = 0;
    for (uint32_t j = 0; j < kMaxN; j++)
        if ((i >> j) & 1u) w += kQ[j & 3u] << (j >> 2);
    return w;
}

// the N positions, most reliable first: larger weight first, ties to the larger position
inline void rank(uint32_t n, std::vector<uint32_t> &order)
{
    const uint32_t N = 1u << n;
    order.resize(N);
    for (uint32_t i = 0; i < N; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [](uint32_t a, uint32_t b) {
        const uint64_t wa = weight(a), wb = weight(b);
        return wa != wb ? wa > wb : a > b;
    });
}

// a schedule word: one node visit of the decoder.  The node takes m = 2^lg values at positions base .. base + m.
//   kF     the left child's values f(a, b)             kG     the right child's values b +- a by the left child's bits
//   kJoin  x[base .. base + m/2) ^= x[base + m/2 ..)   kZero  x[base .. base + m) = 0: a wholly frozen subtree
// A child of `lanes` values is decided in registers right behind its kF / kG; `info` then holds its mask bits.
enum Op : uint32_t { kF = 0, kG = 1, kJoin = 2, kZero = 3 };
inline uint32_t word(Op op, uint32_t lg, uint32_t base, uint32_t info) { return (uint32_t)op | (lg << 2) | (base << 6) | (info << 16); }

inline uint32_t bits_of(const uint8_t *mask, uint32_t base, uint32_t m)
{
    uint32_t v = 0;
    for (uint32_t i = 0; i < m; i++) v |= (uint32_t)(mask[base + i] & 1u) << i;       // m <= 16 where this is used
    return v;
}

inline bool any_info(const uint8_t *mask, uint32_t base, uint32_t m)
{
    for (uint32_t i = 0; i < m; i++)
        if (mask[base + i]) return true;
    return false;
}

// the visits of the subtree (base, 2^lg) in the decoder's order; lg > log2(lanes), and the subtree holds an information bit
inline void schedule(const uint8_t *mask, uint32_t lanes, uint32_t base, uint32_t lg, std::vector<uint32_t> &out)
{
    const uint32_t m = 1u << lg, h = m >> 1;
    const uint32_t halves[2] = {base, base + h};
    for (uint32_t side = 0; side < 2; side++) {
        const uint32_t b = halves[side];
        if (!any_info(mask, b, h)) {                                      // pruned: its values are not needed, only its zero bits
            out.push_back(word(kZero, lg - 1, b, 0));
            continue;
        }
        out.push_back(word(side ? kG : kF, lg, base, h == lanes ? bits_of(mask, b, h) : 0));
        if (h > lanes) schedule(mask, lanes, b, lg - 1, out);
    }
    out.push_back(word(kJoin, lg, base, 0));
}

// ---- the list decoder (aeth_polar_list_*) ----
constexpr uint32_t kMaxList = 8;

inline int check_list(uint32_t L, uint32_t K)
{
    AETH_REQUIRE(L == 1 || L == 2 || L == 4 || L == 8, AETH_E_ARG, "L = %u: a list holds 1, 2, 4 or 8 paths", L);
    AETH_REQUIRE(K >= 3 || (1u << K) >= L, AETH_E_ARG, "K = %u: the code has %u words, fewer than the L = %u paths", K, 1u << K, L);
    return AETH_OK;
}

// lanes per path: not measured yet, so the largest T <= 16 with T L <= 64 and 2 T <= N
inline uint32_t list_lanes(uint32_t n, uint32_t L)
{
    uint32_t T = 16;
    while (T > 4 && (T * L > 64 || 2 * T > (1u << n))) T >>= 1;
    return T;
}

// bytes of LDS per path: the levels of 2 T .. N / 2 int16 values and the packed partial sums, padded to 2 T modulo 128
// so that the lanes of a half wave fall on distinct banks
inline uint32_t list_stride(uint32_t n, uint32_t T)
{
    const uint32_t N = 1u << n, words = N > 32 ? N / 32 : 1;
    const uint32_t raw = 2 * (N - 2 * T) + 4 * words;
    return raw + ((2 * T + 128 - raw % 128) % 128);
}

// the list decoder's visits of the subtree (base, 2^lg): as `schedule`, but a wholly frozen child is visited too, because
// its values add to the path metrics: its kF / kG word carries info = 0 and nothing below it follows.  A child of more
// than `lanes` values that holds information carries info = 1.  No kZero: the frozen visit clears the child's bits.
inline void list_schedule(const uint8_t *mask, uint32_t lanes, uint32_t base, uint32_t lg, std::vector<uint32_t> &out)
{
    const uint32_t m = 1u << lg, h = m >> 1;
    const uint32_t halves[2] = {base, base + h};
    for (uint32_t side = 0; side < 2; side++) {
        const uint32_t b = halves[side];
        const bool frozen = !any_info(mask, b, h);
        out.push_back(word(side ? kG : kF, lg, base, frozen ? 0 : h == lanes ? bits_of(mask, b, h) : 1));
        if (h > lanes && !frozen) list_schedule(mask, lanes, b, lg - 1, out);
    }
    out.push_back(word(kJoin, lg, base, 0));
}

// the encoder's position table: the rank of an information position among the information positions, 0xffff if frozen
inline void positions(const uint8_t *mask, uint32_t N, std::vector<uint16_t> &tab, std::vector<uint16_t> &info)
{
    tab.assign(N, 0xffffu);
    info.clear();
    for (uint32_t i = 0; i < N; i++)
        if (mask[i]) {
            tab[i] = (uint16_t)info.size();
            info.push_back((uint16_t)i);
        }
}

}  // namespace polar
}  // namespace aeth
