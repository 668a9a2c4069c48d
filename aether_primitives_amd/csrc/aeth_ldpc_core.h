// aeth_ldpc_core.h -- the host algebra of a quasi-cyclic LDPC code in plain C++ (not installed): the checks of
// include/aether_hip.h (aeth_ldpc_*) on a shift table, the compact edge list the kernels read, and the dense parity
// generator P = B^-1 A over GF(2) by Gauss-Jordan elimination on 64-bit words.  aeth_ldpc_generator runs it with no
// context, so the algebra is testable without a device.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "aeth_internal.h"

namespace aeth {
namespace ldpc {

constexpr uint32_t kMaxRows = 256;                     // |Q| <= 128 + 127 rows stays below 2^15
constexpr uint64_t kMaxState = 65536;                  // bytes of decoder state per codeword: 2 N + E z

struct Shape {
    uint32_t rows = 0, cols = 0, z = 0;
    uint32_t N = 0, M = 0, K = 0, E = 0;
    std::vector<uint32_t> row_start;                   // [rows + 1] into edges
    std::vector<uint32_t> edges;                       // [E], row by row, columns ascending: (c z) | (shift << 16)
    uint64_t state() const { return 2ull * N + (uint64_t)E * z; }
};

// every refusal that needs no elimination, in the order of the header; fills `s`
inline int check_code(const aeth_ldpc_code *code, Shape &s)
{
    AETH_REQUIRE(code, AETH_E_ARG, "code is null");
    AETH_REQUIRE(code->shift, AETH_E_ARG, "code->shift is null");
    const uint32_t rows = code->rows, cols = code->cols, z = code->z;
    AETH_REQUIRE(rows >= 1 && rows <= kMaxRows, AETH_E_ARG, "rows = %u outside 1 .. %u", rows, kMaxRows);
    AETH_REQUIRE(cols > rows, AETH_E_ARG, "cols = %u not above rows = %u", cols, rows);
    AETH_REQUIRE(z >= 1, AETH_E_ARG, "z = %u: the block size is at least 1", z);
    const uint64_t n = (uint64_t)cols * z;
    // the table is not read before it is known to be small
    AETH_REQUIRE(2 * n <= kMaxState, AETH_E_UNSUPPORTED, "decoder state of %llu bytes for N = %llu alone: above %llu",
                 (unsigned long long)(2 * n), (unsigned long long)n, (unsigned long long)kMaxState);
    AETH_REQUIRE(code->shift, AETH_E_ARG, "code->shift is null");
    s.rows = rows; s.cols = cols; s.z = z;
    s.N = (uint32_t)n; s.M = rows * z; s.K = s.N - s.M;
    s.row_start.assign(1, 0);
    s.edges.clear();
    for (uint32_t r = 0; r < rows; r++) {
        for (uint32_t c = 0; c < cols; c++) {
            const int32_t v = code->shift[(size_t)r * cols + c];
            AETH_REQUIRE(v >= -1 && (int64_t)v < (int64_t)z, AETH_E_ARG, "shift[%u][%u] = %d outside -1 .. %u", r, c, v, z - 1);
            if (v >= 0) s.edges.push_back((c * z) | ((uint32_t)v << 16));
        }
        AETH_REQUIRE(s.edges.size() > s.row_start.back(), AETH_E_ARG, "row %u holds no block", r);
        s.row_start.push_back((uint32_t)s.edges.size());
    }
    s.E = (uint32_t)s.edges.size();
    AETH_REQUIRE(s.state() <= kMaxState, AETH_E_UNSUPPORTED, "decoder state of %llu bytes (2 N + E z, N = %u, E = %u, z = %u) above %llu",
                 (unsigned long long)s.state(), s.N, s.E, z, (unsigned long long)kMaxState);
    return AETH_OK;
}

inline size_t words_of(uint32_t bits) { return ((size_t)bits + 63) / 64; }

// P [M][words_of(K)]: row i holds parity bit i's taps, bit j at word j / 64, bit j % 64.  [B | A] -> [I | B^-1 A]
inline int generator(const Shape &s, std::vector<uint64_t> &P)
{
    const size_t bw = words_of(s.M), kw = words_of(s.K);
    std::vector<uint64_t> B((size_t)s.M * bw, 0);
    P.assign((size_t)s.M * kw, 0);
    const uint32_t kcols = s.cols - s.rows;
    for (uint32_t r = 0; r < s.rows; r++)
        for (uint32_t e = s.row_start[r]; e < s.row_start[r + 1]; e++) {
            const uint32_t base = s.edges[e] & 0xffffu, sh = s.edges[e] >> 16, c = base / s.z;
            for (uint32_t i = 0; i < s.z; i++) {
                const uint32_t row = r * s.z + i, col = base + (i + sh) % s.z;
                if (c < kcols) P[(size_t)row * kw + col / 64] ^= 1ull << (col % 64);
                else B[(size_t)row * bw + (col - s.K) / 64] ^= 1ull << ((col - s.K) % 64);
            }
        }
    for (uint32_t j = 0; j < s.M; j++) {
        const size_t w = j / 64;
        const uint64_t bit = 1ull << (j % 64);
        uint32_t p = j;
        while (p < s.M && !(B[(size_t)p * bw + w] & bit)) p++;
        AETH_REQUIRE(p < s.M, AETH_E_ARG, "parity part singular: no pivot for column %u of its %u", j, s.M);
        if (p != j) {
            for (size_t k = 0; k < bw; k++) std::swap(B[(size_t)p * bw + k], B[(size_t)j * bw + k]);
            for (size_t k = 0; k < kw; k++) std::swap(P[(size_t)p * kw + k], P[(size_t)j * kw + k]);
        }
        const uint64_t *bj = &B[(size_t)j * bw], *pj = &P[(size_t)j * kw];
        for (uint32_t i = 0; i < s.M; i++) {
            if (i == j || !(B[(size_t)i * bw + w] & bit)) continue;
            uint64_t *bi = &B[(size_t)i * bw], *pi = &P[(size_t)i * kw];
            for (size_t k = w; k < bw; k++) bi[k] ^= bj[k];               // the words in front of w are already 0 in row j
            for (size_t k = 0; k < kw; k++) pi[k] ^= pj[k];
        }
    }
    return AETH_OK;
}

}  // namespace ldpc
}  // namespace aeth
