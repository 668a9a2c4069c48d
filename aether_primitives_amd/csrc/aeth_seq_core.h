// aeth_seq_core.h -- linear recurrences over GF(2) by 64-bit windows (reference: src/sequence.rs:18-53).  Plain C++, no
// HIP: aeth_seq_window is this code and nothing else, so the maths is testable on a machine without a GPU.
//
// A register is a set of delays d_k in 1 .. 64: seq[n] = XOR_k seq[n - d_k] for n >= order = max d_k, and seq[i] =
// bit i of `init` below that -- sequence::generate(expand(init, order), |n, s| (sum s[n - d_k]) % 2, len).
// The window W_p holds seq[p .. p+63] (bit i = seq[p + i]) whatever the order.  One step p -> p + 1 is linear:
// shift down, new top bit = parity(W & mask) with mask bit 64 - d_k.  As a 64 x 64 bit matrix P (row r = the input
// bits that XOR into output bit r) a jump by 2^j is P^(2^j), reached by squaring; W_skip takes at most 64
// matrix-vector products from W_0.
#pragma once

#include <cstddef>
#include <cstdint>

namespace aeth {
namespace seq {

struct Mat { uint64_t row[64]; };

inline uint64_t apply(const Mat &m, uint64_t w)
{
    uint64_t o = 0;
    for (int r = 0; r < 64; r++) o |= (uint64_t)__builtin_parityll(m.row[r] & w) << r;
    return o;
}

// out = a * b: apply b, then a
inline void mul(Mat &out, const Mat &a, const Mat &b)
{
    for (int r = 0; r < 64; r++) {
        uint64_t acc = 0;
        for (uint64_t bits = a.row[r]; bits; bits &= bits - 1) acc ^= b.row[__builtin_ctzll(bits)];
        out.row[r] = acc;
    }
}

inline uint64_t step(uint64_t w, uint64_t mask) { return (w >> 1) | ((uint64_t)__builtin_parityll(w & mask) << 63); }

inline Mat step_matrix(uint64_t mask)
{
    Mat p;
    for (int r = 0; r < 63; r++) p.row[r] = 1ull << (r + 1);
    p.row[63] = mask;
    return p;
}

// what is wrong with a register, 0 if nothing: 1 null, 2 ndelays outside 1 .. 64, 3 a delay outside 1 .. 64,
// 4 a repeated delay (`which` = index of the offending delay for 3 and 4)
inline int reg_problem(const uint32_t *delays, size_t ndelays, uint64_t *mask, unsigned *order, size_t *which)
{
    if (!delays) return 1;
    if (ndelays < 1 || ndelays > 64) return 2;
    uint64_t m = 0;
    unsigned ord = 0;
    for (size_t k = 0; k < ndelays; k++) {
        *which = k;
        const uint32_t d = delays[k];
        if (d < 1 || d > 64) return 3;
        const uint64_t bit = 1ull << (64 - d);
        if (m & bit) return 4;
        m |= bit;
        if (d > ord) ord = d;
    }
    *mask = m;
    *order = ord;
    return 0;
}

// W_0: the init bits sit on top of a window 64 - order positions in front of the sequence; the recurrence only ever
// looks `order` bits back, so the positions below are never read and 64 - order plain steps bring the window to 0
inline uint64_t window0(uint64_t mask, unsigned order, uint64_t init)
{
    uint64_t w = (order < 64 ? init & ((1ull << order) - 1) : init) << (64 - order);
    for (unsigned s = order; s < 64; s++) w = step(w, mask);
    return w;
}

// P^(2^j) for j = 0 .. n-1
inline void powers(uint64_t mask, Mat *pw, int n)
{
    pw[0] = step_matrix(mask);
    for (int j = 1; j < n; j++) mul(pw[j], pw[j - 1], pw[j - 1]);
}

// W_skip from kept powers
inline uint64_t window_at(const Mat *pw, uint64_t mask, unsigned order, uint64_t init, uint64_t skip)
{
    uint64_t w = window0(mask, order, init);
    for (int j = 0; j < 64 && (skip >> j); j++)
        if ((skip >> j) & 1) w = apply(pw[j], w);
    return w;
}

// ... and without an object: squares only as far as skip reaches
inline uint64_t window_at(uint64_t mask, unsigned order, uint64_t init, uint64_t skip)
{
    uint64_t w = window0(mask, order, init);
    Mat p = step_matrix(mask), q;
    for (int j = 0; j < 64 && (skip >> j); j++) {
        if ((skip >> j) & 1) w = apply(p, w);
        if (j < 63 && (skip >> (j + 1))) { mul(q, p, p); p = q; }
    }
    return w;
}

}  // namespace seq
}  // namespace aeth
