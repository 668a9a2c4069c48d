// aeth_crc_core.h -- the algebra of a CRC of width 1 .. 64 in plain C++ (not installed): the definition of
// include/aether_hip.h (aeth_crc_*) as a loop, products and powers modulo the generator, the residue and the table of
// named parameter sets.  aeth_crc.hip uses it on the host and, for the step, the product and the power, in its kernels;
// aeth_crc_host runs it on host memory, so the maths is testable without a device.
//
// Two forms of a register.  The header's `reg` is RIGHT-aligned: coefficient of x^(r-1) at bit r-1.  The kernels and the
// product work LEFT-aligned, reg << (64 - r): the coefficient that decides the feedback is bit 63 for every r, a shift by
// one drops it without a mask, and r enters only as the number of steps of a product.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define AETH_CRC_HD __host__ __device__ __forceinline__
#else
#define AETH_CRC_HD inline
#endif

namespace aeth {
namespace crc {

struct Params { uint32_t r; uint64_t poly, init, xorout; };

AETH_CRC_HD uint64_t mask_of(uint32_t r) { return r >= 64 ? ~0ull : ((1ull << r) - 1); }
AETH_CRC_HD uint64_t to_left(uint64_t v, uint32_t r) { return v << (64 - r); }
AETH_CRC_HD uint64_t to_right(uint64_t v, uint32_t r) { return v >> (64 - r); }

// one message bit b into a left-aligned register; poly_l = to_left(poly)
AETH_CRC_HD uint64_t step_l(uint64_t reg, uint64_t poly_l, uint32_t b)
{
    const uint64_t fb = (reg >> 63) ^ (uint64_t)(b & 1u);
    return (reg << 1) ^ (poly_l & (0 - fb));
}

// a b mod g, all left-aligned: Horner over the r coefficients of a
AETH_CRC_HD uint64_t mulmod_l(uint64_t a, uint64_t b, uint64_t poly_l, uint32_t r)
{
    uint64_t res = 0;
    for (uint32_t i = 0; i < r; i++) {
        res = (res << 1) ^ (poly_l & (0 - (res >> 63))) ^ (b & (0 - (a >> 63)));
        a <<= 1;
    }
    return res;
}

// the polynomial 1, left-aligned
AETH_CRC_HD uint64_t one_l(uint32_t r) { return 1ull << (64 - r); }

// x^n mod g, left-aligned, by square and multiply
inline uint64_t xpow_l(uint64_t n, uint64_t poly_l, uint32_t r)
{
    uint64_t res = one_l(r);
    uint64_t sq = r == 1 ? poly_l : one_l(r) << 1;             // x mod g: g = x + 1 when r == 1
    for (; n; n >>= 1) {
        if (n & 1) res = mulmod_l(res, sq, poly_l, r);
        sq = mulmod_l(sq, sq, poly_l, r);
    }
    return res;
}

// the definition: L bits (one byte per bit, & 1) into a right-aligned register
inline uint64_t run(const Params &p, uint64_t reg, const uint8_t *bits, size_t L)
{
    const uint64_t poly_l = to_left(p.poly, p.r);
    uint64_t a = to_left(reg, p.r);
    for (size_t i = 0; i < L; i++) a = step_l(a, poly_l, bits[i]);
    return to_right(a, p.r);
}

// the register (before xorout) a frame followed by its own check bits leaves: the r bits of xorout run from 0
inline uint64_t residue(const Params &p)
{
    const uint64_t poly_l = to_left(p.poly, p.r);
    uint64_t a = 0;
    for (uint32_t j = 0; j < p.r; j++) a = step_l(a, poly_l, (uint32_t)(p.xorout >> (p.r - 1 - j)));
    return to_right(a, p.r);
}

// 0, or what is wrong with the parameters (`what` names it for the message)
inline const char *check(uint64_t r, uint64_t poly, uint64_t init, uint64_t xorout, uint64_t *bad)
{
    if (r < 1 || r > 64) { *bad = r; return "width"; }
    const uint64_t m = mask_of((uint32_t)r);
    if (!(poly & 1)) { *bad = poly; return "even poly"; }
    if (poly > m) { *bad = poly; return "poly"; }
    if (init > m) { *bad = init; return "init"; }
    if (xorout > m) { *bad = xorout; return "xorout"; }
    return nullptr;
}

struct Named { const char *name; Params p; };
inline const Named *named_table(size_t *n)
{
    static const Named t[] = {
        {"crc-8", {8, 0x07, 0, 0}},
        {"crc-8/lte", {8, 0x9B, 0, 0}},
        {"crc-16/xmodem", {16, 0x1021, 0, 0}},
        {"crc-16/ibm-3740", {16, 0x1021, 0xFFFF, 0}},
        {"crc-16/genibus", {16, 0x1021, 0xFFFF, 0xFFFF}},
        {"crc-24/lte-a", {24, 0x864CFB, 0, 0}},
        {"crc-24/lte-b", {24, 0x800063, 0, 0}},
        {"crc-32/bzip2", {32, 0x04C11DB7, 0xFFFFFFFFull, 0xFFFFFFFFull}},
        {"crc-32", {32, 0x04C11DB7, 0xFFFFFFFFull, 0xFFFFFFFFull}},
        {"crc-64/ecma-182", {64, 0x42F0E1EBA9EA3693ull, 0, 0}},
    };
    *n = sizeof(t) / sizeof(t[0]);
    return t;
}
inline const Named *find_named(const char *name)
{
    size_t n;
    const Named *t = named_table(&n);
    for (size_t i = 0; i < n; i++)
        if (!std::strcmp(t[i].name, name)) return &t[i];
    return nullptr;
}

}  // namespace crc
}  // namespace aeth
