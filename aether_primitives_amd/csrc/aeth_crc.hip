// aeth_crc.hip -- frame checks: CRC attach and check over bit frames, and bit packing (no body in the reference;
// definition in include/aether_hip.h, aeth_crc_* and aeth_bits_*).  Everything is integer and defined byte for byte;
// compiled with the EXACT flags like the other bit-exact kernels.
//
// The CRC is linear.  With g the generator, the register of a frame of L bits is
//     state x^L mod g  +  sum_i b_i x^(r + L - 1 - i) mod g
// so a bit's weight depends only on its distance from the frame's end, and nothing needs a serial pass over a frame.
// Registers are held left-aligned (aeth_crc_core.h).
//
// Frames route (L <= kFrameBits).  A group of G = 4 .. 64 lanes owns a frame, 256 / G frames per workgroup.  A lane takes
// the ALIGNED 16 bytes of memory number lane, lane + G, ... of those that hold a bit of the frame, reduces them to a word
// v of 16 bits (first bit highest; bits in front of the frame masked, bits behind it shifted out) and adds v(x) W, where
// W = x^(r + d) mod g belongs to the distance d of the chunk's last bit from the frame's end.  The object keeps
// W[d mod 16][d div 16] in device memory: every aligned chunk of a frame has the same d mod 16, so consecutive lanes read
// consecutive entries.  The product is NOT reduced: it is an 80-bit word, the group adds the lanes' words with xor
// shuffles, and one 16-step reduction brings the top 16 bits back under x^r.  The call's first and last aligned chunk
// are read byte by byte where they reach outside the caller's buffer.
//   Store stage.  attach and check run in the same kernel: the group that knows a frame's register copies its message,
//   & 1, by aligned 16-byte stores (the source is two aligned loads and a byte funnel), and attach puts the check bits
//   behind it; check reads the r received bits, forms diff and the frame's {bad, first} record, which the workgroup folds
//   (aeth_reduce.h) into one record per workgroup and a one-workgroup launch folds into the summary.
// Long route (L > kFrameBits).  Launch 1 treats every chunk of kFrameBits bits as a frame started from 0 and writes its
// register to the object's scratch; launch 2, one workgroup per frame, multiplies every chunk register by x^(bits behind
// the chunk) -- a lane runs Horner over its chunks with x^(256 kFrameBits) and one power by squares from the object's
// table -- folds them and adds the state term.  attach and check then run the store stage as a third launch.
#include "aeth_internal.h"
#include "aeth_crc_core.h"
#include "aeth_reduce.h"

#include <algorithm>
#include <new>
#include <string>
#include <vector>

namespace {

namespace cc = aeth::crc;

constexpr int kBlock = 256;
constexpr uint32_t kFrameBits = 16384;                 // the route boundary, and the long route's chunk
constexpr uint32_t kCols = kFrameBits / 16 + 2;        // d div 16 for d <= kFrameBits + 14
constexpr uint32_t kPart = 65536;                      // output bytes of a frame per workgroup in the store launch
constexpr uint64_t kMaxLen = (uint64_t)1 << 32;
enum { OP_EXEC = 0, OP_ATTACH = 1, OP_CHECK = 2, OP_CHUNKS = 3 };

struct Rec { uint64_t n_bad, first_bad; };             // aeth_crc_summary
struct RecAdd {
    __device__ __forceinline__ Rec operator()(const Rec &a, const Rec &b) const { return Rec{a.n_bad + b.n_bad, a.first_bad < b.first_bad ? a.first_bad : b.first_bad}; }
};
__device__ __forceinline__ uint64_t least(uint64_t a, uint64_t b) { return a < b ? a : b; }

struct CrcCall {
    const uint8_t *in, *in_end;
    const uint64_t *W;                  // [16][kCols], left-aligned
    const uint64_t *state_in;           // [F] right-aligned, or null: `term` is init x^L
    uint64_t *state_out;                // EXEC: [F]; CHUNKS: [F nper]; right-aligned
    uint8_t *out;                       // ATTACH: frames of L + r bytes; CHECK: payload or null
    uint64_t *diff;                     // CHECK, or null
    Rec *recs;                          // CHECK with a summary: one per workgroup, or null
    uint64_t items, F, L, stride_in;
    uint64_t poly_l, xl, term, xorout, mask;
    uint32_t nper, tail;                // CHUNKS: chunks per frame, bits of the last
    uint32_t r, lg_g, op;
};

// 16 bytes at the 16-byte aligned A; bytes outside [lo, hi) read as 0 and are not touched
template <bool NT> __device__ __forceinline__ uint4 load16_al(const uint8_t *A, const uint8_t *lo, const uint8_t *hi)
{
    if (A >= lo && A + 16 <= hi) return aeth::nt_load<NT>(reinterpret_cast<const uint4 *>(A));
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        uint32_t b = 0;
        if (A + k >= lo && A + k < hi) b = (uint32_t)A[k] << (8 * (k & 3));
        if (k < 4) w0 |= b; else if (k < 8) w1 |= b; else if (k < 12) w2 |= b; else w3 |= b;
    }
    return uint4{w0, w1, w2, w3};
}

// 16 bytes at any p: two aligned loads and a funnel by p & 15 bytes
template <bool NT> __device__ __forceinline__ uint4 load16_any(const uint8_t *p, const uint8_t *lo, const uint8_t *hi)
{
    const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u);
    const uint8_t *A = p - sh;
    const uint4 x = load16_al<NT>(A, lo, hi);
    if (sh == 0) return x;
    const uint4 y = load16_al<NT>(A + 16, lo, hi);
    const uint32_t ws = sh >> 2, bs = (sh & 3u) * 8;
    auto pick = [&](uint32_t a, uint32_t b, uint32_t c, uint32_t d) { return ws == 0 ? a : ws == 1 ? b : ws == 2 ? c : d; };
    const uint32_t u0 = pick(x.x, x.y, x.z, x.w), u1 = pick(x.y, x.z, x.w, y.x), u2 = pick(x.z, x.w, y.x, y.y), u3 = pick(x.w, y.x, y.y, y.z),
                   u4 = pick(y.x, y.y, y.z, y.w);
    auto fun = [&](uint32_t l, uint32_t h) { return (uint32_t)((((uint64_t)h << 32) | l) >> bs); };
    return uint4{fun(u0, u1), fun(u1, u2), fun(u2, u3), fun(u3, u4)};
}

// the low bits of four bytes as a nibble: the first byte highest / lowest
__device__ __forceinline__ uint32_t nib_msb(uint32_t w) { return (((w & 0x01010101u) * 0x08040201u) >> 24) & 0xFu; }
__device__ __forceinline__ uint32_t nib_lsb(uint32_t w) { return (((w & 0x01010101u) * 0x01020408u) >> 24) & 0xFu; }
__device__ __forceinline__ uint32_t bits16_msb(const uint4 &v) { return (nib_msb(v.x) << 12) | (nib_msb(v.y) << 8) | (nib_msb(v.z) << 4) | nib_msb(v.w); }
__device__ __forceinline__ uint32_t bits16_lsb(const uint4 &v) { return nib_lsb(v.x) | (nib_lsb(v.y) << 4) | (nib_lsb(v.z) << 8) | (nib_lsb(v.w) << 12); }
// four bits, the lowest first, as four bytes 0 / 1
__device__ __forceinline__ uint32_t spread4(uint32_t t) { return (t & 1u) | ((t & 2u) << 7) | ((t & 4u) << 14) | ((t & 8u) << 21); }

// Bytes [o_begin, o_end) of one frame's output at dst + o: o < L is src[o] & 1, o >= L is check bit o - L of `value`
// (0 behind the r-th).  `nl` lanes share the aligned 16-byte chunks of the range; what is not a whole chunk goes out
// byte by byte.
template <bool NT>
__device__ __forceinline__ void emit(uint8_t *dst, uint64_t o_begin, uint64_t o_end, const uint8_t *src, uint64_t L, uint64_t value, uint32_t r,
                                     const uint8_t *lo, const uint8_t *hi, uint32_t lane, uint32_t nl)
{
    if (o_end <= o_begin) return;
    const uint32_t osh = (uint32_t)(reinterpret_cast<uintptr_t>(dst + o_begin) & 15u);
    const uint64_t end = osh + (o_end - o_begin);
    for (uint64_t e0 = (uint64_t)lane << 4; e0 < end; e0 += (uint64_t)nl << 4) {
        const int64_t o0 = (int64_t)(o_begin + e0) - (int64_t)osh;        // the chunk's first byte in the frame; may lie in front of it
        uint32_t w[4] = {0, 0, 0, 0};
        if (o0 < (int64_t)L) {
            const uint4 m = load16_any<false>(src + o0, lo, hi);
            w[0] = m.x & 0x01010101u; w[1] = m.y & 0x01010101u; w[2] = m.z & 0x01010101u; w[3] = m.w & 0x01010101u;
        }
        if (o0 + 16 > (int64_t)L) {
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const int64_t o = o0 + k;
                if (o >= (int64_t)L) {
                    const uint64_t j = (uint64_t)(o - (int64_t)L);
                    const uint32_t bit = j < r ? (uint32_t)((value >> (r - 1 - j)) & 1u) : 0u;
                    w[k >> 2] = (w[k >> 2] & ~(0xffu << (8 * (k & 3)))) | (bit << (8 * (k & 3)));
                }
            }
        }
        uint8_t *p = dst + o0;                                            // 16-byte aligned
        if (e0 >= osh && e0 + 16 <= end) {
            aeth::nt_store<NT>(reinterpret_cast<uint4 *>(p), uint4{w[0], w[1], w[2], w[3]});
        } else {
#pragma unroll
            for (int k = 0; k < 16; k++)
                if (e0 + k >= osh && e0 + k < end) p[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
        }
    }
}

// the received check bits j = lane, lane + nl, ... of a frame as a word, first bit highest
__device__ __forceinline__ uint64_t recv_part(const uint8_t *src, uint64_t L, uint32_t r, uint32_t lane, uint32_t nl)
{
    uint64_t word = 0;
    for (uint32_t j = lane; j < r; j += nl) word |= (uint64_t)(src[L + j] & 1u) << (r - 1 - j);
    return word;
}

// ---- registers: the frames route, and the chunk launch of the long route --------------------------------------------
template <bool NT, bool LONG> __device__ __forceinline__ void crc_body(const CrcCall &a, Rec *lds)
{
    const uint32_t G = 1u << a.lg_g;
    const uint32_t lane = threadIdx.x & (G - 1);
    const uint64_t item = (uint64_t)blockIdx.x * (kBlock >> a.lg_g) + (threadIdx.x >> a.lg_g);
    const bool active = item < a.items;
    const uint8_t *s = a.in;
    uint32_t len = 0;
    if (active) {
        if constexpr (LONG) {
            const uint32_t f = (uint32_t)item / a.nper, k = (uint32_t)item - f * a.nper;
            s = a.in + (uint64_t)f * a.stride_in + (uint64_t)k * kFrameBits;
            len = k + 1 < a.nper ? kFrameBits : a.tail;
        } else {
            s = a.in + item * a.stride_in;
            len = (uint32_t)a.L;
        }
    }
    // the lanes' unreduced sums
    const uint32_t e = (uint32_t)(reinterpret_cast<uintptr_t>(s) & 15u);
    const uint8_t *A0 = s - e;
    const uint32_t nc = len ? (e + len + 15) >> 4 : 0;
    const int32_t dtop = (int32_t)(len + e) - 16;                         // distance of chunk 0's last bit from the frame's end
    uint64_t lo = 0;
    uint32_t hi = 0;
    for (uint32_t c = lane; c < nc; c += G) {
        const uint4 raw = load16_al<NT>(A0 + 16 * (size_t)c, a.in, a.in_end);
        uint32_t v = bits16_msb(raw);
        if (c == 0) v &= 0xFFFFu >> e;
        int32_t d = dtop - 16 * (int32_t)c;
        if (d < 0) { v >>= -d; d = 0; }                                   // the frame ends inside the chunk: right alignment
        const uint64_t w = a.W[(uint32_t)(d & 15) * kCols + (uint32_t)(d >> 4)];
        uint64_t plo = 0;
        uint32_t phi = 0;
#pragma unroll
        for (int k = 15; k >= 0; k--) {
            phi = (phi << 1) | (uint32_t)(plo >> 63);
            plo = (plo << 1) ^ (w & (0 - (uint64_t)((v >> k) & 1u)));
        }
        lo ^= plo;
        hi ^= phi;
    }
    for (uint32_t m = G >> 1; m; m >>= 1) {
        lo ^= __shfl_xor((unsigned long long)lo, (int)m);
        hi ^= __shfl_xor(hi, (int)m);
    }
    uint64_t red = 0;
#pragma unroll
    for (int k = 15; k >= 0; k--) red = cc::step_l(red, a.poly_l, hi >> k);
    uint64_t reg = lo ^ red;
    if constexpr (!LONG) {
        if (a.state_in) {
            uint64_t t = 0;
            if (active && lane == 0) t = cc::mulmod_l(cc::to_left(a.state_in[item], a.r), a.xl, a.poly_l, a.r);
            reg ^= __shfl((unsigned long long)t, (int)((threadIdx.x & 63u) & ~(G - 1)));
        } else {
            reg ^= a.term;
        }
    }
    const uint64_t reg_r = cc::to_right(reg, a.r);
    if (a.op == OP_EXEC || a.op == OP_CHUNKS) {
        if (active && lane == 0) a.state_out[item] = reg_r;
        return;
    }
    if constexpr (!LONG) {
        const uint64_t value = reg_r ^ a.xorout;
        if (a.op == OP_ATTACH) {
            if (active) emit<NT>(a.out + item * (a.L + a.r), 0, a.L + a.r, s, a.L, value, a.r, a.in, a.in_end, lane, G);
            return;
        }
        uint64_t word = active ? recv_part(s, a.L, a.r, lane, G) : 0;
        for (uint32_t m = G >> 1; m; m >>= 1) word ^= __shfl_xor((unsigned long long)word, (int)m);
        const uint64_t diff = word ^ value ^ a.mask;
        if (active && lane == 0 && a.diff) a.diff[item] = diff;
        if (active && a.out) emit<NT>(a.out + item * a.L, 0, a.L, s, a.L, 0, a.r, a.in, a.in_end, lane, G);
        if (a.recs) {                                                     // uniform over the launch
            Rec rec{0, a.F};
            if (active && lane == 0 && diff) rec = Rec{1, item};
            rec = aeth::red::block_reduce(rec, lds, RecAdd{});
            if (threadIdx.x == 0) a.recs[blockIdx.x] = rec;
        }
    }
}

template <bool NT> __global__ __launch_bounds__(kBlock) void crc_frames_kernel(CrcCall a)
{
    __shared__ Rec lds[4];
    crc_body<NT, false>(a, lds);
}
template <bool NT> __global__ __launch_bounds__(kBlock) void crc_long_kernel(CrcCall a)
{
    crc_body<NT, true>(a, nullptr);
}

// ---- the long route's second launch: one workgroup per frame ---------------------------------------------------------
struct CombineCall {
    const uint64_t *chunks;             // [F][nper] right-aligned, started from 0
    const uint64_t *P;                  // [32]: x^(2^i) mod g, left-aligned
    const uint64_t *state_in;           // [F] or null
    uint64_t *regs;                     // [F] right-aligned
    uint64_t poly_l, step, xl, term;    // step = x^(256 kFrameBits)
    uint32_t nper, tail, r;
};
__global__ __launch_bounds__(kBlock) void crc_combine_kernel(CombineCall a)
{
    __shared__ uint64_t lds[4];
    const uint64_t *regs = a.chunks + (uint64_t)blockIdx.x * a.nper;
    const uint32_t n1 = a.nper - 1;                                       // the chunks in front of the last
    uint64_t acc = 0;
    uint32_t last = ~0u;
    for (uint32_t k = threadIdx.x; k < n1; k += kBlock) {
        acc = cc::mulmod_l(acc, a.step, a.poly_l, a.r) ^ cc::to_left(regs[k], a.r);
        last = k;
    }
    if (last != ~0u) {
        const uint64_t behind = (uint64_t)(n1 - 1 - last) * kFrameBits + a.tail;      // bits behind the lane's last chunk: below 2^32
        uint64_t m = cc::one_l(a.r);
        for (int i = 0; i < 32; i++)
            if ((behind >> i) & 1u) m = cc::mulmod_l(m, a.P[i], a.poly_l, a.r);
        acc = cc::mulmod_l(acc, m, a.poly_l, a.r);
    }
    acc = aeth::red::block_reduce(acc, lds, [](uint64_t x, uint64_t y) { return x ^ y; });
    if (threadIdx.x == 0) {
        acc ^= cc::to_left(regs[n1], a.r);
        acc ^= a.state_in ? cc::mulmod_l(cc::to_left(a.state_in[blockIdx.x], a.r), a.xl, a.poly_l, a.r) : a.term;
        a.regs[blockIdx.x] = cc::to_right(acc, a.r);
    }
}

// ---- the long route's store stage: kPart output bytes of a frame per workgroup -----------------------------------------
struct StoreCall {
    const uint8_t *in, *in_end;
    const uint64_t *regs;               // [F] right-aligned
    uint8_t *out;
    uint64_t *diff;
    Rec *recs;
    uint64_t F, L, xorout, mask;
    uint32_t parts, r, op;
};
template <bool NT> __global__ __launch_bounds__(kBlock) void crc_store_kernel(StoreCall a)
{
    __shared__ Rec lds[4];
    const uint64_t f = blockIdx.x / a.parts, q = blockIdx.x - f * a.parts;
    const uint64_t value = a.regs[f] ^ a.xorout;
    if (a.op == OP_ATTACH) {
        const uint64_t n = a.L + a.r;
        emit<NT>(a.out + f * n, q * kPart, least(n, (q + 1) * kPart), a.in + f * a.L, a.L, value, a.r, a.in, a.in_end, threadIdx.x, kBlock);
        return;
    }
    const uint8_t *src = a.in + f * (a.L + a.r);
    if (a.out) emit<NT>(a.out + f * a.L, q * kPart, least(a.L, (q + 1) * kPart), src, a.L, 0, a.r, a.in, a.in_end, threadIdx.x, kBlock);
    Rec rec{0, a.F};
    if (q == 0 && threadIdx.x == 0) {
        const uint64_t diff = recv_part(src, a.L, a.r, 0, 1) ^ value ^ a.mask;
        if (a.diff) a.diff[f] = diff;
        if (diff) rec = Rec{1, f};
    }
    if (a.recs) {
        rec = aeth::red::block_reduce(rec, lds, RecAdd{});
        if (threadIdx.x == 0) a.recs[blockIdx.x] = rec;
    }
}

__global__ __launch_bounds__(kBlock) void crc_summary_kernel(const Rec *recs, size_t n, uint64_t F, Rec *out)
{
    __shared__ Rec lds[4];
    const Rec t = aeth::red::fold(recs, n, n, Rec{0, F}, lds, RecAdd{});
    if (threadIdx.x == 0) *out = t;
}

// ---- bit packing ----------------------------------------------------------------------------------------------------
// a lane packs the 16 bits at bits + 16 j into bytes 2 j and 2 j + 1
template <bool NT> __global__ __launch_bounds__(kBlock) void bits_pack_kernel(const uint8_t *bits, uint64_t nbits, int msb, uint8_t *bytes, uint64_t nbytes)
{
    const uint64_t nch = (nbits + 15) >> 4;
    for (uint64_t j = (uint64_t)blockIdx.x * kBlock + threadIdx.x; j < nch; j += (uint64_t)gridDim.x * kBlock) {
        const uint4 raw = load16_any<NT>(bits + 16 * j, bits, bits + nbits);
        uint32_t b0, b1;
        if (msb) { const uint32_t v = bits16_msb(raw); b0 = v >> 8; b1 = v & 0xffu; }
        else { const uint32_t v = bits16_lsb(raw); b0 = v & 0xffu; b1 = v >> 8; }
        bytes[2 * j] = (uint8_t)b0;
        if (2 * j + 1 < nbytes) bytes[2 * j + 1] = (uint8_t)b1;
    }
}

// a lane writes an aligned 16 bytes of the bit side from at most three packed bytes
template <bool NT> __global__ __launch_bounds__(kBlock) void bits_unpack_kernel(const uint8_t *bytes, uint64_t nbytes, int msb, uint8_t *bits, uint64_t nbits)
{
    const uint32_t osh = (uint32_t)(reinterpret_cast<uintptr_t>(bits) & 15u);
    const uint64_t end = osh + nbits, nch = (end + 15) >> 4;
    for (uint64_t c = (uint64_t)blockIdx.x * kBlock + threadIdx.x; c < nch; c += (uint64_t)gridDim.x * kBlock) {
        const int64_t i0 = (int64_t)(c << 4) - (int64_t)osh;              // the chunk's first bit; negative in front of the stream
        const int64_t q = i0 >> 3;                                        // floor
        uint32_t win = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            uint32_t b = 0;
            if (q + k >= 0 && (uint64_t)(q + k) < nbytes) b = bytes[q + k];
            if (msb) b = __brev(b) >> 24;
            win |= b << (8 * k);
        }
        const uint32_t t = win >> (uint32_t)(i0 - 8 * q);
        const uint32_t w0 = spread4(t), w1 = spread4(t >> 4), w2 = spread4(t >> 8), w3 = spread4(t >> 12);
        uint8_t *p = bits + i0;                                           // 16-byte aligned
        if (i0 >= 0 && (uint64_t)i0 + 16 <= nbits) {
            aeth::nt_store<NT>(reinterpret_cast<uint4 *>(p), uint4{w0, w1, w2, w3});
        } else {
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const uint32_t w = k < 4 ? w0 : k < 8 ? w1 : k < 12 ? w2 : w3;
                if (i0 + k >= 0 && (uint64_t)(i0 + k) < nbits) p[k] = (uint8_t)(w >> (8 * (k & 3)));
            }
        }
    }
}

// ---- host -----------------------------------------------------------------------------------------------------------
int check_params(uint64_t r, uint64_t poly, uint64_t init, uint64_t xorout)
{
    AETH_REQUIRE(r >= 1 && r <= 64, AETH_E_ARG, "width r = %llu outside 1 .. 64", (unsigned long long)r);
    const uint64_t m = cc::mask_of((uint32_t)r);
    AETH_REQUIRE(poly & 1, AETH_E_ARG, "poly 0x%llx is even: bit 0 of the generator must be set", (unsigned long long)poly);
    AETH_REQUIRE(poly <= m, AETH_E_ARG, "poly 0x%llx at or above 2^%llu", (unsigned long long)poly, (unsigned long long)r);
    AETH_REQUIRE(init <= m, AETH_E_ARG, "init 0x%llx at or above 2^%llu", (unsigned long long)init, (unsigned long long)r);
    AETH_REQUIRE(xorout <= m, AETH_E_ARG, "xorout 0x%llx at or above 2^%llu", (unsigned long long)xorout, (unsigned long long)r);
    return AETH_OK;
}

using aeth::mul_sat;

}  // namespace

struct aeth_crc {
    aeth_ctx *ctx;
    cc::Params p;
    uint64_t poly_l;
    uint64_t step;                      // x^(256 kFrameBits), left-aligned
    uint64_t *tab_dev;                  // [16][kCols] weights, then [32] powers x^(2^i)
    aeth::DevScratch slab;              // long route: [chunk registers][frame registers]; check: [workgroup records]
};

namespace {

int route_of(const aeth_crc *crc, size_t L)
{
    const int forced = aeth::tuning_int("AETH_CRC_ROUTE", 0);
    if (forced == AETH_CRC_ROUTE_LONG && L >= 1) return AETH_CRC_ROUTE_LONG;
    (void)crc;
    return L <= kFrameBits ? AETH_CRC_ROUTE_FRAMES : AETH_CRC_ROUTE_LONG;
}

// lanes of a group, as a power of two: enough to hold a frame of `bytes` bytes at any alignment in one pass, 4 .. 64
uint32_t group_lg(uint64_t bytes)
{
    const uint64_t nc = (bytes + 15 + 15) >> 4;
    uint32_t lg = 2;
    while (lg < 6 && (1ull << lg) < nc) lg++;
    return lg;
}

struct Plan {
    int op;
    const uint8_t *in;
    uint64_t L, F, stride_in;
    const uint64_t *state_in;
    uint64_t *state_out;
    uint8_t *out;
    uint64_t *diff;
    Rec *summary;
    uint64_t mask;
};

// everything behind the checks: the launches of exec, attach and check
int run(aeth_crc *crc, const Plan &pl)
{
    aeth_ctx *ctx = crc->ctx;
    aeth::DeviceGuard dg(ctx->device);
    const uint32_t r = crc->p.r;
    const uint64_t in_bytes = pl.F * pl.stride_in;
    const uint64_t out_bytes = pl.op == OP_ATTACH ? pl.F * (pl.L + r) : pl.op == OP_CHECK && pl.out ? pl.F * pl.L : pl.F * 8;
    const bool nt = aeth::streams_past_cache(in_bytes + out_bytes);
    const bool lng = pl.F && route_of(crc, pl.L) == AETH_CRC_ROUTE_LONG;
    const uint64_t nper = lng ? (pl.L + kFrameBits - 1) / kFrameBits : 0;
    const uint32_t lg_g = lng ? 6 : group_lg(pl.op == OP_EXEC ? pl.L : pl.L + r);
    const uint32_t fpw = kBlock >> lg_g;
    const uint32_t parts = pl.op == OP_ATTACH ? (uint32_t)((pl.L + r + kPart - 1) / kPart) : pl.op == OP_CHECK && pl.out ? (uint32_t)((pl.L + kPart - 1) / kPart) : 1;
    // workgroups of the launch that makes the records
    const uint64_t rec_wgs = !pl.summary || !pl.F ? 0 : lng ? pl.F * parts : (pl.F + fpw - 1) / fpw;
    const bool store_launch = lng && pl.op != OP_EXEC;
    const uint64_t n_chunk = lng ? pl.F * nper : 0, n_regs = store_launch ? pl.F : 0;
    AETH_REQUIRE(n_chunk < kMaxLen && (lng ? pl.F * parts : pl.F / fpw + 1) < ((uint64_t)1 << 31), AETH_E_UNSUPPORTED,
                 "%llu frames in one call: more than 2^31 workgroups", (unsigned long long)pl.F);
    const size_t slab_bytes = (size_t)((n_chunk + n_regs) * 8 + rec_wgs * sizeof(Rec));
    if (slab_bytes) { int rc = aeth::scratch_ensure(ctx, crc->slab, slab_bytes); if (rc) return rc; }
    uint64_t *chunks = static_cast<uint64_t *>(crc->slab.p), *regs = chunks + n_chunk;
    Rec *recs = rec_wgs ? reinterpret_cast<Rec *>(regs + n_regs) : nullptr;
    hipStream_t st = aeth::ctx_stream(ctx);
    const uint64_t xl = cc::xpow_l(pl.L, crc->poly_l, r);
    const uint64_t term = cc::mulmod_l(cc::to_left(crc->p.init, r), xl, crc->poly_l, r);

    if (pl.F) {
        CrcCall a{};
        a.in = pl.in;
        a.in_end = pl.in + in_bytes;
        a.W = crc->tab_dev;
        a.F = pl.F; a.L = pl.L; a.stride_in = pl.stride_in;
        a.poly_l = crc->poly_l; a.xl = xl; a.term = term; a.xorout = crc->p.xorout; a.mask = pl.mask;
        a.r = r; a.lg_g = lg_g;
        if (!lng) {
            a.items = pl.F;
            a.state_in = pl.state_in; a.state_out = pl.state_out;
            a.out = pl.out; a.diff = pl.diff; a.recs = recs;
            a.op = pl.op;
            const dim3 grid((unsigned)((pl.F + fpw - 1) / fpw)), block(kBlock);
            if (nt) hipLaunchKernelGGL(crc_frames_kernel<true>, grid, block, 0, st, a);
            else hipLaunchKernelGGL(crc_frames_kernel<false>, grid, block, 0, st, a);
        } else {
            a.items = n_chunk;
            a.nper = (uint32_t)nper;
            a.tail = (uint32_t)(pl.L - (nper - 1) * kFrameBits);
            a.state_out = chunks;
            a.op = OP_CHUNKS;
            const dim3 grid((unsigned)((n_chunk + fpw - 1) / fpw)), block(kBlock);
            if (nt) hipLaunchKernelGGL(crc_long_kernel<true>, grid, block, 0, st, a);
            else hipLaunchKernelGGL(crc_long_kernel<false>, grid, block, 0, st, a);
            CombineCall c{};
            c.chunks = chunks;
            c.P = crc->tab_dev + 16 * kCols;
            c.state_in = pl.state_in;
            c.regs = store_launch ? regs : pl.state_out;
            c.poly_l = crc->poly_l; c.step = crc->step; c.xl = xl; c.term = term;
            c.nper = a.nper; c.tail = a.tail; c.r = r;
            hipLaunchKernelGGL(crc_combine_kernel, dim3((unsigned)pl.F), dim3(kBlock), 0, st, c);
            if (store_launch) {
                StoreCall s{};
                s.in = pl.in; s.in_end = a.in_end;
                s.regs = regs; s.out = pl.out; s.diff = pl.diff; s.recs = recs;
                s.F = pl.F; s.L = pl.L; s.xorout = crc->p.xorout; s.mask = pl.mask;
                s.parts = parts; s.r = r; s.op = pl.op;
                const dim3 grid2((unsigned)(pl.F * parts));
                if (nt) hipLaunchKernelGGL(crc_store_kernel<true>, grid2, block, 0, st, s);
                else hipLaunchKernelGGL(crc_store_kernel<false>, grid2, block, 0, st, s);
            }
        }
    }
    if (pl.summary) hipLaunchKernelGGL(crc_summary_kernel, dim3(1), dim3(kBlock), 0, st, (const Rec *)recs, (size_t)rec_wgs, pl.F, pl.summary);
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

}  // namespace

extern "C" {

int aeth_crc_named(const char *name, uint32_t *r, uint64_t *poly, uint64_t *init, uint64_t *xorout)
{
    AETH_REQUIRE(name && r && poly && init && xorout, AETH_E_ARG, "null pointer");
    const cc::Named *n = cc::find_named(name);
    if (!n) {
        size_t cnt;
        const cc::Named *t = cc::named_table(&cnt);
        std::string known;
        for (size_t i = 0; i < cnt; i++) known += std::string(i ? ", " : "") + t[i].name;
        return aeth::set_error(AETH_E_ARG, "unknown CRC name \"%.40s\"; known: %s", name, known.c_str());
    }
    *r = n->p.r; *poly = n->p.poly; *init = n->p.init; *xorout = n->p.xorout;
    return AETH_OK;
}

int aeth_crc_host(uint32_t r, uint64_t poly, uint64_t init, uint64_t xorout, const uint8_t *bits_host, size_t L, uint64_t *reg)
{
    AETH_REQUIRE(reg, AETH_E_ARG, "reg is null");
    int rc = check_params(r, poly, init, xorout);
    if (rc) return rc;
    AETH_REQUIRE(bits_host || !L, AETH_E_ARG, "bits_host is null");
    *reg = cc::run(cc::Params{r, poly, init, xorout}, init, bits_host, L);
    return AETH_OK;
}

int aeth_crc_create(aeth_ctx *ctx, uint32_t r, uint64_t poly, uint64_t init, uint64_t xorout, aeth_crc **out)
{
    AETH_REQUIRE(out, AETH_E_ARG, "out is null");
    *out = nullptr;
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    int rc = check_params(r, poly, init, xorout);
    if (rc) return rc;
    aeth_crc *crc = new (std::nothrow) aeth_crc{};
    AETH_REQUIRE(crc, AETH_E_NOMEM, "out of host memory");
    crc->ctx = ctx;
    crc->p = cc::Params{r, poly, init, xorout};
    crc->poly_l = cc::to_left(poly, r);
    crc->step = cc::xpow_l((uint64_t)kBlock * kFrameBits, crc->poly_l, r);
    std::vector<uint64_t> tab((size_t)16 * kCols + 32);
    uint64_t w = crc->poly_l;                                             // x^r mod g
    for (uint32_t d = 0; d < 16 * kCols; d++) {
        tab[(size_t)(d & 15) * kCols + (d >> 4)] = w;
        w = cc::step_l(w, crc->poly_l, 0);
    }
    uint64_t sq = cc::xpow_l(1, crc->poly_l, r);
    for (int i = 0; i < 32; i++) {
        tab[(size_t)16 * kCols + i] = sq;
        sq = cc::mulmod_l(sq, sq, crc->poly_l, r);
    }
    aeth::DeviceGuard dg(ctx->device);
    rc = aeth::upload_table(ctx, tab.data(), tab.size() * sizeof(uint64_t), &crc->tab_dev, "aeth_crc_create: weight table");
    if (rc) { delete crc; return rc; }
    *out = crc;
    return AETH_OK;
}

int aeth_crc_destroy(aeth_crc *crc)
{
    if (!crc) return AETH_OK;
    const hipError_t freed = aeth::release_tables(crc->ctx, {crc->slab.p, crc->tab_dev});
    delete crc;
    return freed == hipSuccess ? AETH_OK : aeth::hip_fail(freed, "hipFree");
}

uint32_t aeth_crc_width(const aeth_crc *crc) { return crc ? crc->p.r : 0; }
uint64_t aeth_crc_poly(const aeth_crc *crc) { return crc ? crc->p.poly : 0; }
uint64_t aeth_crc_init(const aeth_crc *crc) { return crc ? crc->p.init : 0; }
uint64_t aeth_crc_xorout(const aeth_crc *crc) { return crc ? crc->p.xorout : 0; }
uint64_t aeth_crc_residue(const aeth_crc *crc) { return crc ? cc::residue(crc->p) : 0; }
int aeth_crc_route(const aeth_crc *crc, size_t L, size_t F) { (void)F; return crc ? route_of(crc, L) : 0; }
size_t aeth_crc_route_frame_bits(const aeth_crc *crc) { return crc ? kFrameBits : 0; }
size_t aeth_crc_frames_per_workgroup(const aeth_crc *crc, size_t frame_bytes)
{
    return crc ? (size_t)kBlock >> group_lg(frame_bytes) : 0;
}

int aeth_crc_exec(aeth_crc *crc, const uint8_t *bits_dev, size_t L, size_t F, const uint64_t *state_in_dev, uint64_t *state_out_dev)
{
    AETH_REQUIRE(crc, AETH_E_ARG, "crc is null");
    const uint64_t n_in = mul_sat(L, F), n_st = mul_sat(F, 8);
    AETH_REQUIRE(n_in < kMaxLen, AETH_E_UNSUPPORTED, "%zu frames of %zu bits: the input reaches 2^32 bytes (cut the frames and carry the state)", F, L);
    AETH_REQUIRE(n_st < kMaxLen, AETH_E_UNSUPPORTED, "%zu frames: the states reach 2^32 bytes", F);
    if (F == 0) return AETH_OK;
    AETH_REQUIRE(state_out_dev && (bits_dev || !n_in), AETH_E_ARG, "null pointer");
    AETH_REQUIRE(aeth::aligned8(state_in_dev) && aeth::aligned8(state_out_dev), AETH_E_ALIGN, "state pointer not 8-byte aligned");
    if (int rc = aeth::check_disjoint({{bits_dev, n_in}, {state_in_dev, n_st}}, {{state_out_dev, n_st}}, "the output states overlap an input"))
        return rc;
    Plan pl{};
    pl.op = OP_EXEC; pl.in = bits_dev; pl.L = L; pl.F = F; pl.stride_in = L;
    pl.state_in = state_in_dev; pl.state_out = state_out_dev;
    return run(crc, pl);
}

int aeth_crc_attach(aeth_crc *crc, const uint8_t *in_dev, size_t L, size_t F, uint8_t *out_dev)
{
    AETH_REQUIRE(crc, AETH_E_ARG, "crc is null");
    const uint64_t n_in = mul_sat(L, F), n_out = L < kMaxLen ? mul_sat(L + crc->p.r, F) : UINT64_MAX;
    AETH_REQUIRE(L < kMaxLen && n_out < kMaxLen, AETH_E_UNSUPPORTED, "%zu frames of %zu + %u bits: the output reaches 2^32 bytes", F, L, crc->p.r);
    if (F == 0) return AETH_OK;
    AETH_REQUIRE(out_dev && (in_dev || !n_in), AETH_E_ARG, "null pointer");
    if (int rc = aeth::check_disjoint({{in_dev, n_in}}, {{out_dev, n_out}})) return rc;
    Plan pl{};
    pl.op = OP_ATTACH; pl.in = in_dev; pl.L = L; pl.F = F; pl.stride_in = L; pl.out = out_dev;
    return run(crc, pl);
}

int aeth_crc_check(aeth_crc *crc, const uint8_t *in_dev, size_t L, size_t F, uint64_t mask, uint64_t *diff_dev, uint8_t *payload_dev,
                   aeth_crc_summary *summary_dev)
{
    AETH_REQUIRE(crc, AETH_E_ARG, "crc is null");
    AETH_REQUIRE(mask <= cc::mask_of(crc->p.r), AETH_E_ARG, "mask 0x%llx at or above 2^%u", (unsigned long long)mask, crc->p.r);
    AETH_REQUIRE(diff_dev || payload_dev || summary_dev, AETH_E_ARG, "diff_dev, payload_dev and summary_dev are all null");
    const uint64_t n_in = L < kMaxLen ? mul_sat(L + crc->p.r, F) : UINT64_MAX, n_pay = mul_sat(L, F), n_diff = mul_sat(F, 8);
    AETH_REQUIRE(L < kMaxLen && n_in < kMaxLen, AETH_E_UNSUPPORTED, "%zu frames of %zu + %u bits: the input reaches 2^32 bytes", F, L, crc->p.r);
    AETH_REQUIRE(n_diff < kMaxLen, AETH_E_UNSUPPORTED, "%zu frames: the diff words reach 2^32 bytes", F);
    AETH_REQUIRE(in_dev || !F, AETH_E_ARG, "in_dev is null");
    AETH_REQUIRE(aeth::aligned8(diff_dev) && aeth::aligned8(summary_dev), AETH_E_ALIGN, "diff_dev or summary_dev not 8-byte aligned");
    if (int rc = aeth::check_disjoint({{in_dev, n_in}}, {{diff_dev, n_diff}, {payload_dev, n_pay}, {summary_dev, sizeof(aeth_crc_summary)}}))
        return rc;
    if (F == 0 && !summary_dev) return AETH_OK;
    Plan pl{};
    pl.op = OP_CHECK; pl.in = in_dev; pl.L = L; pl.F = F; pl.stride_in = L + crc->p.r;
    pl.out = payload_dev; pl.diff = diff_dev; pl.summary = reinterpret_cast<Rec *>(summary_dev); pl.mask = mask;
    return run(crc, pl);
}

int aeth_bits_pack(aeth_ctx *ctx, const uint8_t *bits_dev, size_t nbits, int order, uint8_t *bytes_dev, size_t nbytes)
{
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    AETH_REQUIRE(order == AETH_BITS_LSB_FIRST || order == AETH_BITS_MSB_FIRST, AETH_E_ARG, "unknown bit order %d", order);
    AETH_REQUIRE(nbytes == nbits / 8 + (nbits % 8 != 0), AETH_E_LEN, "%zu bits pack into %zu bytes, not %zu", nbits, nbits / 8 + (nbits % 8 != 0), nbytes);
    AETH_REQUIRE((uint64_t)nbits < kMaxLen, AETH_E_UNSUPPORTED, "nbits %zu: 2^32 or more in one call (cut at a multiple of 8)", nbits);
    if (nbits == 0) return AETH_OK;
    AETH_REQUIRE(bits_dev && bytes_dev, AETH_E_ARG, "null pointer");
    if (int rc = aeth::check_disjoint({{bits_dev, nbits}}, {{bytes_dev, nbytes}})) return rc;
    aeth::DeviceGuard dg(ctx->device);
    const bool nt = aeth::streams_past_cache(nbits + nbytes);
    hipStream_t st = aeth::ctx_stream(ctx);
    const uint64_t blocks = ((nbits + 15) / 16 + kBlock - 1) / kBlock;
    const dim3 grid((unsigned)std::min<uint64_t>(blocks, (uint64_t)std::max(ctx->num_cus, 1) * 16)), block(kBlock);
    const int msb = order == AETH_BITS_MSB_FIRST;
    if (nt) hipLaunchKernelGGL(bits_pack_kernel<true>, grid, block, 0, st, bits_dev, (uint64_t)nbits, msb, bytes_dev, (uint64_t)nbytes);
    else hipLaunchKernelGGL(bits_pack_kernel<false>, grid, block, 0, st, bits_dev, (uint64_t)nbits, msb, bytes_dev, (uint64_t)nbytes);
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

int aeth_bits_unpack(aeth_ctx *ctx, const uint8_t *bytes_dev, size_t nbytes, int order, uint8_t *bits_dev, size_t nbits)
{
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    AETH_REQUIRE(order == AETH_BITS_LSB_FIRST || order == AETH_BITS_MSB_FIRST, AETH_E_ARG, "unknown bit order %d", order);
    AETH_REQUIRE(nbits / 8 + (nbits % 8 != 0) <= nbytes, AETH_E_LEN, "%zu bits need %zu bytes, the input holds %zu", nbits, nbits / 8 + (nbits % 8 != 0), nbytes);
    AETH_REQUIRE((uint64_t)nbits < kMaxLen, AETH_E_UNSUPPORTED, "nbits %zu: 2^32 or more in one call (cut at a multiple of 8)", nbits);
    if (nbits == 0) return AETH_OK;
    AETH_REQUIRE(bits_dev && bytes_dev, AETH_E_ARG, "null pointer");
    if (int rc = aeth::check_disjoint({{bytes_dev, nbytes}}, {{bits_dev, nbits}})) return rc;
    aeth::DeviceGuard dg(ctx->device);
    const bool nt = aeth::streams_past_cache(nbits + nbytes);
    hipStream_t st = aeth::ctx_stream(ctx);
    const uint64_t blocks = ((nbits + 15 + 15) / 16 + kBlock - 1) / kBlock;
    const dim3 grid((unsigned)std::min<uint64_t>(blocks, (uint64_t)std::max(ctx->num_cus, 1) * 16)), block(kBlock);
    const int msb = order == AETH_BITS_MSB_FIRST;
    if (nt) hipLaunchKernelGGL(bits_unpack_kernel<true>, grid, block, 0, st, bytes_dev, (uint64_t)((nbits + 7) / 8), msb, bits_dev, (uint64_t)nbits);
    else hipLaunchKernelGGL(bits_unpack_kernel<false>, grid, block, 0, st, bytes_dev, (uint64_t)((nbits + 7) / 8), msb, bits_dev, (uint64_t)nbits);
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

}  // extern "C"
