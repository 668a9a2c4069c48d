// aeth_polar.hip -- polar codes: the encoder and a successive-cancellation decoder with one bit flip per codeword and a
// record of the four least reliable decisions (no body in the reference; definition in include/aether_hip.h,
// aeth_polar_*).  Everything is integer and defined byte for byte; compiled with the EXACT flags like the other
// bit-exact kernels.
//
// Decoder.  T lanes share a codeword (T = 4, 8, 16: a template parameter, chosen at create from n) and a workgroup is
// one wave of 64 / T codewords, so nothing waits at a workgroup barrier: a codeword's lanes run in lockstep and order
// their LDS traffic with a wave-level fence.  The mask is the same for every codeword, so the host lays the tree walk
// out as a schedule of words (aeth_polar_core.h): kF and kG make a child's values, kJoin folds the children's bits,
// kZero stands for a wholly frozen subtree.  The word is read with a uniform index through the constant address space,
// so it comes by a scalar load and every branch on it is uniform.
//   - Levels of more than T values live in LDS as int16 (a level of 2^k values lies k <= 7 levels below the channel
//     here, so |v| <= 128 * 2^7), lane j taking values j, j + T, ...; the top level's kF and kG read the int8 channel
//     values from memory, twice in all.  A codeword's state is padded so that the wave's codewords start 2 T bytes apart
//     modulo 128: the lanes of a half wave then fall on distinct banks.
//   - A child of T values is decided in registers right behind the kF / kG that made it: dec_reg<S> is the recursion of
//     the header unrolled at compile time on values replicated over the lanes (lane j of the codeword holds value
//     j mod S), so f and g take one cross-lane move (DPP for distances 1, 2 and 8, a swizzle for 4) and the bits need
//     none.  A frozen subtree inside it is skipped by a uniform branch on the word's mask bits.
//   - Partial sums are packed bits in LDS, N per codeword, folded in place; the decisions u are a second packed array.
//   - The candidate list is four ordered keys |L| << 10 | i per lane; an information leaf inserts with four min / max.
//
// Encoder.  A wave takes a tile of 64 words of 64 coded bits: lane l gathers bit 64 t + l of word t through the
// position table, a ballot packs the word, stages s < 6 run inside it on the scalar unit (w ^= (w >> 2^s) & M_s), lane t
// keeps word t, stages s >= 6 exchange whole words across lanes, and the words are unpacked to bytes.  Codewords of
// N < 64 bits lie side by side in a word.  No LDS.
//
// List decoder (aeth_polar_list_*).  The SC decoder's frame with L paths per codeword: T lanes per path,
// T L <= 64 lanes per codeword, one wave of 64 / (T L) codewords per workgroup, wave-level fences only.  The paths walk one
// schedule in lockstep, each in the LDS slot of its list position; an information leaf ranks the 2 L candidates by counting
// and moves registers and packed bits to the survivors' positions, never a level.  The pick is a copy that chooses its
// source row by the CRC words.
#include "aeth_polar_core.h"

#include <new>
#include <vector>

namespace {

namespace pc = aeth::polar;

constexpr int kWave = 64;
constexpr int kEncBlock = 256;
constexpr uint32_t kTileBits = 64 * 64;                // coded bits an encoder wave takes

typedef const uint32_t __attribute__((address_space(4))) *ConstTab;
__device__ __forceinline__ ConstTab const_tab(const uint32_t *p) { return (ConstTab)(uintptr_t)p; }

struct DecCall {
    const int8_t *soft;
    const uint32_t *flip;               // or null
    uint8_t *bits;
    aeth_polar_record *rec;             // or null
    const uint32_t *sched;
    const uint16_t *info;               // [K] the information positions, ascending
    uint64_t F;
    uint32_t n, K, nsched, stride;      // stride: bytes of LDS per codeword
    uint32_t codeword;
};

struct Pass {                           // what a codeword's lanes carry through the walk (the same in all of them)
    uint32_t flip, u;                   // u: the decisions of the subtree in registers, bit per leaf
    uint32_t k0, k1, k2, k3;            // candidate keys, ascending
    bool rec;
};

__device__ __forceinline__ int32_t f_of(int32_t a, int32_t b)
{
    const int32_t m = min(abs(a), abs(b));
    return (a ^ b) < 0 ? -m : m;
}

// the value of the lane D away (lane ^ D); D < 16 and a power of two
template <int D> __device__ __forceinline__ int32_t across(int32_t v)
{
    if constexpr (D == 1) return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);       // quad_perm [1, 0, 3, 2]
    else if constexpr (D == 2) return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);  // quad_perm [2, 3, 0, 1]
    else if constexpr (D == 8) return __builtin_amdgcn_update_dpp(0, v, 0x128, 0xF, 0xF, false); // row_ror 8
    else return __builtin_amdgcn_ds_swizzle(v, (D << 10) | 0x1F);                                // xor D in groups of 32
}

// dec(L, base + OFF) of the header for S values held in registers: the lane holds L[j mod S] and gets bit j mod S of the result
template <int S, int OFF> __device__ __forceinline__ uint32_t dec_reg(int32_t v, uint32_t info, uint32_t base, uint32_t j, Pass &p)
{
    if (((info >> OFF) & ((1u << S) - 1u)) == 0) return 0;                // frozen throughout: uniform
    if constexpr (S == 1) {
        const uint32_t i = base + OFF;
        const uint32_t u = (uint32_t)(v < 0) ^ (uint32_t)(i == p.flip);
        p.u |= u << OFF;
        if (p.rec) {
            uint32_t key = ((uint32_t)abs(v) << 10) | i, t;
            t = min(p.k0, key); key = max(p.k0, key); p.k0 = t;
            t = min(p.k1, key); key = max(p.k1, key); p.k1 = t;
            t = min(p.k2, key); key = max(p.k2, key); p.k2 = t;
            p.k3 = min(p.k3, key);
        }
        return u;
    } else {
        constexpr int H = S / 2;
        const int32_t o = across<H>(v);
        const bool hi = (j & H) != 0;
        const int32_t a = hi ? o : v, b = hi ? v : o;
        const uint32_t x1 = dec_reg<H, OFF>(f_of(a, b), info, base, j, p);
        const uint32_t x2 = dec_reg<H, OFF + H>(x1 ? b - a : b + a, info, base, j, p);
        return hi ? x2 : x1 ^ x2;
    }
}

// the lanes of a codeword have written LDS that the others read next
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int T> __global__ __launch_bounds__(kWave) void polar_decode_kernel(DecCall a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char polar_lds[];
    constexpr uint32_t G = kWave / T, TMASK = (1u << T) - 1u;
    const uint32_t lane = threadIdx.x, g = lane / T, j = lane % T;
    const uint32_t N = 1u << a.n;
    const uint64_t cw = (uint64_t)blockIdx.x * G + g;
    const bool real = cw < a.F;
    const uint64_t src = real ? cw : a.F - 1;                             // idle lanes walk along on the call's last codeword
    const int8_t *soft = a.soft + src * N;
    const ConstTab sched = const_tab(a.sched);

    // the codeword's state: levels of 2 T, 4 T, ... N / 2 values (the level of m values at m - 2 T), x bits, u bits
    unsigned char *st = polar_lds + (size_t)g * a.stride;
    int16_t *L = reinterpret_cast<int16_t *>(st);
    uint32_t *X = reinterpret_cast<uint32_t *>(st + 2u * (N - 2u * T));
    uint32_t *U = X + (N > 32 ? N / 32 : 1);

    Pass p;
    p.flip = a.flip ? a.flip[src] : AETH_POLAR_NONE;
    p.k0 = p.k1 = p.k2 = p.k3 = 0xFFFFFFFFu;
    p.rec = a.rec != nullptr;
    p.u = 0;

    for (uint32_t s = 0; s < a.nsched; s++) {
        const uint32_t w = sched[s];
        const uint32_t op = w & 3u, lg = (w >> 2) & 15u, base = (w >> 6) & 1023u;
        const uint32_t m = 1u << lg, h = m >> 1;
        if (op == pc::kF || op == pc::kG) {
            const bool top = lg == a.n, right = op == pc::kG;
            const int16_t *in = L + (m - 2u * T);                         // not followed at the top level
            if (h > (uint32_t)T) {
                int16_t *out = L + (h - 2u * T);
                if (!right) {
                    if (top) for (uint32_t k = j; k < h; k += T) out[k] = (int16_t)f_of(soft[k], soft[k + h]);
                    else for (uint32_t k = j; k < h; k += T) out[k] = (int16_t)f_of(in[k], in[k + h]);
                } else {
                    for (uint32_t k = j; k < h; k += T) {
                        const int32_t va = top ? (int32_t)soft[k] : (int32_t)in[k], vb = top ? (int32_t)soft[k + h] : (int32_t)in[k + h];
                        const uint32_t x = (X[(base + k) >> 5] >> ((base + k) & 31u)) & 1u;
                        out[k] = (int16_t)(x ? vb - va : vb + va);
                    }
                }
            } else {                                                      // h == T: into registers, and decide the child
                const int32_t va = top ? (int32_t)soft[j] : (int32_t)in[j], vb = top ? (int32_t)soft[j + h] : (int32_t)in[j + h];
                int32_t v;
                if (!right) v = f_of(va, vb);
                else v = ((X[(base + j) >> 5] >> ((base + j) & 31u)) & 1u) ? vb - va : vb + va;
                const uint32_t cb = right ? base + h : base;
                p.u = 0;
                const uint32_t x = dec_reg<T, 0>(v, w >> 16, cb, j, p);
                const uint32_t xb = (uint32_t)(__ballot(x != 0) >> (lane & ~(uint32_t)(T - 1))) & TMASK;
                if (j == 0) {
                    const uint32_t wi = cb >> 5, sh = cb & 31u;
                    X[wi] = (X[wi] & ~(TMASK << sh)) | (xb << sh);
                    U[wi] = (U[wi] & ~(TMASK << sh)) | (p.u << sh);
                }
            }
        } else if (h >= 32 || (op == pc::kZero && m >= 32)) {             // whole words of bits
            if (op == pc::kJoin) for (uint32_t k = j; k < h / 32; k += T) X[base / 32 + k] ^= X[(base + h) / 32 + k];
            else for (uint32_t k = j; k < m / 32; k += T) X[base / 32 + k] = 0;
        } else if (j == 0) {                                              // inside one word
            const uint32_t wi = base >> 5, sh = base & 31u, x = X[wi];
            if (op == pc::kJoin) X[wi] = x ^ ((x >> h) & (((1u << h) - 1u) << sh));
            else X[wi] = x & ~(((1u << m) - 1u) << sh);
        }
        wave_sync();
    }

    if (!real) return;
    if (a.codeword) {
        uint8_t *dst = a.bits + cw * N;
        for (uint32_t k = j; k < N; k += T) dst[k] = (uint8_t)((X[k >> 5] >> (k & 31u)) & 1u);
    } else {
        uint8_t *dst = a.bits + cw * a.K;
        for (uint32_t r = j; r < a.K; r += T) {
            const uint32_t i = a.info[r];
            dst[r] = (uint8_t)((U[i >> 5] >> (i & 31u)) & 1u);
        }
    }
    if (a.rec && j == 0) {
        const uint32_t k[4] = {p.k0, p.k1, p.k2, p.k3};
        aeth_polar_record r;
        for (int q = 0; q < 4; q++) {
            const bool none = k[q] == 0xFFFFFFFFu;
            r.index[q] = none ? 0xFFFFFFFFu : k[q] & 1023u;
            r.abs[q] = none ? 0xFFFFFFFFu : k[q] >> 10;
        }
        a.rec[cw] = r;
    }
}

// ---- the list decoder ----
struct ListCall {
    const int8_t *soft;
    uint8_t *bits;
    aeth_polar_list_record *rec;        // or null
    const uint32_t *sched;
    const uint16_t *info;               // [K] the information positions, ascending
    uint64_t F;
    uint32_t n, K, nsched, stride;      // stride: bytes of LDS per path
    uint32_t codeword, all;
};

constexpr int lg2(int v) { return v <= 1 ? 0 : 1 + lg2(v / 2); }

__device__ __forceinline__ uint32_t from_lane(uint32_t v, uint32_t lane) { return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(lane << 2), (int)v); }

// the sum of s over the T lanes of a path, in all of them
template <int T> __device__ __forceinline__ int32_t path_sum(int32_t s)
{
    s += across<1>(s);
    s += across<2>(s);
    if constexpr (T > 4) s += across<4>(s);
    if constexpr (T > 8) s += across<8>(s);
    return s;
}

// What the T lanes of a path carry: the levels of T, T / 2, ... 1 values of the subtree in registers (v[d]: 2^d values, lane
// j holding value j mod 2^d), the finished left children's bits of those levels packed into xs (level d: 2^d bits from bit
// 2^d - 1), the slot each LDS level of this path was written to (srcs: three bits per level, level 2^lg at bit 3 lg), and the
// metric.  xs, srcs and pm are the same in all lanes of the path.
template <int T> struct Path {
    int32_t v[lg2(T) + 1];
    uint32_t xs, srcs, pm;
};

struct Where {                          // a lane's place
    uint32_t q, j, lane0;               // the path's list position, the lane in the path, the codeword's first lane
    unsigned char *cw;                  // the state of the codeword's path 0
    uint32_t *sel;                      // [L] the codeword's survivors
    uint32_t stride, xoff;              // bytes per path, and from a path's state to its x bits
};

template <int D, int T> __device__ __forceinline__ void f_down(Path<T> &p)                       // v[D - 1] .. v[0] from v[D]
{
    if constexpr (D > 0) {
        p.v[D - 1] = f_of(p.v[D], across<(1 << (D - 1))>(p.v[D]));
        f_down<D - 1, T>(p);
    }
}

template <int t, int D, int T> __device__ __forceinline__ void move_levels(Path<T> &p, uint32_t lane)   // those a later leaf reads
{
    if constexpr (D <= lg2(T)) {
        if constexpr (((t >> (D - 1)) & 1) == 0) p.v[D] = (int32_t)from_lane((uint32_t)p.v[D], lane);
        move_levels<t, D + 1, T>(p, lane);
    }
}

// leaf t of the subtree has decided x (2^D bits by now): fold it with the finished left children; the subtree's bits at t = T - 1
template <int t, int D, int T> __device__ __forceinline__ uint32_t fold(Path<T> &p, uint32_t x)
{
    constexpr uint32_t w = 1u << D, off = w - 1u, mask = (1u << w) - 1u;
    if constexpr ((t >> D) & 1) return fold<t, D + 1, T>(p, (((p.xs >> off) & mask) ^ x) | (x << w));
    else if constexpr (D < lg2(T)) {
        p.xs = (p.xs & ~(mask << off)) | (x << off);
        return 0;
    } else return x;
}

// An information leaf (header: candidates, sort, survivors).  A of the L positions are active; the new position r takes
// the candidate of rank r: its bit, its metric, and its parent's registers and x bits.  Returns the leaf's bit.
template <int T, int L, int t> __device__ __forceinline__ uint32_t fork(Path<T> &p, int32_t lam, uint32_t &A, uint32_t leaf, const Where &at)
{
    if constexpr (L == 1) return (uint32_t)(lam < 0);
    else {
        const bool neg = lam < 0, active = at.q < A;
        const uint32_t mag = (uint32_t)abs(lam);
        const uint32_t k0 = active ? (p.pm + (neg ? mag : 0u)) * (2u * L) + 2u * at.q : 0xFFFFFFFFu;
        const uint32_t k1 = active ? (p.pm + (neg ? 0u : mag)) * (2u * L) + 2u * at.q + 1u : 0xFFFFFFFFu;
        uint32_t r0 = 0, r1 = 0;
#pragma unroll
        for (uint32_t o = 0; o < (uint32_t)L; o++) {
            const uint32_t o0 = from_lane(k0, at.lane0 + o * T), o1 = from_lane(k1, at.lane0 + o * T);
            r0 += (uint32_t)(o0 < k0) + (uint32_t)(o1 < k0);
            r1 += (uint32_t)(o0 < k1) + (uint32_t)(o1 < k1);
        }
        A = min(2u * A, (uint32_t)L);
        if (at.j == 0 && active) {
            if (r0 < A) at.sel[r0] = k0;
            if (r1 < A) at.sel[r1] = k1;
        }
        wave_sync();
        uint32_t par = at.q, bit = 0;
        if (at.q < A) {
            const uint32_t key = at.sel[at.q];
            par = (key >> 1) & (uint32_t)(L - 1);
            bit = key & 1u;
            p.pm = key / (2u * L);
        }
        const uint32_t lane = at.lane0 + par * T + at.j;
        move_levels<t, 1, T>(p, lane);
        p.xs = from_lane(p.xs, lane);
        p.srcs = from_lane(p.srcs, lane);
        if (__any(par != at.q)) {                                         // the x bits decided so far: words 0 .. leaf / 32
            constexpr uint32_t W = 32 / T;
            const uint32_t *from = reinterpret_cast<const uint32_t *>(at.cw + (size_t)par * at.stride + at.xoff);
            uint32_t *to = reinterpret_cast<uint32_t *>(at.cw + (size_t)at.q * at.stride + at.xoff);
            const uint32_t last = leaf >> 5;
            uint32_t tmp[W];
#pragma unroll
            for (uint32_t c = 0; c < W; c++) tmp[c] = at.j + c * T <= last ? from[at.j + c * T] : 0u;
            wave_sync();
#pragma unroll
            for (uint32_t c = 0; c < W; c++)
                if (at.j + c * T <= last) to[at.j + c * T] = tmp[c];
            wave_sync();
        }
        return bit;
    }
}

// leaves t .. T - 1 of the subtree in registers whose first leaf is `base`; returns the subtree's T bits
template <int T, int L, int t> __device__ __forceinline__ uint32_t walk(Path<T> &p, uint32_t info, uint32_t base, uint32_t &A, const Where &at)
{
    constexpr int LGT = lg2(T), s = t == 0 ? LGT : __builtin_ctz(t | (1 << LGT));
    if constexpr (s < LGT) {                                              // g of the node of 2^(s+1) values, by its left child's bits
        constexpr uint32_t h = 1u << s;
        const int32_t own = p.v[s + 1], o = across<(int)h>(own);
        const bool hi = (at.j & h) != 0;
        const int32_t a = hi ? o : own, b = hi ? own : o;
        p.v[s] = ((p.xs >> ((h - 1u) + (at.j & (h - 1u)))) & 1u) ? b - a : b + a;
    }
    f_down<s, T>(p);
    const int32_t lam = p.v[0];
    uint32_t bit = 0;
    if ((info >> t) & 1u) bit = fork<T, L, t>(p, lam, A, base + t, at);   // uniform
    else p.pm += lam < 0 ? (uint32_t)(-lam) : 0u;
    const uint32_t x = fold<t, 0, T>(p, bit);
    if constexpr (t + 1 < T) return walk<T, L, t + 1>(p, info, base, A, at);
    else return x;
}

// T lanes per path, L paths per codeword, 64 / (T L) codewords per wave.  The paths walk the schedule in lockstep, each in
// the slot of its list position: a level is written into the path's own slot and found again through srcs, so that a fork
// moves registers and the x bits only.
template <int T, int L> __global__ __launch_bounds__(kWave) void polar_list_kernel(ListCall a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char polar_lds[];
    static_assert(T * L <= kWave, "a codeword never leaves its wave");
    constexpr uint32_t G = kWave / (T * L), S = kWave / T, TMASK = (1u << T) - 1u, LGT = lg2(T);
    const uint32_t lane = threadIdx.x, slot = lane / T, g = slot / L;
    const uint32_t N = 1u << a.n;
    const uint64_t cw = (uint64_t)blockIdx.x * G + g;
    const bool real = cw < a.F;
    const uint64_t src = real ? cw : a.F - 1;                             // idle lanes walk along on the call's last codeword
    const int8_t *soft = a.soft + src * N;
    const ConstTab sched = const_tab(a.sched);

    // a path's state: levels of 2 T, 4 T, ... N / 2 values (the level of m values at m - 2 T), x bits; the survivors behind all
    Where at;
    at.q = slot % L; at.j = lane % T; at.lane0 = g * L * T;
    at.stride = a.stride; at.xoff = 2u * (N - 2u * T);
    at.cw = polar_lds + (size_t)(g * L) * a.stride;
    at.sel = reinterpret_cast<uint32_t *>(polar_lds + (size_t)S * a.stride) + g * L;
    const uint32_t j = at.j, q = at.q;
    int16_t *Lv = reinterpret_cast<int16_t *>(at.cw + (size_t)q * a.stride);
    uint32_t *X = reinterpret_cast<uint32_t *>(at.cw + (size_t)q * a.stride + at.xoff);

    Path<T> p;
#pragma unroll
    for (uint32_t d = 0; d <= LGT; d++) p.v[d] = 0;
    p.xs = 0; p.pm = 0;
    p.srcs = q * 0x09249249u;                                             // every level in the path's own slot
    uint32_t A = 1;

    for (uint32_t s = 0; s < a.nsched; s++) {
        const uint32_t w = sched[s];
        const uint32_t op = w & 3u, lg = (w >> 2) & 15u, base = (w >> 6) & 1023u, info = w >> 16;
        const uint32_t m = 1u << lg, h = m >> 1;
        if (op == pc::kF || op == pc::kG) {
            const bool top = lg == a.n, right = op == pc::kG;
            const uint32_t cb = right ? base + h : base;
            const int16_t *in = reinterpret_cast<const int16_t *>(at.cw + (size_t)((p.srcs >> (3u * lg)) & 7u) * a.stride) + (m - 2u * T);   // not followed at the top level
            if (h > (uint32_t)T) {
                int16_t *out = Lv + (h - 2u * T);
                int32_t pen = 0;
                for (uint32_t k = j; k < h; k += T) {
                    const int32_t va = top ? (int32_t)soft[k] : (int32_t)in[k], vb = top ? (int32_t)soft[k + h] : (int32_t)in[k + h];
                    int32_t v;
                    if (!right) v = f_of(va, vb);
                    else v = ((X[(base + k) >> 5] >> ((base + k) & 31u)) & 1u) ? vb - va : vb + va;
                    if (info) out[k] = (int16_t)v;
                    else pen += v < 0 ? -v : 0;
                }
                if (info) p.srcs = (p.srcs & ~(7u << (3u * (lg - 1u)))) | (q << (3u * (lg - 1u)));
                else {                                                    // wholly frozen: its values' share of the metric, zero bits
                    p.pm += (uint32_t)path_sum<T>(pen);
                    if (h >= 32) for (uint32_t k = j; k < h / 32; k += T) X[cb / 32 + k] = 0;
                    else if (j == 0) X[cb >> 5] &= ~(((1u << h) - 1u) << (cb & 31u));
                }
            } else {                                                      // h == T: into registers, and walk the child's leaves
                const int32_t va = top ? (int32_t)soft[j] : (int32_t)in[j], vb = top ? (int32_t)soft[j + h] : (int32_t)in[j + h];
                int32_t v;
                if (!right) v = f_of(va, vb);
                else v = ((X[(base + j) >> 5] >> ((base + j) & 31u)) & 1u) ? vb - va : vb + va;
                uint32_t xb = 0;
                if (info) {
                    p.v[LGT] = v;
                    xb = walk<T, L, 0>(p, info, cb, A, at);
                } else p.pm += (uint32_t)path_sum<T>(v < 0 ? -v : 0);
                if (j == 0) {
                    const uint32_t wi = cb >> 5, sh = cb & 31u;
                    X[wi] = (X[wi] & ~(TMASK << sh)) | (xb << sh);
                }
            }
        } else if (h >= 32) {                                             // kJoin on whole words of bits
            for (uint32_t k = j; k < h / 32; k += T) X[base / 32 + k] ^= X[(base + h) / 32 + k];
        } else if (j == 0) {                                              // inside one word
            const uint32_t wi = base >> 5, sh = base & 31u, x = X[wi];
            X[wi] = x ^ ((x >> h) & (((1u << h) - 1u) << sh));
        }
        wave_sync();
    }

    // the final order: by (metric, position); all L positions are active, since the code has at least L words
    uint32_t row = 0;
    if constexpr (L > 1) {
        const uint32_t key = p.pm * L + q;
#pragma unroll
        for (uint32_t o = 0; o < (uint32_t)L; o++) row += (uint32_t)(from_lane(key, at.lane0 + o * T) < key);
    }
    const bool wanted = real && (a.all || row == 0);
    const uint64_t dst_row = a.all ? cw * L + row : cw;
    if (a.rec && real && j == 0) {
        uint32_t *metric = a.rec[cw].metric;
        metric[row] = p.pm;
        if (row == 0) for (uint32_t r = L; r < 8; r++) metric[r] = 0xFFFFFFFFu;
    }
    if (a.codeword) {
        if (!wanted) return;
        uint8_t *dst = a.bits + dst_row * N;
        for (uint32_t k = j; k < N; k += T) dst[k] = (uint8_t)((X[k >> 5] >> (k & 31u)) & 1u);
        return;
    }
    // the decisions: u = transform(x^), on the packed words in place
    const uint32_t words = N > 32 ? N / 32 : 1;
    for (uint32_t k = j; k < words; k += T) {
        uint32_t x = X[k];
        x ^= (x >> 1) & 0x55555555u;
        x ^= (x >> 2) & 0x33333333u;
        x ^= (x >> 4) & 0x0F0F0F0Fu;
        if (a.n > 3) x ^= (x >> 8) & 0x00FF00FFu;
        if (a.n > 4) x ^= (x >> 16) & 0x0000FFFFu;
        X[k] = x;
    }
    wave_sync();
    for (uint32_t d = 1; d < words; d <<= 1) {
        for (uint32_t k = j; k < words; k += T)
            if (!(k & d)) X[k] ^= X[k + d];
        wave_sync();
    }
    if (!wanted) return;
    uint8_t *dst = a.bits + dst_row * a.K;
    for (uint32_t r = j; r < a.K; r += T) {
        const uint32_t i = a.info[r];
        dst[r] = (uint8_t)((X[i >> 5] >> (i & 31u)) & 1u);
    }
}

// ---- the pick: per codeword the first of its L rows whose CRC word is zero ----
constexpr uint32_t kPickBlock = 256, kPickBytes = 16 * kPickBlock;       // output bytes a workgroup takes

struct PickCall {
    const uint8_t *rows;
    const uint64_t *diff;
    uint8_t *out;
    uint32_t *which;                    // or null
    uint64_t total;                     // output bytes of the call
    uint32_t row_bytes, L;
};

__global__ __launch_bounds__(kPickBlock) void polar_pick_kernel(PickCall a)
{
    __shared__ uint8_t row_of[kPickBytes + 2];                            // the row taken, for the codewords this workgroup touches
    const uint64_t start = (uint64_t)blockIdx.x * kPickBytes;
    const uint64_t end = min(start + kPickBytes, a.total);
    const uint64_t f0 = start / a.row_bytes, f1 = (end - 1) / a.row_bytes;
    const uint32_t nf = (uint32_t)(f1 - f0) + 1u;                         // <= kPickBytes + 1
    for (uint32_t i = threadIdx.x; i < nf; i += kPickBlock) {
        const uint64_t f = f0 + i;
        uint32_t r = AETH_POLAR_NONE;
        for (uint32_t k = a.L; k-- > 0;)
            if (a.diff[f * a.L + k] == 0) r = k;
        row_of[i] = r == AETH_POLAR_NONE ? (uint8_t)0 : (uint8_t)r;
        if (a.which && f * a.row_bytes >= start) a.which[f] = r;          // the workgroup that holds the row's first byte
    }
    __syncthreads();
    const uint32_t c0 = (uint32_t)(start - f0 * a.row_bytes);             // < row_bytes
    for (uint32_t o = threadIdx.x; o < kPickBytes && start + o < end; o += kPickBlock) {
        const uint32_t rel = c0 + o, i = rel / a.row_bytes, c = rel - i * a.row_bytes;
        a.out[start + o] = a.rows[((f0 + i) * a.L + row_of[i]) * a.row_bytes + c];
    }
}

struct EncCall {
    const uint8_t *in;
    uint8_t *out;
    const uint16_t *tab;                // [N] rank among the information positions, 0xffff where frozen
    uint64_t total;                     // coded bits of the call
    uint32_t n, K;
};

__global__ __launch_bounds__(kEncBlock) void polar_encode_kernel(EncCall a)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t p0 = ((uint64_t)blockIdx.x * (kEncBlock / kWave) + wave) * kTileBits;
    if (p0 >= a.total) return;                                            // the whole wave
    const uint32_t N = 1u << a.n;
    unsigned long long mine = 0;
    for (uint32_t t = 0; t < 64; t++) {
        const uint64_t p = p0 + t * 64u + lane;
        uint32_t bit = 0;
        if (p < a.total) {
            const uint32_t r = a.tab[(uint32_t)p & (N - 1u)];
            if (r != 0xffffu) bit = a.in[(p >> a.n) * a.K + r] & 1u;
        }
        unsigned long long w = __ballot(bit != 0);
        w ^= (w >> 1) & 0x5555555555555555ull;
        w ^= (w >> 2) & 0x3333333333333333ull;
        w ^= (w >> 4) & 0x0F0F0F0F0F0F0F0Full;
        if (a.n > 3) w ^= (w >> 8) & 0x00FF00FF00FF00FFull;
        if (a.n > 4) w ^= (w >> 16) & 0x0000FFFF0000FFFFull;
        if (a.n > 5) w ^= (w >> 32) & 0x00000000FFFFFFFFull;
        if (lane == t) mine = w;
    }
    for (uint32_t s = 6; s < a.n; s++) {                                  // word t ^= word t + d of the same codeword
        const uint32_t d = 1u << (s - 6);
        const unsigned long long o = __shfl_xor(mine, (int)d);
        if (!(lane & d)) mine ^= o;
    }
    for (uint32_t t = 0; t < 64; t++) {
        const unsigned long long w = __shfl(mine, (int)t);
        const uint64_t p = p0 + t * 64u + lane;
        if (p < a.total) a.out[p] = (uint8_t)((w >> lane) & 1u);
    }
}

// lanes per codeword, as measured: few lanes waste the fewest lane-steps and win while a codeword's walk
// is short; from n = 9 on the walk is long and the state large, so that more lanes per codeword (a shorter serial path,
// more waves on the LDS) win although they idle more.  T <= N / 2: the top level's f feeds at least the subtree in
// registers.  AETH_POLAR_LANES (lab build only) forces a value for tools/polar_bw.py.
uint32_t lanes_of(uint32_t n)
{
    const uint32_t forced = (uint32_t)aeth::lab_int("AETH_POLAR_LANES", 0);
    uint32_t T = forced ? forced : (n <= 6 ? 4u : n <= 8 ? 8u : 16u);
    while (T > 4 && 2 * T > (1u << n)) T >>= 1;
    return T == 4 || T == 8 || T == 16 ? T : 8u;
}

// bytes of LDS per codeword: the levels, x and u, padded to 2 T modulo 128
uint32_t stride_of(uint32_t n, uint32_t T)
{
    const uint32_t N = 1u << n, words = N > 32 ? N / 32 : 1;
    const uint32_t raw = 2 * (N - 2 * T) + 8 * words;
    return raw + ((2 * T + 128 - raw % 128) % 128);
}

}  // namespace

struct aeth_polar {
    aeth_ctx *ctx;
    uint32_t n, N, K, T, G, stride, nsched;
    uint32_t *sched_dev;                // [nsched]
    uint16_t *pos_dev;                  // [N] the encoder's table, then [K] the information positions
};

struct aeth_polar_list {
    aeth_ctx *ctx;
    uint32_t n, N, K, L, T, G, stride, nsched;
    uint32_t *sched_dev;                // [nsched]
    uint16_t *info_dev;                 // [K] the information positions, ascending
};

extern "C" {

int aeth_polar_rank(uint32_t n, uint32_t *order_out, size_t count)
{
    const int rc = pc::check_n(n);
    if (rc) return rc;
    AETH_REQUIRE(count >= ((size_t)1 << n), AETH_E_LEN, "the order of n = %u has %u positions, order_out holds %zu", n, 1u << n, count);
    AETH_REQUIRE(order_out, AETH_E_ARG, "order_out is null");
    std::vector<uint32_t> order;
    pc::rank(n, order);
    std::copy(order.begin(), order.end(), order_out);
    return AETH_OK;
}

int aeth_polar_mask(uint32_t n, uint32_t K, uint8_t *mask_out, size_t count)
{
    const int rc = pc::check_n(n);
    if (rc) return rc;
    const uint32_t N = 1u << n;
    AETH_REQUIRE(K >= 1 && K <= N, AETH_E_ARG, "K = %u outside 1 .. %u", K, N);
    AETH_REQUIRE(count >= N, AETH_E_LEN, "the mask of n = %u has %u bytes, mask_out holds %zu", n, N, count);
    AETH_REQUIRE(mask_out, AETH_E_ARG, "mask_out is null");
    std::vector<uint32_t> order;
    pc::rank(n, order);
    std::fill(mask_out, mask_out + N, (uint8_t)0);
    for (uint32_t r = 0; r < K; r++) mask_out[order[r]] = 1;
    return AETH_OK;
}

int aeth_polar_create(aeth_ctx *ctx, uint32_t n, const uint8_t *mask, aeth_polar **out)
{
    AETH_REQUIRE(out, AETH_E_ARG, "out is null");
    *out = nullptr;
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    int rc = pc::check_n(n);
    if (rc) return rc;
    AETH_REQUIRE(mask, AETH_E_ARG, "mask is null");
    const uint32_t N = 1u << n;
    uint32_t K = 0;
    for (uint32_t i = 0; i < N; i++) {
        AETH_REQUIRE(mask[i] <= 1, AETH_E_ARG, "mask[%u] = %u: a mask byte is 0 (frozen) or 1 (information)", i, mask[i]);
        K += mask[i];
    }
    AETH_REQUIRE(K >= 1, AETH_E_ARG, "K = 0: the mask of n = %u holds no information position", n);
    aeth_polar *p = new (std::nothrow) aeth_polar{};
    AETH_REQUIRE(p, AETH_E_NOMEM, "out of host memory");
    p->ctx = ctx;
    p->n = n; p->N = N; p->K = K;
    p->T = lanes_of(n);
    p->G = kWave / p->T;
    p->stride = stride_of(n, p->T);
    std::vector<uint32_t> sched;
    pc::schedule(mask, p->T, 0, n, sched);
    p->nsched = (uint32_t)sched.size();
    std::vector<uint16_t> tab, info;
    pc::positions(mask, N, tab, info);
    tab.insert(tab.end(), info.begin(), info.end());
    rc = aeth::upload_table(ctx, sched.data(), sched.size() * sizeof(uint32_t), &p->sched_dev, "aeth_polar_create: schedule");
    if (!rc) rc = aeth::upload_table(ctx, tab.data(), tab.size() * sizeof(uint16_t), &p->pos_dev, "aeth_polar_create: position table");
    if (rc) {
        (void)aeth::release_tables(ctx, {p->sched_dev, p->pos_dev});
        delete p;
        return rc;
    }
    *out = p;
    return AETH_OK;
}

int aeth_polar_destroy(aeth_polar *p)
{
    if (!p) return AETH_OK;
    const hipError_t freed = aeth::release_tables(p->ctx, {p->sched_dev, p->pos_dev});
    delete p;
    return freed == hipSuccess ? AETH_OK : aeth::hip_fail(freed, "hipFree");
}

size_t aeth_polar_n(const aeth_polar *p) { return p ? p->N : 0; }
size_t aeth_polar_k(const aeth_polar *p) { return p ? p->K : 0; }
uint32_t aeth_polar_lanes(const aeth_polar *p) { return p ? p->T : 0; }
uint32_t aeth_polar_group(const aeth_polar *p) { return p ? p->G : 0; }
size_t aeth_polar_lds_bytes(const aeth_polar *p) { return p ? (size_t)p->G * p->stride : 0; }

int aeth_polar_encode(aeth_polar *p, const uint8_t *bits_dev, size_t nbits, uint8_t *coded_dev, size_t ncoded)
{
    AETH_REQUIRE(p, AETH_E_ARG, "polar is null");
    size_t F;
    if (int rc = aeth::check_codewords(false, nbits, p->K, ncoded, p->N, &F)) return rc;
    if (F == 0) return AETH_OK;
    AETH_REQUIRE(bits_dev && coded_dev, AETH_E_ARG, "null pointer");
    if (int rc = aeth::check_disjoint({{bits_dev, nbits}}, {{coded_dev, ncoded}})) return rc;
    const uint64_t tiles = ((uint64_t)ncoded + kTileBits - 1) / kTileBits;
    const uint64_t wgs = (tiles + kEncBlock / kWave - 1) / (kEncBlock / kWave);
    if (int rc = aeth::check_grid(wgs, F, "codewords")) return rc;
    aeth::DeviceGuard dg(p->ctx->device);
    hipStream_t st = aeth::ctx_stream(p->ctx);
    EncCall a{bits_dev, coded_dev, p->pos_dev, (uint64_t)ncoded, p->n, p->K};
    hipLaunchKernelGGL(polar_encode_kernel, dim3((unsigned)wgs), dim3(kEncBlock), 0, st, a);
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

int aeth_polar_decode(aeth_polar *p, const int8_t *soft_dev, size_t nsoft, const uint32_t *flip_dev, uint32_t flags, uint8_t *bits_dev,
                      size_t nbits, aeth_polar_record *rec_dev)
{
    AETH_REQUIRE(p, AETH_E_ARG, "polar is null");
    if (int rc = aeth::check_flags(flags, AETH_POLAR_CODEWORD)) return rc;
    size_t F;
    if (int rc = aeth::check_codewords(true, nsoft, p->N, nbits, (flags & AETH_POLAR_CODEWORD) ? p->N : p->K, &F)) return rc;
    if (F == 0) return AETH_OK;
    AETH_REQUIRE(soft_dev && bits_dev, AETH_E_ARG, "null pointer");
    AETH_REQUIRE(aeth::aligned4(flip_dev), AETH_E_ALIGN, "flip_dev not 4-byte aligned");
    AETH_REQUIRE(aeth::aligned4(rec_dev), AETH_E_ALIGN, "rec_dev not 4-byte aligned");
    const size_t nrec = F * sizeof(aeth_polar_record), nflip = F * sizeof(uint32_t);
    if (int rc = aeth::check_disjoint({{soft_dev, nsoft}, {flip_dev, nflip}}, {{bits_dev, nbits}, {rec_dev, nrec}})) return rc;
    const uint64_t wgs = (F + p->G - 1) / p->G;
    if (int rc = aeth::check_grid(wgs, F, "codewords")) return rc;
    aeth::DeviceGuard dg(p->ctx->device);
    hipStream_t st = aeth::ctx_stream(p->ctx);
    DecCall a{};
    a.soft = soft_dev; a.flip = flip_dev; a.bits = bits_dev; a.rec = rec_dev;
    a.sched = p->sched_dev; a.info = p->pos_dev + p->N;
    a.F = F;
    a.n = p->n; a.K = p->K; a.nsched = p->nsched; a.stride = p->stride;
    a.codeword = (flags & AETH_POLAR_CODEWORD) ? 1 : 0;
    const size_t lds = (size_t)p->G * p->stride;
    switch (p->T) {
    case 4: hipLaunchKernelGGL(polar_decode_kernel<4>, dim3((unsigned)wgs), dim3(kWave), lds, st, a); break;
    case 8: hipLaunchKernelGGL(polar_decode_kernel<8>, dim3((unsigned)wgs), dim3(kWave), lds, st, a); break;
    default: hipLaunchKernelGGL(polar_decode_kernel<16>, dim3((unsigned)wgs), dim3(kWave), lds, st, a); break;
    }
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

int aeth_polar_list_create(aeth_ctx *ctx, uint32_t n, const uint8_t *mask, uint32_t L, aeth_polar_list **out)
{
    AETH_REQUIRE(out, AETH_E_ARG, "out is null");
    *out = nullptr;
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    int rc = pc::check_n(n);
    if (rc) return rc;
    AETH_REQUIRE(mask, AETH_E_ARG, "mask is null");
    const uint32_t N = 1u << n;
    uint32_t K = 0;
    for (uint32_t i = 0; i < N; i++) {
        AETH_REQUIRE(mask[i] <= 1, AETH_E_ARG, "mask[%u] = %u: a mask byte is 0 (frozen) or 1 (information)", i, mask[i]);
        K += mask[i];
    }
    AETH_REQUIRE(K >= 1, AETH_E_ARG, "K = 0: the mask of n = %u holds no information position", n);
    if ((rc = pc::check_list(L, K))) return rc;
    aeth_polar_list *p = new (std::nothrow) aeth_polar_list{};
    AETH_REQUIRE(p, AETH_E_NOMEM, "out of host memory");
    p->ctx = ctx;
    p->n = n; p->N = N; p->K = K; p->L = L;
    p->T = pc::list_lanes(n, L);
    p->G = kWave / (p->T * L);
    p->stride = pc::list_stride(n, p->T);
    std::vector<uint32_t> sched;
    pc::list_schedule(mask, p->T, 0, n, sched);
    p->nsched = (uint32_t)sched.size();
    std::vector<uint16_t> tab, info;
    pc::positions(mask, N, tab, info);
    rc = aeth::upload_table(ctx, sched.data(), sched.size() * sizeof(uint32_t), &p->sched_dev, "aeth_polar_list_create: schedule");
    if (!rc) rc = aeth::upload_table(ctx, info.data(), info.size() * sizeof(uint16_t), &p->info_dev, "aeth_polar_list_create: information positions");
    if (rc) {
        (void)aeth::release_tables(ctx, {p->sched_dev, p->info_dev});
        delete p;
        return rc;
    }
    *out = p;
    return AETH_OK;
}

int aeth_polar_list_destroy(aeth_polar_list *p)
{
    if (!p) return AETH_OK;
    const hipError_t freed = aeth::release_tables(p->ctx, {p->sched_dev, p->info_dev});
    delete p;
    return freed == hipSuccess ? AETH_OK : aeth::hip_fail(freed, "hipFree");
}

size_t aeth_polar_list_n(const aeth_polar_list *p) { return p ? p->N : 0; }
size_t aeth_polar_list_k(const aeth_polar_list *p) { return p ? p->K : 0; }
uint32_t aeth_polar_list_paths(const aeth_polar_list *p) { return p ? p->L : 0; }
uint32_t aeth_polar_list_lanes(const aeth_polar_list *p) { return p ? p->T : 0; }
uint32_t aeth_polar_list_group(const aeth_polar_list *p) { return p ? p->G : 0; }
size_t aeth_polar_list_lds_bytes(const aeth_polar_list *p) { return p ? (size_t)(kWave / p->T) * (p->stride + 4) : 0; }

int aeth_polar_list_decode(aeth_polar_list *p, const int8_t *soft_dev, size_t nsoft, uint32_t flags, uint8_t *bits_dev, size_t nbits,
                           aeth_polar_list_record *rec_dev)
{
    AETH_REQUIRE(p, AETH_E_ARG, "polar list is null");
    if (int rc = aeth::check_flags(flags, AETH_POLAR_CODEWORD | AETH_POLAR_ALL)) return rc;
    const uint32_t per = ((flags & AETH_POLAR_ALL) ? p->L : 1u) * ((flags & AETH_POLAR_CODEWORD) ? p->N : p->K);
    size_t F;
    if (int rc = aeth::check_codewords(true, nsoft, p->N, nbits, per, &F)) return rc;
    if (F == 0) return AETH_OK;
    AETH_REQUIRE(soft_dev && bits_dev, AETH_E_ARG, "null pointer");
    AETH_REQUIRE(aeth::aligned4(rec_dev), AETH_E_ALIGN, "rec_dev not 4-byte aligned");
    if (int rc = aeth::check_disjoint({{soft_dev, nsoft}}, {{bits_dev, nbits}, {rec_dev, F * sizeof(aeth_polar_list_record)}})) return rc;
    const uint64_t wgs = (F + p->G - 1) / p->G;
    if (int rc = aeth::check_grid(wgs, F, "codewords")) return rc;
    aeth::DeviceGuard dg(p->ctx->device);
    hipStream_t st = aeth::ctx_stream(p->ctx);
    ListCall a{};
    a.soft = soft_dev; a.bits = bits_dev; a.rec = rec_dev;
    a.sched = p->sched_dev; a.info = p->info_dev;
    a.F = F;
    a.n = p->n; a.K = p->K; a.nsched = p->nsched; a.stride = p->stride;
    a.codeword = (flags & AETH_POLAR_CODEWORD) ? 1 : 0;
    a.all = (flags & AETH_POLAR_ALL) ? 1 : 0;
    const size_t lds = (size_t)(kWave / p->T) * (p->stride + 4);
#define AETH_LIST(T_, L_) hipLaunchKernelGGL((polar_list_kernel<T_, L_>), dim3((unsigned)wgs), dim3(kWave), lds, st, a)
    switch (p->T * 16 + p->L) {
    case 4 * 16 + 1: AETH_LIST(4, 1); break;
    case 4 * 16 + 2: AETH_LIST(4, 2); break;
    case 4 * 16 + 4: AETH_LIST(4, 4); break;
    case 4 * 16 + 8: AETH_LIST(4, 8); break;
    case 8 * 16 + 1: AETH_LIST(8, 1); break;
    case 8 * 16 + 2: AETH_LIST(8, 2); break;
    case 8 * 16 + 4: AETH_LIST(8, 4); break;
    case 8 * 16 + 8: AETH_LIST(8, 8); break;
    case 16 * 16 + 1: AETH_LIST(16, 1); break;
    case 16 * 16 + 2: AETH_LIST(16, 2); break;
    case 16 * 16 + 4: AETH_LIST(16, 4); break;
    default: return aeth::set_error(AETH_E_UNSUPPORTED, "no list kernel of %u lanes and %u paths", p->T, p->L);
    }
#undef AETH_LIST
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

int aeth_polar_list_pick(aeth_ctx *ctx, const uint8_t *rows_dev, size_t row_bytes, size_t F, uint32_t L, const uint64_t *diff_dev,
                         uint8_t *out_dev, uint32_t *which_dev)
{
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    AETH_REQUIRE(L >= 1 && L <= pc::kMaxList, AETH_E_ARG, "L = %u outside 1 .. %u", L, pc::kMaxList);
    AETH_REQUIRE(row_bytes >= 1, AETH_E_LEN, "row_bytes = 0");
    AETH_REQUIRE(row_bytes <= ((size_t)1 << 30), AETH_E_UNSUPPORTED, "row_bytes = %zu above 2^30", row_bytes);
    if (F == 0) return AETH_OK;
    const uint64_t total = aeth::mul_sat(F, row_bytes), all = aeth::mul_sat(total, L);
    AETH_REQUIRE(all <= ((uint64_t)1 << 48), AETH_E_LEN, "%zu codewords of %u rows of %zu bytes: more than 2^48 bytes", F, L, row_bytes);
    AETH_REQUIRE(rows_dev && diff_dev && out_dev, AETH_E_ARG, "null pointer");
    AETH_REQUIRE(aeth::aligned8(diff_dev), AETH_E_ALIGN, "diff_dev not 8-byte aligned");
    AETH_REQUIRE(aeth::aligned4(which_dev), AETH_E_ALIGN, "which_dev not 4-byte aligned");
    if (int rc = aeth::check_disjoint({{rows_dev, (size_t)all}, {diff_dev, F * L * sizeof(uint64_t)}},
                                      {{out_dev, (size_t)total}, {which_dev, F * sizeof(uint32_t)}}))
        return rc;
    const uint64_t wgs = (total + kPickBytes - 1) / kPickBytes;
    if (int rc = aeth::check_grid(wgs, F, "codewords")) return rc;
    aeth::DeviceGuard dg(ctx->device);
    hipStream_t st = aeth::ctx_stream(ctx);
    PickCall a{rows_dev, diff_dev, out_dev, which_dev, total, (uint32_t)row_bytes, L};
    hipLaunchKernelGGL(polar_pick_kernel, dim3((unsigned)wgs), dim3(kPickBlock), 0, st, a);
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

}  // extern "C"
