// aeth_sequence.hip -- LFSR sequences generated on the device: bits, scramble, chips, spread
// (reference: src/sequence.rs:18-53, expand + generate with a linear generator closure).
// The recurrence is linear over GF(2), so a 64-bit window of the sequence moves p -> p + 2^j by one 64 x 64 bit
// matrix (aeth_seq_core.h).  The host computes every register's window at the start of the call; a wave owns kChunk
// consecutive positions, jumps to its start by the rows of P^(kChunk * 2^j) (lane r holds row r, the new window is the
// ballot of parity(row & window)), then makes 64 bits per ballot with the rows of P^64.  The sequence never touches
// memory: the four epilogues turn 64 words (one per lane) straight into 16-byte stores.
// All integer; compiled with the EXACT flags like the other bit-exact kernels.
#include "aeth_internal.h"
#include "aeth_seq_core.h"

#include <new>

namespace {

constexpr int kBlock = 256;                        // 4 waves
constexpr int kWaves = kBlock / 64;
constexpr int kRound = 4096;                       // positions per round: 64 lanes x one 64-bit word
constexpr int kRounds = 4;                         // rounds a wave makes from one jump-ahead
constexpr int kChunkLog2 = 14;
constexpr size_t kChunk = (size_t)kRound * kRounds;
static_assert(kChunk == (size_t)1 << kChunkLog2, "the jump table is P^(kChunk * 2^j) = P^(2^(kChunkLog2 + j))");
constexpr int kLevels = 32;                        // chunk indices are 32-bit
constexpr int kMaxRegs = 4;
constexpr size_t kRegRows = (size_t)(1 + kLevels) * 64;   // per register: rows of P^64, then of every level

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 u32x4_u __attribute__((aligned(1)));

struct SeqCall {
    uint64_t w[kMaxRegs];      // every register's window at the first position of the aligned body
    const uint64_t *tab;       // kRegRows rows per register
    unsigned nregs, nlevels;   // nlevels: bits of the largest chunk index of this launch
    unsigned head, nhead;      // the elements in front of the 16-byte aligned body: bit i of head = c[i], i < nhead
};

__device__ __forceinline__ uint64_t jump(uint64_t row, uint64_t w) { return __ballot(__popcll(row & w) & 1); }

__device__ __forceinline__ uint64_t shfl64(uint64_t v, unsigned src)
{
    const unsigned lo = __shfl((unsigned)v, (int)src), hi = __shfl((unsigned)(v >> 32), (int)src);
    return ((uint64_t)hi << 32) | lo;
}

// The shared generator.  epi.head() stores the elements in front of the aligned body (one lane of the launch);
// epi.load(p) may start loads for the round at body position p; epi.store(p, word, lane) receives the round's 4096
// sequence bits, lane k holding positions p + 64k .. p + 64k + 63.
template <class Epi> __device__ __forceinline__ void generate(const SeqCall &a, size_t nbody, Epi &epi)
{
    const unsigned lane = threadIdx.x & 63u;
    const unsigned c = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // chunk index, wave-uniform
    if (c == 0 && lane == 0) epi.head();
    const size_t p0 = (size_t)c * kChunk;
    if (p0 >= nbody) return;
    uint64_t p64[kMaxRegs], w[kMaxRegs];
#pragma unroll
    for (int r = 0; r < kMaxRegs; r++) {
        p64[r] = 0; w[r] = 0;
        if (r >= (int)a.nregs) continue;
        const uint64_t *t = a.tab + r * kRegRows + lane;
        p64[r] = t[0];
        uint64_t wr = a.w[r];
        // the rows of eight levels at a time, all loads first: the addresses do not depend on the data
        for (unsigned jb = 0; jb < a.nlevels; jb += 8) {
            uint64_t rows[8];
#pragma unroll
            for (unsigned i = 0; i < 8; i++) rows[i] = (jb + i < a.nlevels) ? t[(size_t)(1 + jb + i) * 64] : 0;
#pragma unroll
            for (unsigned i = 0; i < 8; i++)
                if ((c >> (jb + i)) & 1u) wr = jump(rows[i], wr);
        }
        w[r] = wr;
    }
    for (int b = 0; b < kRounds; b++) {
        const size_t pb = p0 + (size_t)b * kRound;
        if (pb >= nbody) return;
        epi.load(pb, lane);
        uint64_t mine = 0;
#pragma unroll 8
        for (unsigned k = 0; k < 64; k++) {
            uint64_t x = 0;
#pragma unroll
            for (int r = 0; r < kMaxRegs; r++) {
                if (r >= (int)a.nregs) continue;
                x ^= w[r];
                w[r] = jump(p64[r], w[r]);
            }
            mine = (lane == k) ? x : mine;
        }
        epi.store(pb, mine, lane);
    }
}

// four bits -> four bytes of 0 / 1
__device__ __forceinline__ unsigned spread4(unsigned nib) { return (nib | (nib << 7) | (nib << 14) | (nib << 21)) & 0x01010101u; }

// ---- bits / scramble: 1 B per position, 16 positions per store ------------------------------------------------------
template <bool SCR, bool NT> struct BitsEpi {
    const SeqCall &a;
    const uint8_t *in;         // body-relative (SCR only)
    uint8_t *out;              // body-relative, 16-byte aligned
    size_t nbody;
    bool in_al;                // `in` is 16-byte aligned too
    u32x4 pre[4];

    __device__ __forceinline__ void head()
    {
        for (unsigned i = 0; i < a.nhead; i++) {
            uint8_t *o = out - a.nhead + i;
            unsigned v = (a.head >> i) & 1u;
            if constexpr (SCR) v ^= in[(ptrdiff_t)i - (ptrdiff_t)a.nhead] & 1u;
            *o = (uint8_t)v;
        }
    }
    __device__ __forceinline__ void load(size_t pb, unsigned lane)
    {
        if constexpr (SCR) {
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const size_t i0 = pb + (size_t)(s * 64 + lane) * 16;
                pre[s] = u32x4{0, 0, 0, 0};
                if (i0 + 16 <= nbody) {
                    if (in_al) pre[s] = aeth::nt_load<NT>(reinterpret_cast<const u32x4 *>(in + i0));
                    else pre[s] = *reinterpret_cast<const u32x4_u *>(in + i0);
                }
            }
        }
    }
    __device__ __forceinline__ void store(size_t pb, uint64_t mine, unsigned lane)
    {
#pragma unroll
        for (int s = 0; s < 4; s++) {
            // group g = s * 64 + lane holds positions 16 g .. 16 g + 15 of the round: word g / 4, bits 16 (g % 4) ..
            const uint64_t wd = shfl64(mine, (unsigned)s * 16u + (lane >> 2));
            const unsigned h = (unsigned)(wd >> ((lane & 3u) * 16u)) & 0xffffu;
            u32x4 v = {spread4(h & 15u), spread4((h >> 4) & 15u), spread4((h >> 8) & 15u), spread4(h >> 12)};
            const size_t i0 = pb + (size_t)(s * 64 + lane) * 16;
            if (i0 + 16 <= nbody) {
                if constexpr (SCR) v ^= pre[s] & 0x01010101u;
                aeth::nt_store<NT>(reinterpret_cast<u32x4 *>(out + i0), v);
            } else if (i0 < nbody) {                                  // the ragged tail: one lane of the launch
#pragma unroll
                for (int t = 0; t < 16; t++) {
                    if (i0 + t >= nbody) break;
                    unsigned bit = (h >> t) & 1u;
                    if constexpr (SCR) bit ^= in[i0 + t] & 1u;
                    out[i0 + t] = (uint8_t)bit;
                }
            }
        }
    }
};

template <bool NT> __global__ __launch_bounds__(kBlock) void seq_bits_kernel(SeqCall a, uint8_t *out, size_t nbody)
{
    BitsEpi<false, NT> epi{a, nullptr, out, nbody, true, {}};
    generate(a, nbody, epi);
}

template <bool NT>
__global__ __launch_bounds__(kBlock) void seq_scramble_kernel(SeqCall a, const uint8_t *in, uint8_t *out, size_t nbody, int in_al)
{
    BitsEpi<true, NT> epi{a, in, out, nbody, in_al != 0, {}};
    generate(a, nbody, epi);
}

// ---- chips / spread: 8 B per position, two positions per store ------------------------------------------------------
// pair q = t * 64 + lane of a round holds positions 2q and 2q + 1: word q / 32 = 2t + lane / 32, bits 2 (lane % 32) ..
template <bool NT> __device__ __forceinline__ void store_pair(uint2 *out, size_t i0, size_t nbody, uint2 v0, uint2 v1)
{
    if (i0 + 2 <= nbody) aeth::nt_store<NT>(reinterpret_cast<u32x4 *>(out + i0), u32x4{v0.x, v0.y, v1.x, v1.y});
    else if (i0 < nbody) out[i0] = v0;
}

template <bool NT> struct ChipsEpi {
    const SeqCall &a;
    uint2 zero, one;
    uint2 *out;                // body-relative, 16-byte aligned
    size_t nbody;

    __device__ __forceinline__ void head() { if (a.nhead) out[-1] = (a.head & 1u) ? one : zero; }
    __device__ __forceinline__ void load(size_t, unsigned) {}
    __device__ __forceinline__ void store(size_t pb, uint64_t mine, unsigned lane)
    {
#pragma unroll 4
        for (unsigned t = 0; t < 32; t++) {
            const uint64_t wd = shfl64(mine, 2u * t + (lane >> 5));
            const unsigned two = (unsigned)(wd >> (2u * (lane & 31u))) & 3u;
            const uint2 v0 = (two & 1u) ? one : zero, v1 = (two & 2u) ? one : zero;
            store_pair<NT>(out, pb + 2 * (size_t)(t * 64 + lane), nbody, v0, v1);
        }
    }
};

template <bool NT> __global__ __launch_bounds__(kBlock) void seq_chips_kernel(SeqCall a, uint2 zero, uint2 one, uint2 *out, size_t nbody)
{
    ChipsEpi<NT> epi{a, zero, one, out, nbody};
    generate(a, nbody, epi);
}

// SF1: sf == 1 and `sym` 16-byte aligned like the body: symbols by 16-byte loads, no index arithmetic
template <bool SF1, bool NT> struct SpreadEpi {
    const SeqCall &a;
    const uint2 *sym;          // the call's sym_dev (NOT body-relative: element i of the call reads sym[i / sf])
    uint2 *out;                // body-relative, 16-byte aligned
    size_t nbody, sf;
    aeth::FastDiv fd;          // of sf, when sf < 2^31
    bool wide;                 // sf >= 2^31: a round crosses at most one symbol boundary

    static __device__ __forceinline__ uint2 flip(uint2 v, unsigned bit) { return make_uint2(v.x ^ (bit << 31), v.y ^ (bit << 31)); }
    __device__ __forceinline__ void head() { if (a.nhead) out[-1] = flip(sym[0], a.head & 1u); }
    __device__ __forceinline__ void load(size_t, unsigned) {}
    __device__ __forceinline__ void store(size_t pb, uint64_t mine, unsigned lane)
    {
        size_t qb = 0, rb = 0;
        if constexpr (!SF1) { qb = (pb + a.nhead) / sf; rb = (pb + a.nhead) % sf; }     // wave-uniform
#pragma unroll 4
        for (unsigned t = 0; t < 32; t++) {
            const uint64_t wd = shfl64(mine, 2u * t + (lane >> 5));
            const unsigned two = (unsigned)(wd >> (2u * (lane & 31u))) & 3u;
            const unsigned l = 2u * (t * 64u + lane);
            const size_t i0 = pb + l;
            if (i0 >= nbody) continue;
            const bool full = i0 + 2 <= nbody;
            uint2 s0, s1;
            if constexpr (SF1) {
                if (full) {
                    const u32x4 s = aeth::nt_load<NT>(reinterpret_cast<const u32x4 *>(sym + a.nhead + i0));
                    s0 = make_uint2(s.x, s.y); s1 = make_uint2(s.z, s.w);
                } else s0 = s1 = sym[a.nhead + i0];
            } else {
                size_t q0, q1;
                if (wide) { q0 = qb + (rb + l >= sf); q1 = qb + (rb + l + 1 >= sf); }
                else { q0 = qb + aeth::fdiv((uint32_t)rb + l, fd); q1 = qb + aeth::fdiv((uint32_t)rb + l + 1u, fd); }
                s0 = sym[q0];
                s1 = full ? sym[q1] : s0;
            }
            store_pair<NT>(out, i0, nbody, flip(s0, two & 1u), flip(s1, two >> 1));
        }
    }
};

template <bool SF1, bool NT>
__global__ __launch_bounds__(kBlock) void seq_spread_kernel(SeqCall a, const uint2 *sym, uint2 *out, size_t nbody, size_t sf,
                                                            aeth::FastDiv fd, int wide)
{
    SpreadEpi<SF1, NT> epi{a, sym, out, nbody, sf, fd, wide != 0};
    generate(a, nbody, epi);
}

}  // namespace

struct aeth_seq {
    aeth_ctx *ctx;
    size_t nregs;
    size_t order[kMaxRegs];
    uint64_t mask[kMaxRegs];
    aeth::seq::Mat *pw;        // [nregs][64]: P^(2^j), host
    uint64_t *tab_dev;         // [nregs][kRegRows]
};

namespace {

int check_reg(const aeth_seq_reg *reg, size_t idx, uint64_t *mask, unsigned *order)
{
    AETH_REQUIRE(reg, AETH_E_ARG, "register is null");
    size_t which = 0;
    switch (aeth::seq::reg_problem(reg->delays, reg->ndelays, mask, order, &which)) {
    case 1: return aeth::set_error(AETH_E_ARG, "register %zu: delays is null", idx);
    case 2: return aeth::set_error(AETH_E_ARG, "register %zu: %zu delays, 1 .. 64 supported", idx, reg->ndelays);
    case 3: return aeth::set_error(AETH_E_ARG, "register %zu: delay %u outside 1 .. 64", idx, reg->delays[which]);
    case 4: return aeth::set_error(AETH_E_ARG, "register %zu: delay %u is repeated", idx, reg->delays[which]);
    default: return AETH_OK;
    }
}

// what every device call checks first, in this order: object, init, skip + n
int check_call(const aeth_seq *s, const uint64_t *init, uint64_t skip, size_t n)
{
    AETH_REQUIRE(s, AETH_E_ARG, "seq is null");
    AETH_REQUIRE(init, AETH_E_ARG, "init is null");
    AETH_REQUIRE(skip + (uint64_t)n >= skip, AETH_E_ARG, "skip %llu + n %zu overflows", (unsigned long long)skip, n);
    return AETH_OK;
}

bool overlaps(const void *a, size_t na, const void *b, size_t nb)
{
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + nb && b0 < a0 + na;
}

// fills the kernel argument for a call whose first nhead elements sit in front of the aligned body
int prepare(aeth_seq *s, const uint64_t *init, uint64_t skip, size_t n, size_t nhead, SeqCall &a, unsigned &grid)
{
    const size_t nbody = n - nhead;
    const size_t nchunks = nbody ? (nbody + kChunk - 1) / kChunk : 1;
    AETH_REQUIRE(nchunks <= ((size_t)1 << kLevels), AETH_E_UNSUPPORTED, "n %zu: at most 2^%d positions per call", n, kLevels + kChunkLog2);
    a.tab = s->tab_dev;
    a.nregs = (unsigned)s->nregs;
    a.nlevels = 0;
    while (((nchunks - 1) >> a.nlevels) != 0) a.nlevels++;
    a.nhead = (unsigned)nhead;
    uint64_t head = 0;
    for (size_t r = 0; r < kMaxRegs; r++) {
        a.w[r] = 0;
        if (r >= s->nregs) continue;
        uint64_t w = aeth::seq::window_at(s->pw + r * 64, s->mask[r], (unsigned)s->order[r], init[r], skip);
        head ^= w;
        for (size_t i = 0; i < nhead; i++) w = aeth::seq::step(w, s->mask[r]);
        a.w[r] = w;
    }
    a.head = (unsigned)(head & 0xffffu);
    grid = (unsigned)((nchunks + kWaves - 1) / kWaves);
    return AETH_OK;
}

}  // namespace

extern "C" {

// sequence::generate with a linear generator, one window of it (src/sequence.rs:18-21, :47-53)
int aeth_seq_window(const struct aeth_seq_reg *reg, uint64_t init, uint64_t skip, uint64_t *window)
{
    uint64_t mask = 0;
    unsigned order = 0;
    int rc = check_reg(reg, 0, &mask, &order); if (rc) return rc;
    AETH_REQUIRE(window, AETH_E_ARG, "window is null");
    *window = aeth::seq::window_at(mask, order, init, skip);
    return AETH_OK;
}

int aeth_seq_create(aeth_ctx *ctx, const struct aeth_seq_reg *regs, size_t nregs, aeth_seq **out)
{
    AETH_REQUIRE(out, AETH_E_ARG, "out is null");
    *out = nullptr;
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    AETH_REQUIRE(regs, AETH_E_ARG, "regs is null");
    AETH_REQUIRE(nregs >= 1 && nregs <= (size_t)kMaxRegs, AETH_E_ARG, "%zu registers, 1 .. %d supported", nregs, kMaxRegs);
    aeth_seq tmp{};
    tmp.ctx = ctx;
    tmp.nregs = nregs;
    for (size_t r = 0; r < nregs; r++) {
        unsigned order = 0;
        int rc = check_reg(regs + r, r, &tmp.mask[r], &order); if (rc) return rc;
        tmp.order[r] = order;
    }
    aeth_seq *s = new (std::nothrow) aeth_seq(tmp);
    AETH_REQUIRE(s, AETH_E_NOMEM, "out of host memory");
    s->pw = new (std::nothrow) aeth::seq::Mat[nregs * 64];
    uint64_t *host = new (std::nothrow) uint64_t[nregs * kRegRows];
    if (!s->pw || !host) { delete[] s->pw; delete[] host; delete s; return aeth::set_error(AETH_E_NOMEM, "out of host memory"); }
    for (size_t r = 0; r < nregs; r++) {
        aeth::seq::Mat *pw = s->pw + r * 64;
        aeth::seq::powers(s->mask[r], pw, 64);
        uint64_t *t = host + r * kRegRows;
        for (int i = 0; i < 64; i++) t[i] = pw[6].row[i];                                        // P^64
        for (int j = 0; j < kLevels; j++)
            for (int i = 0; i < 64; i++) t[(size_t)(1 + j) * 64 + i] = pw[kChunkLog2 + j].row[i];   // P^(kChunk * 2^j)
    }
    const int rc = aeth::upload_table(ctx, host, nregs * kRegRows * sizeof(uint64_t), &s->tab_dev, "aeth_seq_create: jump table upload");
    delete[] host;
    if (rc) { delete[] s->pw; delete s; return rc; }
    *out = s;
    return AETH_OK;
}

int aeth_seq_destroy(aeth_seq *seq)
{
    if (!seq) return AETH_OK;
    aeth::DeviceGuard dg(seq->ctx->device);
    if (seq->tab_dev) (void)hipFree(seq->tab_dev);
    delete[] seq->pw;
    delete seq;
    return AETH_OK;
}

size_t aeth_seq_nregs(const aeth_seq *seq) { return seq ? seq->nregs : 0; }
size_t aeth_seq_order(const aeth_seq *seq, size_t reg) { return seq && reg < seq->nregs ? seq->order[reg] : 0; }
size_t aeth_seq_chunk(const aeth_seq *) { return kChunk; }

int aeth_seq_bits(aeth_seq *seq, const uint64_t *init, uint64_t skip, uint8_t *bits_dev, size_t n)
{
    int rc = check_call(seq, init, skip, n); if (rc) return rc;
    if (n == 0) return AETH_OK;
    AETH_REQUIRE(bits_dev, AETH_E_ARG, "null pointer");
    size_t nhead = (size_t)(-(uintptr_t)bits_dev & 15u);
    if (nhead > n) nhead = n;
    SeqCall a;
    unsigned grid;
    rc = prepare(seq, init, skip, n, nhead, a, grid); if (rc) return rc;
    aeth::DeviceGuard dg(seq->ctx->device);
    auto k = aeth::streams_past_cache(n) ? seq_bits_kernel<true> : seq_bits_kernel<false>;
    hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), 0, aeth::ctx_stream(seq->ctx), a, bits_dev + nhead, n - nhead);
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

int aeth_seq_scramble(aeth_seq *seq, const uint64_t *init, uint64_t skip, const uint8_t *in_dev, uint8_t *out_dev, size_t n)
{
    int rc = check_call(seq, init, skip, n); if (rc) return rc;
    if (n == 0) return AETH_OK;
    AETH_REQUIRE(in_dev && out_dev, AETH_E_ARG, "null pointer");
    AETH_REQUIRE(in_dev == out_dev || !overlaps(in_dev, n, out_dev, n), AETH_E_ARG,
                 "the output overlaps the input (only out == in runs in place)");
    size_t nhead = (size_t)(-(uintptr_t)out_dev & 15u);
    if (nhead > n) nhead = n;
    SeqCall a;
    unsigned grid;
    rc = prepare(seq, init, skip, n, nhead, a, grid); if (rc) return rc;
    aeth::DeviceGuard dg(seq->ctx->device);
    const int in_al = aeth::aligned16(in_dev + nhead) ? 1 : 0;
    auto k = aeth::streams_past_cache(2 * n) ? seq_scramble_kernel<true> : seq_scramble_kernel<false>;
    hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), 0, aeth::ctx_stream(seq->ctx), a, in_dev + nhead, out_dev + nhead, n - nhead, in_al);
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

int aeth_seq_chips(aeth_seq *seq, const uint64_t *init, uint64_t skip, aeth_cf32 zero, aeth_cf32 one, aeth_cf32 *out_dev, size_t n)
{
    int rc = check_call(seq, init, skip, n); if (rc) return rc;
    if (n == 0) return AETH_OK;
    AETH_REQUIRE(out_dev, AETH_E_ARG, "null pointer");
    AETH_REQUIRE(aeth::aligned8(out_dev), AETH_E_ALIGN, "output pointer not 8-byte aligned");
    const size_t nhead = aeth::aligned16(out_dev) ? 0 : 1;
    SeqCall a;
    unsigned grid;
    rc = prepare(seq, init, skip, n, nhead, a, grid); if (rc) return rc;
    aeth::DeviceGuard dg(seq->ctx->device);
    uint2 z, o;
    static_assert(sizeof(aeth_cf32) == sizeof(uint2), "cf32 is two 32-bit words");
    __builtin_memcpy(&z, &zero, sizeof z);
    __builtin_memcpy(&o, &one, sizeof o);
    auto k = aeth::streams_past_cache(n * sizeof(uint2)) ? seq_chips_kernel<true> : seq_chips_kernel<false>;
    hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), 0, aeth::ctx_stream(seq->ctx), a, z, o, (uint2 *)out_dev + nhead, n - nhead);
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

int aeth_seq_spread(aeth_seq *seq, const uint64_t *init, uint64_t skip, const aeth_cf32 *sym_dev, size_t nsym, size_t sf,
                    aeth_cf32 *out_dev, size_t n_out)
{
    int rc = check_call(seq, init, skip, n_out); if (rc) return rc;
    AETH_REQUIRE(sf >= 1, AETH_E_ARG, "spreading factor 0");
    AETH_REQUIRE(nsym <= SIZE_MAX / sf && n_out == nsym * sf, AETH_E_LEN, "output holds %zu chips, %zu symbols x %zu give %zu", n_out,
                 nsym, sf, nsym <= SIZE_MAX / sf ? nsym * sf : (size_t)0);
    if (n_out == 0) return AETH_OK;
    AETH_REQUIRE(sym_dev && out_dev, AETH_E_ARG, "null pointer");
    AETH_REQUIRE(aeth::aligned8(sym_dev) && aeth::aligned8(out_dev), AETH_E_ALIGN, "pointer not 8-byte aligned");
    AETH_REQUIRE((sf == 1 && (const aeth_cf32 *)out_dev == sym_dev) || !overlaps(sym_dev, nsym * 8, out_dev, n_out * 8), AETH_E_ARG,
                 "the output overlaps the symbols (only sf == 1 with out == sym runs in place)");
    const size_t nhead = aeth::aligned16(out_dev) ? 0 : 1;
    SeqCall a;
    unsigned grid;
    rc = prepare(seq, init, skip, n_out, nhead, a, grid); if (rc) return rc;
    aeth::DeviceGuard dg(seq->ctx->device);
    const bool sf1 = sf == 1 && aeth::aligned16(sym_dev + nhead);
    const bool wide = sf >= ((size_t)1 << 31);
    const aeth::FastDiv fd = aeth::make_fastdiv(wide ? 1u : (uint32_t)sf);
    const bool nt = aeth::streams_past_cache(n_out * sizeof(uint2));
    auto k = sf1 ? (nt ? seq_spread_kernel<true, true> : seq_spread_kernel<true, false>)
                 : (nt ? seq_spread_kernel<false, true> : seq_spread_kernel<false, false>);
    hipLaunchKernelGGL(k, dim3(grid), dim3(kBlock), 0, aeth::ctx_stream(seq->ctx), a, (const uint2 *)sym_dev, (uint2 *)out_dev + nhead,
                       n_out - nhead, sf, fd, wide ? 1 : 0);
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

int aeth_host_seq_bits(aeth_seq *seq, const uint64_t *init, uint64_t skip, uint8_t *bits_host, size_t n)
{
    int rc = check_call(seq, init, skip, n); if (rc) return rc;
    if (n == 0) return AETH_OK;
    AETH_REQUIRE(bits_host, AETH_E_ARG, "null pointer");
    aeth::HostIO io;
    rc = io.open(seq->ctx, n, 0); if (rc) return rc;
    rc = aeth_seq_bits(seq, init, skip, (uint8_t *)io.buf[0], n); if (rc) return rc;
    return io.get(bits_host, 0, n);
}

}  // extern "C"
