// aeth_ldpc.hip -- quasi-cyclic LDPC codes: a systematic encoder and a layered normalised min-sum decoder in integers (no
// body in the reference; definition in include/aether_hip.h, aeth_ldpc_*).  Everything is integer and defined byte for
// byte; compiled with the EXACT flags like the other bit-exact kernels.
//
// Decoder.  A workgroup holds G codewords (group_of): G z <= 256 lanes where z < 256, else one codeword whose checks the
// 256 lanes take in turns.  Per codeword the LDS holds Q as int16 [N] and R as int8 [E][z]; a lane owns check (r, i) of
// the current layer and walks the row's edges twice: once for the two minima, the argmin and the sign parity, once to
// write R and Q back (the messages of a check are not kept in registers, so the degree is unbounded and nothing spills).
// The row's edge list -- (c z) | (shift << 16), columns ascending -- is read with a uniform index, so it comes through
// the scalar cache.  Lanes i, i + 1 of a check row touch Q[c z + (i + s) mod z] and R[e z + i]: consecutive int16 and
// bytes, two and four lanes per LDS bank word and no conflicts apart from the wrap.  One workgroup barrier per layer.
// After an iteration (every one with AETH_LDPC_EARLY, else the last) the lanes count their rows' unsatisfied checks from
// the hard decisions and add them per codeword with an LDS atomic; the count is a sum of integers, so it is the same in
// every run.  A finished codeword's lanes only keep the barriers; with early stop a flag in LDS (one more barrier per
// iteration) tells the workgroup when none of its codewords goes on.
//
// Encoder.  A workgroup takes kEncGroup codewords.  Each wave packs 64 information bits at a time into an LDS word with a
// ballot (and copies them, & 1, to the output); then lane i holds row i of P, one word at a time from the transposed
// table Pt[w][i] (consecutive lanes, consecutive words), ands it with the word of every codeword (a broadcast read) and
// writes the parity of the popcount.
#include "aeth_ldpc_core.h"

#include <algorithm>
#include <new>
#include <vector>

namespace {

namespace lc = aeth::ldpc;

constexpr int kBlock = 256;
constexpr uint32_t kEncGroup = 8;                      // codewords per encoder workgroup
constexpr uint32_t kMaxIter = 1000;
constexpr size_t kLdsBudget = 65536;                   // dynamic LDS of a decoder workgroup

// The row starts and the edge list never change while a kernel runs: read through the constant address space they come
// by scalar loads (as global memory the compiler could not rule out a store in between and took a vector load and a wait
// per edge).
typedef const uint32_t __attribute__((address_space(4))) *ConstTab;
__device__ __forceinline__ ConstTab const_tab(const uint32_t *p) { return (ConstTab)(uintptr_t)p; }

struct DecCall {
    const int8_t *soft;
    uint8_t *bits;
    aeth_ldpc_record *rec;              // or null
    const uint32_t *row_start, *edges;
    uint64_t F;
    uint32_t rows, z, N, E, G, nb;      // nb: output bits per codeword (N or K)
    uint32_t max_iter, early;
};

// the unsatisfied checks among rows x {i} of one codeword, from the hard decisions
__device__ __forceinline__ uint32_t unsat_of(const DecCall &a, const int16_t *Qg, uint32_t i)
{
    const ConstTab row_start = const_tab(a.row_start), edges = const_tab(a.edges);
    uint32_t bad = 0;
    for (uint32_t r = 0; r < a.rows; r++) {
        const uint32_t e1 = row_start[r + 1];
        uint32_t par = 0;
        for (uint32_t e = row_start[r]; e < e1; e++) {
            const uint32_t pk = edges[e];
            uint32_t x = i + (pk >> 16);
            x -= x >= a.z ? a.z : 0;
            par ^= (uint32_t)(Qg[(pk & 0xffffu) + x] < 0);
        }
        bad += par;
    }
    return bad;
}

__global__ __launch_bounds__(kBlock) void ldpc_decode_kernel(DecCall a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldpc_lds[];
    __shared__ uint32_t cnt[2][kBlock];                                   // unsatisfied checks per codeword, two iterations apart
    __shared__ uint32_t live[2];                                          // early stop: a codeword of the workgroup goes on
    const uint32_t tid = threadIdx.x, bd = blockDim.x;
    const uint32_t Ez = a.E * a.z, lanes = a.G * a.z;
    const ConstTab row_start = const_tab(a.row_start), edges = const_tab(a.edges);
    int8_t *R = reinterpret_cast<int8_t *>(ldpc_lds);                     // [G][E z]
    int16_t *Q = reinterpret_cast<int16_t *>(ldpc_lds + ((a.G * Ez + 1u) & ~1u));      // [G][N]
    const uint64_t f0 = (uint64_t)blockIdx.x * a.G;
    const uint32_t Gv = (uint32_t)(a.F - f0 < a.G ? a.F - f0 : a.G);      // codewords of this workgroup

    // the lane's codeword and, where G z <= 256, its one check index; a lone codeword's lanes take i = tid, tid + bd, ...
    const uint32_t g = a.G > 1 ? tid / a.z : 0;
    const uint32_t i0 = a.G > 1 ? tid - g * a.z : tid;
    const bool mine = tid < lanes && g < Gv;                              // the lane has a check of a real codeword
    int16_t *Qg = Q + (size_t)g * a.N;
    int8_t *Rg = R + (size_t)g * Ez;

    {   // R = 0: whole words, then the bytes behind them
        const uint32_t nR = a.G * Ez;
        uint32_t *Rw = reinterpret_cast<uint32_t *>(R);
        for (uint32_t k = tid; k < nR / 4; k += bd) Rw[k] = 0;
        for (uint32_t k = (nR & ~3u) + tid; k < nR; k += bd) R[k] = 0;
    }
    for (uint32_t c = 0; c < Gv; c++) {
        const int8_t *src = a.soft + (f0 + c) * a.N;
        for (uint32_t v = tid; v < a.N; v += bd) Q[(size_t)c * a.N + v] = src[v];
    }
    cnt[0][tid & (kBlock - 1)] = 0;
    cnt[1][tid & (kBlock - 1)] = 0;
    if (tid < 2) live[tid] = 0;
    __syncthreads();

    bool done = !mine;
    uint32_t iters = 0, unsat = 0;
    if (a.max_iter == 0) {
        if (mine) {
            uint32_t bad = 0;
            for (uint32_t i = i0; i < a.z; i += bd) { bad += unsat_of(a, Qg, i); if (a.G > 1) break; }
            if (bad) atomicAdd(&cnt[0][g], bad);
        }
        __syncthreads();
        if (mine) unsat = cnt[0][g];
    }
    for (uint32_t it = 0; it < a.max_iter; it++) {
        if (a.early && it > 0) {
            __syncthreads();
            if (!live[(it - 1) & 1]) break;                               // every codeword of the workgroup has stopped
        }
        for (uint32_t r = 0; r < a.rows; r++) {
            const uint32_t e0 = row_start[r], e1 = row_start[r + 1];
            if (!done) {
                for (uint32_t i = i0; i < a.z; i += bd) {
                    int32_t m1 = 32767, m2 = 32767;
                    uint32_t arg = ~0u, par = 0;
                    for (uint32_t e = e0; e < e1; e++) {
                        const uint32_t pk = edges[e];
                        uint32_t x = i + (pk >> 16);
                        x -= x >= a.z ? a.z : 0;
                        const int32_t T = (int32_t)Qg[(pk & 0xffffu) + x] - (int32_t)Rg[e * a.z + i];
                        par ^= (uint32_t)(T < 0);
                        const int32_t m = T < 0 ? -T : T;
                        if (m < m1) { m2 = m1; m1 = m; arg = e; }
                        else if (m < m2) m2 = m;
                    }
                    const int32_t mag_arg = min((3 * m2) >> 2, 127), mag = min((3 * m1) >> 2, 127);
                    for (uint32_t e = e0; e < e1; e++) {
                        const uint32_t pk = edges[e];
                        uint32_t x = i + (pk >> 16);
                        x -= x >= a.z ? a.z : 0;
                        int16_t *q = Qg + (pk & 0xffffu) + x;
                        int8_t *rr = Rg + e * a.z + i;
                        const int32_t T = (int32_t)*q - (int32_t)*rr;
                        const int32_t mg = e == arg ? mag_arg : mag;
                        const int32_t Rn = (par ^ (uint32_t)(T < 0)) ? -mg : mg;
                        *rr = (int8_t)Rn;
                        *q = (int16_t)(T + Rn);
                    }
                    if (a.G > 1) break;
                }
            }
            __syncthreads();
        }
        if (!done) iters = it + 1;
        if (a.early || it + 1 == a.max_iter) {
            if (!done) {
                uint32_t bad = 0;
                for (uint32_t i = i0; i < a.z; i += bd) { bad += unsat_of(a, Qg, i); if (a.G > 1) break; }
                if (bad) atomicAdd(&cnt[it & 1][g], bad);
            }
            cnt[(it + 1) & 1][tid & (kBlock - 1)] = 0;                    // last read one iteration (at least one barrier) ago
            if (tid == 0) live[(it + 1) & 1] = 0;
            __syncthreads();
            if (!done) {
                unsat = cnt[it & 1][g];
                if (a.early && unsat == 0) done = true;
                else live[it & 1] = 1;
            }
        }
    }
    __syncthreads();
    for (uint32_t c = 0; c < Gv; c++) {
        uint8_t *dst = a.bits + (f0 + c) * a.nb;
        for (uint32_t v = tid; v < a.nb; v += bd) dst[v] = (uint8_t)(Q[(size_t)c * a.N + v] < 0);
    }
    if (a.rec && mine && i0 == 0) a.rec[f0 + g] = aeth_ldpc_record{iters, unsat};
}

struct EncCall {
    const uint8_t *in;
    uint8_t *out;
    const uint64_t *Pt;                 // [KW][M]
    uint64_t F;
    uint32_t N, K, M, KW;
};

__global__ __launch_bounds__(kBlock) void ldpc_encode_kernel(EncCall a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ldpc_lds[];
    uint64_t *u = reinterpret_cast<uint64_t *>(ldpc_lds);                 // [kEncGroup][KW]
    const uint32_t tid = threadIdx.x, wave = tid >> 6, lane = tid & 63u;
    const uint64_t f0 = (uint64_t)blockIdx.x * kEncGroup;
    for (uint32_t c = 0; c < kEncGroup; c++) {
        const bool real = f0 + c < a.F;
        const uint8_t *src = a.in + (f0 + c) * a.K;
        uint8_t *dst = a.out + (f0 + c) * a.N;
        for (uint32_t w = wave; w < a.KW; w += kBlock / 64) {
            const uint32_t j = w * 64 + lane;
            uint32_t bit = 0;
            if (real && j < a.K) {
                bit = src[j] & 1u;
                dst[j] = (uint8_t)bit;
            }
            const uint64_t word = __ballot(bit);
            if (lane == 0) u[c * a.KW + w] = word;
        }
    }
    __syncthreads();
    for (uint32_t i = tid; i < a.M; i += kBlock) {
        uint64_t acc[kEncGroup];
#pragma unroll
        for (uint32_t c = 0; c < kEncGroup; c++) acc[c] = 0;
        for (uint32_t w = 0; w < a.KW; w++) {
            const uint64_t p = a.Pt[(size_t)w * a.M + i];
#pragma unroll
            for (uint32_t c = 0; c < kEncGroup; c++) acc[c] ^= p & u[c * a.KW + w];
        }
#pragma unroll
        for (uint32_t c = 0; c < kEncGroup; c++)
            if (f0 + c < a.F) a.out[(f0 + c) * a.N + a.K + i] = (uint8_t)(__popcll(acc[c]) & 1);
    }
}

// codewords per decoder workgroup: as many as keep G z <= 256 lanes and G states inside the LDS budget, at least one
uint32_t group_of(uint32_t z, uint64_t state)
{
    const uint64_t by_lanes = z < (uint32_t)kBlock ? (uint32_t)kBlock / z : 1;
    const uint64_t by_lds = kLdsBudget / (state + 1);                     // + 1: R is padded to an even byte count
    return (uint32_t)std::max<uint64_t>(1, std::min(by_lanes, by_lds));
}

}  // namespace

struct aeth_ldpc {
    aeth_ctx *ctx;
    uint32_t rows, cols, z, N, M, K, E, G, KW;
    uint32_t *tab_dev;                  // [rows + 1] row starts, then [E] edges
    uint64_t *pt_dev;                   // [KW][M]
};

namespace {
size_t dec_lds(const aeth_ldpc *l) { return (((size_t)l->G * l->E * l->z + 1) & ~(size_t)1) + (size_t)2 * l->G * l->N; }
}  // namespace

extern "C" {

int aeth_ldpc_generator(const aeth_ldpc_code *code, uint64_t *p_out, size_t nwords)
{
    lc::Shape s;
    int rc = lc::check_code(code, s);
    if (rc) return rc;
    const size_t need = (size_t)s.M * lc::words_of(s.K);
    AETH_REQUIRE(nwords >= need, AETH_E_LEN, "P of %u rows of %zu words needs %zu words, p_out holds %zu", s.M, lc::words_of(s.K), need, nwords);
    AETH_REQUIRE(p_out, AETH_E_ARG, "p_out is null");
    std::vector<uint64_t> P;
    rc = lc::generator(s, P);
    if (rc) return rc;
    std::copy(P.begin(), P.end(), p_out);
    return AETH_OK;
}

int aeth_ldpc_create(aeth_ctx *ctx, const aeth_ldpc_code *code, aeth_ldpc **out)
{
    AETH_REQUIRE(out, AETH_E_ARG, "out is null");
    *out = nullptr;
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    lc::Shape s;
    int rc = lc::check_code(code, s);
    if (rc) return rc;
    std::vector<uint64_t> P;
    rc = lc::generator(s, P);
    if (rc) return rc;
    aeth_ldpc *l = new (std::nothrow) aeth_ldpc{};
    AETH_REQUIRE(l, AETH_E_NOMEM, "out of host memory");
    l->ctx = ctx;
    l->rows = s.rows; l->cols = s.cols; l->z = s.z; l->N = s.N; l->M = s.M; l->K = s.K; l->E = s.E;
    l->KW = (uint32_t)lc::words_of(s.K);
    l->G = group_of(s.z, s.state());
    std::vector<uint64_t> Pt((size_t)l->KW * s.M);
    for (uint32_t i = 0; i < s.M; i++)
        for (uint32_t w = 0; w < l->KW; w++) Pt[(size_t)w * s.M + i] = P[(size_t)i * l->KW + w];
    std::vector<uint32_t> tab(s.row_start);
    tab.insert(tab.end(), s.edges.begin(), s.edges.end());
    rc = aeth::upload_table(ctx, tab.data(), tab.size() * sizeof(uint32_t), &l->tab_dev, "aeth_ldpc_create: edge table");
    if (!rc) rc = aeth::upload_table(ctx, Pt.data(), Pt.size() * sizeof(uint64_t), &l->pt_dev, "aeth_ldpc_create: generator");
    if (rc) {
        (void)aeth::release_tables(ctx, {l->tab_dev, l->pt_dev});
        delete l;
        return rc;
    }
    *out = l;
    return AETH_OK;
}

int aeth_ldpc_destroy(aeth_ldpc *l)
{
    if (!l) return AETH_OK;
    const hipError_t freed = aeth::release_tables(l->ctx, {l->tab_dev, l->pt_dev});
    delete l;
    return freed == hipSuccess ? AETH_OK : aeth::hip_fail(freed, "hipFree");
}

size_t aeth_ldpc_n(const aeth_ldpc *l) { return l ? l->N : 0; }
size_t aeth_ldpc_k(const aeth_ldpc *l) { return l ? l->K : 0; }
uint32_t aeth_ldpc_rows(const aeth_ldpc *l) { return l ? l->rows : 0; }
uint32_t aeth_ldpc_cols(const aeth_ldpc *l) { return l ? l->cols : 0; }
uint32_t aeth_ldpc_z(const aeth_ldpc *l) { return l ? l->z : 0; }
size_t aeth_ldpc_edges(const aeth_ldpc *l) { return l ? l->E : 0; }
size_t aeth_ldpc_lds_bytes(const aeth_ldpc *l) { return l ? dec_lds(l) : 0; }
uint32_t aeth_ldpc_group(const aeth_ldpc *l) { return l ? l->G : 0; }

int aeth_ldpc_encode(aeth_ldpc *l, const uint8_t *bits_dev, size_t nbits, uint8_t *coded_dev, size_t ncoded)
{
    AETH_REQUIRE(l, AETH_E_ARG, "ldpc is null");
    size_t F;
    if (int rc = aeth::check_codewords(false, nbits, l->K, ncoded, l->N, &F)) return rc;
    if (F == 0) return AETH_OK;
    AETH_REQUIRE(bits_dev && coded_dev, AETH_E_ARG, "null pointer");
    if (int rc = aeth::check_disjoint({{bits_dev, nbits}}, {{coded_dev, ncoded}})) return rc;
    const uint64_t wgs = (F + kEncGroup - 1) / kEncGroup;
    if (int rc = aeth::check_grid(wgs, F, "codewords")) return rc;
    aeth::DeviceGuard dg(l->ctx->device);
    hipStream_t st = aeth::ctx_stream(l->ctx);
    EncCall a{bits_dev, coded_dev, l->pt_dev, (uint64_t)F, l->N, l->K, l->M, l->KW};
    hipLaunchKernelGGL(ldpc_encode_kernel, dim3((unsigned)wgs), dim3(kBlock), (size_t)kEncGroup * l->KW * sizeof(uint64_t), st, a);
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

int aeth_ldpc_decode(aeth_ldpc *l, const int8_t *soft_dev, size_t nsoft, uint32_t max_iter, uint32_t flags, uint8_t *bits_dev, size_t nbits,
                     aeth_ldpc_record *rec_dev)
{
    AETH_REQUIRE(l, AETH_E_ARG, "ldpc is null");
    if (int rc = aeth::check_flags(flags, AETH_LDPC_EARLY | AETH_LDPC_PAYLOAD)) return rc;
    AETH_REQUIRE(max_iter <= kMaxIter, AETH_E_ARG, "max_iter %u above %u", max_iter, kMaxIter);
    const uint32_t nb = (flags & AETH_LDPC_PAYLOAD) ? l->K : l->N;
    size_t F;
    if (int rc = aeth::check_codewords(true, nsoft, l->N, nbits, nb, &F)) return rc;
    if (F == 0) return AETH_OK;
    AETH_REQUIRE(soft_dev && bits_dev, AETH_E_ARG, "null pointer");
    AETH_REQUIRE(aeth::aligned4(rec_dev), AETH_E_ALIGN, "rec_dev not 4-byte aligned");
    if (int rc = aeth::check_disjoint({{soft_dev, nsoft}}, {{bits_dev, nbits}, {rec_dev, F * sizeof(aeth_ldpc_record)}})) return rc;
    const uint64_t wgs = (F + l->G - 1) / l->G;
    if (int rc = aeth::check_grid(wgs, F, "codewords")) return rc;
    aeth::DeviceGuard dg(l->ctx->device);
    hipStream_t st = aeth::ctx_stream(l->ctx);
    const size_t lds = dec_lds(l);
    if (lds > 48 * 1024)
        AETH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(ldpc_decode_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    DecCall a{};
    a.soft = soft_dev; a.bits = bits_dev; a.rec = rec_dev;
    a.row_start = l->tab_dev; a.edges = l->tab_dev + l->rows + 1;
    a.F = F;
    a.rows = l->rows; a.z = l->z; a.N = l->N; a.E = l->E; a.G = l->G; a.nb = nb;
    a.max_iter = max_iter; a.early = (flags & AETH_LDPC_EARLY) ? 1 : 0;
    const uint32_t lanes = std::min<uint64_t>((uint64_t)l->G * l->z, kBlock);
    hipLaunchKernelGGL(ldpc_decode_kernel, dim3((unsigned)wgs), dim3((lanes + 63) & ~63u), lds, st, a);
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

}  // extern "C"
