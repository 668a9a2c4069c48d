// aeth_rs.hip -- Reed-Solomon codes over GF(2^m), 3 <= m <= 8: a systematic encoder and a bounded-distance
// errors-and-erasures decoder over symbol-interleaved frames (no body in the reference; definition in
// include/aether_hip.h, aeth_rs_*).  Everything is integer and defined byte for byte; compiled with the EXACT flags like
// the other bit-exact kernels.
//
// Lane groups.  A codeword belongs to a group of R2 lanes, R2 the power of two at or above r; a workgroup of 256 lanes
// takes G = 256 / R2 consecutive codewords of the call (aeth_rs_group), numbered frame by frame, so with depth > 1
// neighbouring groups read neighbouring bytes.  A group never leaves its wave.
// Constant products.  Multiplying by a lane's constant c is GF(2)-linear: the lane keeps the eight images c x^b as the
// bytes of two registers and forms v c as eight select-XORs, with no table and no LDS access.
//   Encoder: lane q holds rem[q] of the LFSR and g_(r-1-q); per data symbol one broadcast of rem[0], one shift of rem
//   by a lane and one constant product.
//   Syndromes: lane q holds beta^(fcr + q) and runs Horner over the n symbols, which its group reads as one address.
// Decoder.  Stage 1, all lanes: syndromes, the erased positions (an LDS list per group), and the input copied through,
// masked.  A group whose syndromes are all zero and that has no erasure is finished.  Stage 2, lane 0 of every other
// group: Gamma, Berlekamp-Massey and Omega (aeth_rs_core.h, solve) on the group's LDS arrays with log / antilog tables in
// LDS.  Stage 3, all lanes of those groups: lane q tests the positions q, q + R2, ... (locate) and lists roots and error
// values.  Stage 4: a group with exactly L roots and no vanishing denominator writes its corrections over the copy and
// its record.  The stages are separated by workgroup barriers that every lane reaches.  A workgroup's {failed,
// corrected} goes to a scratch record; a one-workgroup launch folds the records into the summary (aeth_reduce.h), so
// the summary is the same in every run.
#include "aeth_internal.h"
#include "aeth_rs_core.h"
#include "aeth_reduce.h"

#include <algorithm>
#include <new>
#include <string>
#include <vector>

namespace {

namespace rc = aeth::rs;

constexpr int kBlock = 256;

struct Sum { uint64_t n_failed, n_corrected; };                           // aeth_rs_summary
struct SumAdd {
    __device__ __forceinline__ Sum operator()(const Sum &a, const Sum &b) const { return Sum{a.n_failed + b.n_failed, a.n_corrected + b.n_corrected}; }
};

// the images c x^b, b = 0 .. 7, of a constant: byte b of lo (b < 4) or hi
struct Images { uint32_t lo, hi; };
__device__ __forceinline__ Images images_of(uint32_t c, uint32_t m, uint32_t poly)
{
    Images im{0, 0};
    uint32_t v = c;
#pragma unroll
    for (int b = 0; b < 8; b++) {
        if (b < 4) im.lo |= v << (8 * b); else im.hi |= v << (8 * (b - 4));
        v <<= 1;
        if (v >> m) v ^= poly;
    }
    return im;
}
__device__ __forceinline__ uint32_t mulc(uint32_t v, const Images &im)
{
    uint32_t p = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        p ^= (0u - ((v >> b) & 1u)) & (im.lo >> (8 * b));
        p ^= (0u - ((v >> (b + 4)) & 1u)) & (im.hi >> (8 * b));
    }
    return p & 0xffu;
}

// what both kernels know of the code and the call
struct Geom {
    uint64_t W;                         // codewords of the call: frames x depth
    uint32_t m, poly, N0, fcr, prim, r, n, k;
    uint32_t lg, depth;                 // R2 = 1 << lg
};

// codeword w of the call: frame w / depth, column w % depth
__device__ __forceinline__ void place(const Geom &g, uint64_t w, uint64_t *frame, uint32_t *col)
{
    *frame = w / g.depth;
    *col = (uint32_t)(w - *frame * g.depth);
}

struct EncCall {
    Geom g;
    const uint8_t *in;
    uint8_t *out;
    const uint8_t *gen;                 // [r]: g_(r-1-q) for lane q
};

__global__ __launch_bounds__(kBlock) void rs_encode_kernel(EncCall a)
{
    const Geom &g = a.g;
    const uint32_t R2 = 1u << g.lg, q = threadIdx.x & (R2 - 1);
    const uint64_t w = (uint64_t)blockIdx.x * (kBlock >> g.lg) + (threadIdx.x >> g.lg);
    const bool live = w < g.W;
    uint64_t frame = 0;
    uint32_t col = 0;
    if (live) place(g, w, &frame, &col);
    const uint8_t *src = a.in + frame * g.depth * g.k + col;
    uint8_t *dst = a.out + frame * g.depth * g.n + col;
    const Images im = images_of(q < g.r ? a.gen[q] : 0u, g.m, g.poly);
    uint32_t rem = 0;
    for (uint32_t j = 0; j < g.k; j++) {
        const uint32_t d = live ? (uint32_t)src[(size_t)j * g.depth] & g.N0 : 0u;
        if (live && q == (j & (R2 - 1))) dst[(size_t)j * g.depth] = (uint8_t)d;
        const uint32_t fb = d ^ (uint32_t)__shfl((int)rem, 0, (int)R2);
        const uint32_t nxt = (uint32_t)__shfl_down((int)rem, 1, (int)R2);
        rem = (q + 1 < g.r ? nxt : 0u) ^ mulc(fb, im);
    }
    if (live && q < g.r) dst[(size_t)(g.k + q) * g.depth] = (uint8_t)rem;
}

struct DecCall {
    Geom g;
    const uint8_t *in, *era;            // era or null
    uint8_t *out;
    rc::Record *rec;                    // or null
    Sum *sums;                          // one per workgroup, or null
    const uint8_t *tab;                 // exp[512], log[256], roots[64]
    uint32_t nb;                        // output symbols per codeword: n or k
    uint32_t slot;                      // bytes of a group's LDS arrays
};

// the LDS arrays of group `grp`: five of r + 1 bytes, three of r, then three counters
__device__ __forceinline__ rc::Work work_of(unsigned char *base, uint32_t r)
{
    const uint32_t s = r + 1;
    return rc::Work{base, base + s, base + 2 * s, base + 3 * s, base + 4 * s, base + 5 * s, base + 6 * s, base + 7 * s};
}

__global__ __launch_bounds__(kBlock) void rs_decode_kernel(DecCall a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_lds[];
    __shared__ uint8_t t_exp[512];
    __shared__ uint8_t t_log[256];
    __shared__ Sum red_lds[4];
    const Geom &g = a.g;
    const uint32_t R2 = 1u << g.lg, q = threadIdx.x & (R2 - 1), grp = threadIdx.x >> g.lg, G = kBlock >> g.lg;
    const uint64_t w = (uint64_t)blockIdx.x * G + grp;
    const bool live = w < g.W;
    uint64_t frame = 0;
    uint32_t col = 0;
    if (live) place(g, w, &frame, &col);
    const size_t ibase = (size_t)(frame * g.depth * g.n + col);
    const uint8_t *src = a.in + ibase;
    const uint8_t *era = a.era ? a.era + ibase : nullptr;
    uint8_t *dst = a.out + frame * g.depth * a.nb + col;
    // counters of all groups behind the groups' arrays: erasures, roots, flags (1: a syndrome is non-zero, 2: a vanishing denominator)
    uint32_t *cnt = reinterpret_cast<uint32_t *>(rs_lds + (((size_t)G * a.slot + 3) & ~(size_t)3)) + 3 * grp;
    const rc::Work wk = work_of(rs_lds + (size_t)grp * a.slot, g.r);
    const rc::Tab tab{t_exp, t_log, g.N0, g.fcr, g.prim, g.r, g.n};

    for (uint32_t i = threadIdx.x; i < 512; i += kBlock) t_exp[i] = a.tab[i];
    t_log[threadIdx.x] = a.tab[512 + threadIdx.x];
    if (q == 0) { cnt[0] = 0; cnt[1] = 0; cnt[2] = 0; }
    __syncthreads();

    // stage 1
    if (live) {
        const Images im = images_of(q < g.r ? a.tab[768 + q] : 0u, g.m, g.poly);
        uint32_t S = 0;
#pragma unroll 4
        for (uint32_t j = 0; j < g.n; j++) S = mulc(S, im) ^ ((uint32_t)src[(size_t)j * g.depth] & g.N0);
        if (q < g.r) {
            wk.S[q] = (uint8_t)S;
            if (S) atomicOr(&cnt[2], 1u);
        }
        for (uint32_t j = q; j < g.n; j += R2) {
            if (j < a.nb) dst[(size_t)j * g.depth] = (uint8_t)(src[(size_t)j * g.depth] & g.N0);
            if (era && era[(size_t)j * g.depth]) {
                const uint32_t e = atomicAdd(&cnt[0], 1u);
                if (e < g.r) wk.era[e] = (uint8_t)(g.n - 1 - j);
            }
        }
    }
    __syncthreads();

    // stage 2
    const uint32_t f = cnt[0];
    const bool damaged = live && (f != 0 || (cnt[2] & 1u));
    const bool open = damaged && f <= g.r;
    if (open && q == 0) {
        const uint32_t L = rc::solve(tab, wk, f);
        wk.tmp[0] = (uint8_t)(L == ~0u ? 255u : L);                      // L <= r <= 64
    }
    __syncthreads();

    // stage 3
    const uint32_t L = open ? wk.tmp[0] : 255u;
    if (L != 255u) {
        for (uint32_t j = q; j < g.n; j += R2) {
            uint32_t mag = 0;
            const uint32_t h = rc::locate(tab, wk, L, j, &mag);
            if (h == 2) atomicOr(&cnt[2], 2u);
            if (h) {
                const uint32_t e = atomicAdd(&cnt[1], 1u);
                if (e < g.r) { wk.rpos[e] = (uint8_t)j; wk.rmag[e] = (uint8_t)(h == 1 ? mag : 0u); }
            }
        }
    }
    __syncthreads();

    // stage 4
    Sum mine{0, 0};
    if (damaged) {
        const bool ok = L != 255u && cnt[1] == L && !(cnt[2] & 2u);
        uint32_t corrected = 0;
        if (ok) {
            for (uint32_t e = 0; e < L; e++) corrected += wk.rmag[e] != 0;
            for (uint32_t e = q; e < L; e += R2) {
                const uint32_t j = wk.rpos[e], mag = wk.rmag[e];
                if (mag && j < a.nb) dst[(size_t)j * g.depth] = (uint8_t)(((uint32_t)src[(size_t)j * g.depth] & g.N0) ^ mag);
            }
        }
        if (q == 0) {
            mine = Sum{ok ? 0u : 1u, corrected};
            if (a.rec) a.rec[w] = rc::Record{corrected, ok ? 0u : 1u};
        }
    } else if (live && q == 0 && a.rec) {
        a.rec[w] = rc::Record{0, 0};
    }
    if (a.sums) {                                                         // uniform over the launch
        mine = aeth::red::block_reduce(mine, red_lds, SumAdd{});
        if (threadIdx.x == 0) a.sums[blockIdx.x] = mine;
    }
}

__global__ __launch_bounds__(kBlock) void rs_summary_kernel(const Sum *sums, size_t n, Sum *out)
{
    __shared__ Sum lds[4];
    const Sum t = aeth::red::fold(sums, n, n, Sum{0, 0}, lds, SumAdd{});
    if (threadIdx.x == 0) *out = t;
}

// every rule of the header on a code; fills the field
int check_code(const aeth_rs_code *code, rc::Field &f)
{
    AETH_REQUIRE(code, AETH_E_ARG, "code is null");
    AETH_REQUIRE(code->m >= 3 && code->m <= 8, AETH_E_ARG, "symbol width m = %u outside 3 .. 8", code->m);
    const uint32_t N0 = (1u << code->m) - 1;
    AETH_REQUIRE((code->poly >> code->m) == 1, AETH_E_ARG, "poly 0x%x is not of degree m = %u (the x^m term is part of it)", code->poly, code->m);
    AETH_REQUIRE(rc::build_field(code->m, code->poly, f), AETH_E_ARG, "polynomial not primitive: poly 0x%x, m = %u", code->poly, code->m);
    AETH_REQUIRE(code->prim >= 1 && rc::gcd(code->prim, N0) == 1, AETH_E_ARG, "prim %u shares a factor with 2^m - 1 = %u", code->prim, N0);
    AETH_REQUIRE(code->fcr < N0, AETH_E_ARG, "fcr %u at or above 2^m - 1 = %u", code->fcr, N0);
    AETH_REQUIRE(code->nroots >= 1, AETH_E_ARG, "nroots %u below 1", code->nroots);
    AETH_REQUIRE(code->nroots <= rc::kMaxRoots, AETH_E_UNSUPPORTED, "nroots %u above %u", code->nroots, rc::kMaxRoots);
    AETH_REQUIRE(code->n > code->nroots && code->n <= N0, AETH_E_ARG, "length n = %u outside nroots + 1 = %u .. 2^m - 1 = %u", code->n, code->nroots + 1, N0);
    return AETH_OK;
}

rc::Code code_of(const aeth_rs_code *c) { return rc::Code{c->m, c->poly, c->fcr, c->prim % (((1u << c->m) - 1)), c->nroots, c->n}; }

int check_depth(uint32_t depth)
{
    AETH_REQUIRE(depth >= 1 && depth <= rc::kMaxDepth, AETH_E_ARG, "depth %u outside 1 .. %u", depth, rc::kMaxDepth);
    return AETH_OK;
}

// the lengths of a call: whole frames on both sides, the same number of them
int check_frames(const char *in_name, size_t nin, size_t in_frame, const char *out_name, size_t nout, size_t out_frame, size_t *F)
{
    AETH_REQUIRE(nin % in_frame == 0, AETH_E_LEN, "%s %zu is no multiple of the frame of %zu bytes", in_name, nin, in_frame);
    *F = nin / in_frame;
    AETH_REQUIRE(nout / out_frame == *F && nout % out_frame == 0, AETH_E_LEN, "%zu frames are %llu bytes of %s (%zu each), not %zu", *F,
                 (unsigned long long)aeth::mul_sat(*F, out_frame), out_name, out_frame, nout);
    return AETH_OK;
}

uint32_t lg_of(uint32_t r)
{
    uint32_t lg = 0;
    while ((1u << lg) < r) lg++;
    return lg;
}

}  // namespace

struct aeth_rs {
    aeth_ctx *ctx;
    rc::Code c;
    uint32_t lg;                        // lanes of a group: 1 << lg
    uint8_t *tab_dev;                   // exp[512], log[256], roots[64], gen[64]
    aeth::DevScratch slab;              // decode with a summary: one record per workgroup
};

namespace {

uint32_t slot_of(uint32_t r) { return 8 * (r + 1); }
size_t dec_lds(const aeth_rs *rs) { return ((((size_t)(kBlock >> rs->lg) * slot_of(rs->c.nroots)) + 3) & ~(size_t)3) + (size_t)(kBlock >> rs->lg) * 12; }

Geom geom_of(const aeth_rs *rs, uint64_t F, uint32_t depth)
{
    Geom g{};
    g.W = F * depth;
    g.m = rs->c.m; g.poly = rs->c.poly; g.N0 = (1u << rs->c.m) - 1; g.fcr = rs->c.fcr; g.prim = rs->c.prim;
    g.r = rs->c.nroots; g.n = rs->c.n; g.k = rs->c.n - rs->c.nroots;
    g.lg = rs->lg; g.depth = depth;
    return g;
}

}  // namespace

extern "C" {

int aeth_rs_named(const char *name, aeth_rs_code *code)
{
    AETH_REQUIRE(name && code, AETH_E_ARG, "null pointer");
    const rc::Named *n = rc::find_named(name);
    if (!n) {
        size_t cnt;
        const rc::Named *t = rc::named_table(&cnt);
        std::string known;
        for (size_t i = 0; i < cnt; i++) known += std::string(i ? ", " : "") + t[i].name;
        return aeth::set_error(AETH_E_ARG, "unknown RS code name \"%.40s\"; known: %s", name, known.c_str());
    }
    *code = aeth_rs_code{n->c.m, n->c.poly, n->c.fcr, n->c.prim, n->c.nroots, n->c.n};
    return AETH_OK;
}

int aeth_rs_generator(const aeth_rs_code *code, uint8_t *g_out, size_t ng)
{
    rc::Field f;
    int rv = check_code(code, f);
    if (rv) return rv;
    AETH_REQUIRE(ng >= (size_t)code->nroots + 1, AETH_E_LEN, "g has %u coefficients, g_out holds %zu", code->nroots + 1, ng);
    AETH_REQUIRE(g_out, AETH_E_ARG, "g_out is null");
    rc::generator(rc::tab_of(f, code_of(code)), g_out);
    return AETH_OK;
}

int aeth_rs_host_encode(const aeth_rs_code *code, const uint8_t *data_host, size_t ndata, uint32_t depth, uint8_t *coded_host, size_t ncoded)
{
    rc::Field f;
    int rv = check_code(code, f);
    if (rv) return rv;
    rv = check_depth(depth);
    if (rv) return rv;
    const size_t k = code->n - code->nroots;
    size_t F;
    rv = check_frames("ndata", ndata, depth * k, "coded symbols", ncoded, (size_t)depth * code->n, &F);
    if (rv) return rv;
    if (F == 0) return AETH_OK;
    AETH_REQUIRE(data_host && coded_host, AETH_E_ARG, "null pointer");
    if ((rv = aeth::check_disjoint({{data_host, ndata}}, {{coded_host, ncoded}}))) return rv;
    const rc::Tab t = rc::tab_of(f, code_of(code));
    uint8_t g[rc::kMaxRoots + 1];
    rc::generator(t, g);
    for (size_t fr = 0; fr < F; fr++) {
        const uint8_t *src = data_host + fr * depth * k;
        uint8_t *dst = coded_host + fr * depth * code->n;
        for (size_t b = 0; b < depth * k; b++) dst[b] = (uint8_t)(src[b] & t.N0);
        for (uint32_t i = 0; i < depth; i++) rc::encode_word(t, g, src + i, depth, dst + depth * k + i);
    }
    return AETH_OK;
}

int aeth_rs_host_decode(const aeth_rs_code *code, const uint8_t *in_host, size_t nin, const uint8_t *era_host, uint32_t depth, uint32_t flags,
                        uint8_t *out_host, size_t nout, aeth_rs_record *rec_host, aeth_rs_summary *summary_host)
{
    rc::Field f;
    int rv = check_code(code, f);
    if (rv) return rv;
    rv = check_depth(depth);
    if (rv) return rv;
    if ((rv = aeth::check_flags(flags, AETH_RS_PAYLOAD))) return rv;
    const uint32_t nb = (flags & AETH_RS_PAYLOAD) ? code->n - code->nroots : code->n;
    size_t F;
    rv = check_frames("nin", nin, (size_t)depth * code->n, "output", nout, (size_t)depth * nb, &F);
    if (rv) return rv;
    AETH_REQUIRE(!F || (in_host && out_host), AETH_E_ARG, "null pointer");
    if ((rv = aeth::check_disjoint({{in_host, nin}, {era_host, nin}}, {{out_host, nout}}))) return rv;
    const rc::Tab t = rc::tab_of(f, code_of(code));
    aeth_rs_summary sum{0, 0};
    for (size_t fr = 0; fr < F; fr++)
        for (uint32_t i = 0; i < depth; i++) {
            const size_t ib = fr * depth * code->n + i;
            const rc::Record r = rc::decode_word(t, in_host + ib, era_host ? era_host + ib : nullptr, depth, out_host + fr * depth * nb + i, depth, nb);
            if (rec_host) rec_host[fr * depth + i] = aeth_rs_record{r.corrected, r.status};
            sum.n_failed += r.status;
            sum.n_corrected += r.corrected;
        }
    if (summary_host) *summary_host = sum;
    return AETH_OK;
}

int aeth_rs_create(aeth_ctx *ctx, const aeth_rs_code *code, aeth_rs **out)
{
    AETH_REQUIRE(out, AETH_E_ARG, "out is null");
    *out = nullptr;
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    rc::Field f;
    int rv = check_code(code, f);
    if (rv) return rv;
    aeth_rs *rs = new (std::nothrow) aeth_rs{};
    AETH_REQUIRE(rs, AETH_E_NOMEM, "out of host memory");
    rs->ctx = ctx;
    rs->c = code_of(code);
    rs->lg = lg_of(rs->c.nroots);
    const rc::Tab t = rc::tab_of(f, rs->c);
    std::vector<uint8_t> tab(512 + 256 + 64 + 64, 0);
    std::copy(f.exp, f.exp + 512, tab.begin());
    std::copy(f.log, f.log + 256, tab.begin() + 512);
    uint8_t g[rc::kMaxRoots + 1];
    rc::generator(t, g);
    for (uint32_t q = 0; q < t.r; q++) {
        tab[768 + q] = (uint8_t)rc::beta_pow(t, (uint64_t)t.fcr + q);
        tab[832 + q] = g[t.r - 1 - q];
    }
    aeth::DeviceGuard dg(ctx->device);
    rv = aeth::upload_table(ctx, tab.data(), tab.size(), &rs->tab_dev, "aeth_rs_create: field tables");
    if (rv) { delete rs; return rv; }
    *out = rs;
    return AETH_OK;
}

int aeth_rs_destroy(aeth_rs *rs)
{
    if (!rs) return AETH_OK;
    const hipError_t freed = aeth::release_tables(rs->ctx, {rs->slab.p, rs->tab_dev});
    delete rs;
    return freed == hipSuccess ? AETH_OK : aeth::hip_fail(freed, "hipFree");
}

size_t aeth_rs_n(const aeth_rs *rs) { return rs ? rs->c.n : 0; }
size_t aeth_rs_k(const aeth_rs *rs) { return rs ? rs->c.n - rs->c.nroots : 0; }
uint32_t aeth_rs_nroots(const aeth_rs *rs) { return rs ? rs->c.nroots : 0; }
uint32_t aeth_rs_m(const aeth_rs *rs) { return rs ? rs->c.m : 0; }
uint32_t aeth_rs_group(const aeth_rs *rs) { return rs ? (uint32_t)kBlock >> rs->lg : 0; }
size_t aeth_rs_lds_bytes(const aeth_rs *rs, uint32_t depth) { return rs && depth >= 1 && depth <= rc::kMaxDepth ? dec_lds(rs) : 0; }

int aeth_rs_encode(aeth_rs *rs, const uint8_t *data_dev, size_t ndata, uint32_t depth, uint8_t *coded_dev, size_t ncoded)
{
    AETH_REQUIRE(rs, AETH_E_ARG, "rs is null");
    int rv = check_depth(depth);
    if (rv) return rv;
    const size_t k = rs->c.n - rs->c.nroots;
    size_t F;
    rv = check_frames("ndata", ndata, depth * k, "coded symbols", ncoded, (size_t)depth * rs->c.n, &F);
    if (rv) return rv;
    if (F == 0) return AETH_OK;
    AETH_REQUIRE(data_dev && coded_dev, AETH_E_ARG, "null pointer");
    if ((rv = aeth::check_disjoint({{data_dev, ndata}}, {{coded_dev, ncoded}}))) return rv;
    const Geom g = geom_of(rs, F, depth);
    const uint32_t G = (uint32_t)kBlock >> rs->lg;
    const uint64_t wgs = (g.W + G - 1) / G;
    if ((rv = aeth::check_grid(wgs, F, "frames"))) return rv;
    aeth::DeviceGuard dg(rs->ctx->device);
    hipStream_t st = aeth::ctx_stream(rs->ctx);
    EncCall a{g, data_dev, coded_dev, rs->tab_dev + 832};
    hipLaunchKernelGGL(rs_encode_kernel, dim3((unsigned)wgs), dim3(kBlock), 0, st, a);
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

int aeth_rs_decode(aeth_rs *rs, const uint8_t *in_dev, size_t nin, const uint8_t *era_dev, uint32_t depth, uint32_t flags, uint8_t *out_dev,
                   size_t nout, aeth_rs_record *rec_dev, aeth_rs_summary *summary_dev)
{
    AETH_REQUIRE(rs, AETH_E_ARG, "rs is null");
    int rv = check_depth(depth);
    if (rv) return rv;
    if ((rv = aeth::check_flags(flags, AETH_RS_PAYLOAD))) return rv;
    const uint32_t nb = (flags & AETH_RS_PAYLOAD) ? rs->c.n - rs->c.nroots : rs->c.n;
    size_t F;
    rv = check_frames("nin", nin, (size_t)depth * rs->c.n, "output", nout, (size_t)depth * nb, &F);
    if (rv) return rv;
    AETH_REQUIRE(!F || (in_dev && out_dev), AETH_E_ARG, "null pointer");
    AETH_REQUIRE(aeth::aligned4(rec_dev), AETH_E_ALIGN, "rec_dev not 4-byte aligned");
    AETH_REQUIRE(aeth::aligned8(summary_dev), AETH_E_ALIGN, "summary_dev not 8-byte aligned");
    const size_t nrec = aeth::mul_sat(aeth::mul_sat(F, depth), sizeof(aeth_rs_record));
    rv = aeth::check_disjoint({{in_dev, nin}, {era_dev, nin}}, {{out_dev, nout}, {rec_dev, nrec}, {summary_dev, sizeof(aeth_rs_summary)}});
    if (rv) return rv;
    if (F == 0 && !summary_dev) return AETH_OK;
    const Geom g = geom_of(rs, F, depth);
    const uint32_t G = (uint32_t)kBlock >> rs->lg;
    const uint64_t wgs = (g.W + G - 1) / G;
    if ((rv = aeth::check_grid(wgs, F, "frames"))) return rv;
    aeth::DeviceGuard dg(rs->ctx->device);
    Sum *sums = nullptr;
    if (summary_dev && wgs) {
        rv = aeth::scratch_ensure(rs->ctx, rs->slab, (size_t)wgs * sizeof(Sum));
        if (rv) return rv;
        sums = static_cast<Sum *>(rs->slab.p);
    }
    hipStream_t st = aeth::ctx_stream(rs->ctx);
    if (wgs) {
        DecCall a{};
        a.g = g;
        a.in = in_dev; a.era = era_dev; a.out = out_dev;
        a.rec = reinterpret_cast<rc::Record *>(rec_dev);
        a.sums = sums;
        a.tab = rs->tab_dev;
        a.nb = nb;
        a.slot = slot_of(rs->c.nroots);
        hipLaunchKernelGGL(rs_decode_kernel, dim3((unsigned)wgs), dim3(kBlock), dec_lds(rs), st, a);
    }
    if (summary_dev) hipLaunchKernelGGL(rs_summary_kernel, dim3(1), dim3(kBlock), 0, st, (const Sum *)sums, (size_t)wgs, reinterpret_cast<Sum *>(summary_dev));
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

}  // extern "C"
