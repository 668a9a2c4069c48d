// aeth_remap.hip -- rate matching: a periodic gather of bytes with a constant where nothing is gathered (no body in the
// reference; definition in include/aether_hip.h, aeth_remap_*).  Puncturing, depuncturing to erasures, block interleaving
// and any chain of them composed on the host are this one operation with one table:
//     out[q R_out + i] = map[i] < 0 ? fill : in[q R_in + map[i]]
// Bytes are never interpreted, so the output is defined byte for byte; compiled with the EXACT flags like the other
// bit-exact kernels.  The roofline is HBM at n_in + n_out bytes.
//
// Tile route (a tile of g >= 1 whole periods and its table fit kLdsBudget).  A workgroup stages the g R_in input bytes of
// a tile in LDS -- 16-byte loads over the aligned body, single bytes at the ragged ends -- and every lane then assembles
// 16 consecutive output bytes by LDS byte reads at table addresses and stores them with one 16-byte store; output bytes
// ahead of the first and behind the last 16-byte boundary go out singly.
//   Staging image.  Input byte j of the tile sits at pad(j + sh), sh = the tile's input address & 15, so that an aligned
//     16-byte chunk of global memory is four aligned dwords of LDS.  pad(J) = J + 4 (J / 128) skips one dword in 33:
//     lanes read bytes 16 apart when the map is the identity, i.e. dwords 4 apart, which would be 8 banks for the 32 lanes
//     of a ds_read group; with the skipped dword the 32 lanes meet 32 banks.  What conflicts remain come from the
//     permutation.  One more slot behind the image, pad(sh + g R_in), carries the fill byte: a -1 is a table entry that
//     points there, and needs no branch.
//   Table.  The object keeps, per output of a tile, the input offset inside the tile (or g R_in for the fill slot) as
//     uint16_t in device memory.  A workgroup turns it into LDS byte addresses once -- entry e = o + osh for output o,
//     osh = the tile's output address & 15, so that lane chunk m is the aligned 16 bytes of global memory -- and keeps it
//     while it walks over its tiles; g is a multiple of what makes g R_in and g R_out multiples of 16 where the budget
//     allows, so sh and osh are the same for every tile and the table is built once per workgroup.  Where it does not
//     (large odd periods) the table is rebuilt when sh or osh changes, by the same code.  The 16 entries of a chunk are two
//     ds_read_b128 in a layout [half][chunk][8], consecutive lanes reading consecutive 16 bytes.
//   The last, shorter tile and the partial period are the same code with the bounds len_in and len_out.
// Gather route (every other period up to 2^20).  One lane takes an aligned 16 bytes of output, walks (q, i) from one
// division, reads its table entries from global memory (int32_t, at most 4 MiB: L2-resident) and its inputs by byte loads.
// A whole chunk runs without a branch, so that its 16 table loads and then its 16 byte loads are in flight together (with
// a branch per byte the compiler waits for every load before it issues the next: 32 memory latencies in a row per lane).
#include "aeth_internal.h"

#include <algorithm>
#include <new>
#include <numeric>
#include <vector>

namespace {

constexpr int kBlock = 256;
constexpr uint32_t kLdsBudget = 32768;             // staging image + table of a tile: five workgroups share a CU's LDS
constexpr size_t kMaxPeriod = (size_t)1 << 20;
constexpr uint64_t kMaxLen = (uint64_t)1 << 32;

__host__ __device__ constexpr uint32_t pad(uint32_t j) { return j + ((j >> 7) << 2); }
// the staging image of t_in bytes at any sh <= 15, and the fill slot behind it
constexpr uint32_t stage_bytes(uint32_t t_in) { return (pad(t_in + 15) + 1 + 15) & ~15u; }
// 16-entry chunks of the LDS table of t_out outputs at any osh <= 15
constexpr uint32_t tab_chunks(uint32_t t_out) { return (t_out + 15 + 15) >> 4; }

struct TileCall {
    const uint8_t *in;
    uint8_t *out;
    const uint16_t *tab;       // [t_out]: input offset inside the tile, t_in for the fill slot
    uint64_t n_out, need;      // bytes to write; input bytes the call may read (aeth_remap_in_count)
    uint64_t ntiles;
    uint32_t t_in, t_out;      // g R_in, g R_out
    uint32_t tab_base;         // LDS offset of the table: stage_bytes(t_in)
    uint32_t fill;
};

template <bool NT> __global__ __launch_bounds__(kBlock) void remap_tile_kernel(TileCall a)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsBudget];
    const uint32_t tid = threadIdx.x;
    const uint32_t M = tab_chunks(a.t_out);
    uint16_t *ltab = reinterpret_cast<uint16_t *>(lds + a.tab_base);
    uint32_t have = ~0u;                                                  // sh | osh << 4 the LDS table holds
    for (uint64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const uint64_t i0 = tile * a.t_in, o0 = tile * a.t_out;
        const uint8_t *src = a.in + i0;
        uint8_t *dst = a.out + o0;
        const uint32_t len_in = (uint32_t)min((uint64_t)a.t_in, a.need - i0);
        const uint32_t len_out = (uint32_t)min((uint64_t)a.t_out, a.n_out - o0);
        const uint32_t sh = (uint32_t)(reinterpret_cast<uintptr_t>(src) & 15u), osh = (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u);
        __syncthreads();                                                  // the tile before has been read
        if ((sh | (osh << 4)) != have) {
            have = sh | (osh << 4);
            for (uint32_t e = tid; e < 16 * M; e += kBlock) {
                const uint32_t o = e - osh;                               // wraps below osh: no output
                const uint32_t j = o < a.t_out ? a.tab[o] : a.t_in;
                ltab[((e >> 3) & 1u) * 8 * M + (e >> 4) * 8 + (e & 7u)] = (uint16_t)pad(j + sh);
            }
        }
        const uint32_t end_in = sh + len_in;
        for (uint32_t J0 = tid << 4; J0 < end_in; J0 += kBlock << 4) {
            if (J0 >= sh && J0 + 16 <= end_in) {
                const uint4 v = aeth::nt_load<NT>(reinterpret_cast<const uint4 *>(src + (J0 - sh)));
                uint32_t *p = reinterpret_cast<uint32_t *>(lds + pad(J0));
                p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
            } else {
                for (uint32_t J = max(J0, sh); J < min(J0 + 16, end_in); J++) lds[pad(J)] = src[J - sh];
            }
        }
        if (tid == 0) lds[pad(sh + a.t_in)] = (uint8_t)a.fill;
        __syncthreads();

        const uint32_t end_out = osh + len_out;
        for (uint32_t e0 = tid << 4; e0 < end_out; e0 += kBlock << 4) {
            const uint32_t m = e0 >> 4;
            const uint4 ta = *reinterpret_cast<const uint4 *>(lds + a.tab_base + 16 * m);
            const uint4 tb = *reinterpret_cast<const uint4 *>(lds + a.tab_base + 16 * M + 16 * m);
            auto four = [&](uint32_t lo, uint32_t hi) {
                return (uint32_t)lds[lo & 0xffffu] | ((uint32_t)lds[lo >> 16] << 8) | ((uint32_t)lds[hi & 0xffffu] << 16) |
                       ((uint32_t)lds[hi >> 16] << 24);
            };
            const uint32_t w0 = four(ta.x, ta.y), w1 = four(ta.z, ta.w), w2 = four(tb.x, tb.y), w3 = four(tb.z, tb.w);
            if (e0 >= osh && e0 + 16 <= end_out) {
                aeth::nt_store<NT>(reinterpret_cast<uint4 *>(dst + (e0 - osh)), uint4{w0, w1, w2, w3});
            } else {
                auto bytes = [&](uint32_t w, uint32_t e) {
#pragma unroll
                    for (uint32_t k = 0; k < 4; k++)
                        if (e + k >= osh && e + k < end_out) dst[e + k - osh] = (uint8_t)(w >> (8 * k));
                };
                bytes(w0, e0); bytes(w1, e0 + 4); bytes(w2, e0 + 8); bytes(w3, e0 + 12);
            }
        }
    }
}

struct GatherCall {
    const uint8_t *in;
    uint8_t *out;
    const int32_t *map;        // [r_out]
    uint64_t n_out;
    uint32_t r_in, r_out;
    aeth::FastDiv div;         // by r_out
    uint32_t fill;
};

template <bool NT> __global__ __launch_bounds__(kBlock) void remap_gather_kernel(GatherCall a)
{
    const uint32_t osh = (uint32_t)(reinterpret_cast<uintptr_t>(a.out) & 15u);
    const uint64_t end_out = osh + a.n_out, nch = (end_out + 15) >> 4;
    for (uint64_t c = (uint64_t)blockIdx.x * kBlock + threadIdx.x; c < nch; c += (uint64_t)gridDim.x * kBlock) {
        const uint64_t e0 = c << 4;
        const uint32_t first = (uint32_t)(max(e0, (uint64_t)osh) - osh);  // the chunk's first output: below 2^32
        uint32_t q = aeth::fdiv(first, a.div), i = first - q * a.r_out;
        uint8_t *dst = a.out - osh + e0;                                  // 16-byte aligned
        if (e0 >= osh && e0 + 16 <= end_out) {
            // a whole chunk, without a branch: the 16 table entries are loaded together, then the 16 bytes (a -1 reads a
            // byte of the table instead, which is there whatever the input holds, and is replaced by the fill)
            int32_t t[16];
            uint32_t qq[16];
#pragma unroll
            for (int k = 0; k < 16; k++) {
                t[k] = a.map[i];
                qq[k] = q;
                const bool wrap = ++i == a.r_out;
                i = wrap ? 0u : i;
                q += wrap ? 1u : 0u;
            }
            uint32_t b[16];
#pragma unroll
            for (int k = 0; k < 16; k++) {
                const uint8_t *p = t[k] < 0 ? reinterpret_cast<const uint8_t *>(a.map) : a.in + ((uint64_t)qq[k] * a.r_in + (uint32_t)t[k]);
                b[k] = *p;
            }
            uint32_t w[4];
#pragma unroll
            for (int k = 0; k < 16; k += 4) {
                auto byte = [&](int kk) { return t[kk] < 0 ? a.fill : b[kk]; };
                w[k / 4] = byte(k) | (byte(k + 1) << 8) | (byte(k + 2) << 16) | (byte(k + 3) << 24);
            }
            aeth::nt_store<NT>(reinterpret_cast<uint4 *>(dst), uint4{w[0], w[1], w[2], w[3]});
            continue;
        }
        // the call's ragged first and last chunk, byte by byte
        for (uint32_t k = 0; k < 16; k++) {
            if (e0 + k < osh || e0 + k >= end_out) continue;
            const int32_t t = a.map[i];
            dst[k] = (uint8_t)(t < 0 ? a.fill : (uint32_t)a.in[(uint64_t)q * a.r_in + (uint32_t)t]);
            if (++i == a.r_out) { i = 0; q++; }
        }
    }
}

// the periods of a tile: the most that fit the budget, rounded down to a multiple of what makes both tile lengths
// multiples of 16 when that leaves any; 0: no tile fits
uint32_t tile_periods(size_t r_in, size_t r_out)
{
    auto fits = [&](uint64_t g) {
        const uint64_t t_in = g * r_in, t_out = g * r_out;
        return t_in < 65536 && t_out < 65536 && (uint64_t)stage_bytes((uint32_t)t_in) + 32ull * tab_chunks((uint32_t)t_out) <= kLdsBudget;
    };
    if (!fits(1)) return 0;
    uint64_t lo = 1, hi = kLdsBudget;                                     // fits(lo), !fits(hi)
    while (hi - lo > 1) {
        const uint64_t mid = (lo + hi) / 2;
        (fits(mid) ? lo : hi) = mid;
    }
    const uint64_t u = std::lcm<uint64_t>(16 / std::gcd<uint64_t>(r_in, 16), 16 / std::gcd<uint64_t>(r_out, 16));
    return (uint32_t)(lo >= u ? lo - lo % u : lo);
}

// a table's entries lie in [-1, r_in): else the position and the value are named
int check_map(const char *name, const int32_t *map, size_t r_out, size_t r_in)
{
    AETH_REQUIRE(map, AETH_E_ARG, "%s is null", name);
    AETH_REQUIRE(r_in >= 1 && r_in <= kMaxPeriod, AETH_E_ARG, "%s: input period %zu outside 1 .. 2^20", name, r_in);
    AETH_REQUIRE(r_out >= 1 && r_out <= kMaxPeriod, AETH_E_ARG, "%s: output period %zu outside 1 .. 2^20", name, r_out);
    for (size_t i = 0; i < r_out; i++)
        AETH_REQUIRE(map[i] >= -1 && (int64_t)map[i] < (int64_t)r_in, AETH_E_ARG, "%s[%zu] = %d outside -1 .. %zu", name, i, map[i], r_in - 1);
    return AETH_OK;
}

}  // namespace

struct aeth_remap {
    aeth_ctx *ctx;
    uint32_t r_in, r_out;
    uint32_t g;                      // periods per tile; 0: the gather route
    void *tab_dev;                   // tile route: uint16_t[g r_out]; gather route: int32_t[r_out]
    std::vector<uint32_t> reach;     // [r_out]: one more than the largest non-negative map[0 .. i], 0 if none
};

extern "C" {

int aeth_remap_create(aeth_ctx *ctx, const int32_t *map, size_t r_out, size_t r_in, aeth_remap **out)
{
    AETH_REQUIRE(out, AETH_E_ARG, "out is null");
    *out = nullptr;
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    int rc = check_map("map", map, r_out, r_in);
    if (rc) return rc;
    aeth_remap *rm = new (std::nothrow) aeth_remap{};
    AETH_REQUIRE(rm, AETH_E_NOMEM, "out of host memory");
    rm->ctx = ctx;
    rm->r_in = (uint32_t)r_in;
    rm->r_out = (uint32_t)r_out;
    rm->g = tile_periods(r_in, r_out);
    rm->tab_dev = nullptr;
    rm->reach.resize(r_out);
    uint32_t top = 0;
    for (size_t i = 0; i < r_out; i++) {
        if (map[i] >= 0) top = std::max(top, (uint32_t)map[i] + 1);
        rm->reach[i] = top;
    }
    aeth::DeviceGuard dg(ctx->device);
    if (rm->g) {
        const uint32_t t_in = rm->g * rm->r_in;
        std::vector<uint16_t> tab((size_t)rm->g * r_out);
        for (uint32_t p = 0; p < rm->g; p++)
            for (size_t i = 0; i < r_out; i++) tab[p * r_out + i] = (uint16_t)(map[i] < 0 ? t_in : p * rm->r_in + (uint32_t)map[i]);
        rc = aeth::upload_table(ctx, tab.data(), tab.size() * sizeof(uint16_t), &rm->tab_dev, "aeth_remap_create: tile table");
    } else {
        rc = aeth::upload_table(ctx, map, r_out * sizeof(int32_t), &rm->tab_dev, "aeth_remap_create: table");
    }
    if (rc) { delete rm; return rc; }
    *out = rm;
    return AETH_OK;
}

int aeth_remap_destroy(aeth_remap *rm)
{
    if (!rm) return AETH_OK;
    const hipError_t freed = aeth::release_tables(rm->ctx, {rm->tab_dev});
    delete rm;
    return freed == hipSuccess ? AETH_OK : aeth::hip_fail(freed, "hipFree");
}

size_t aeth_remap_in_period(const aeth_remap *rm) { return rm ? rm->r_in : 0; }
size_t aeth_remap_out_period(const aeth_remap *rm) { return rm ? rm->r_out : 0; }
int aeth_remap_route(const aeth_remap *rm) { return !rm ? 0 : rm->g ? AETH_REMAP_ROUTE_TILE : AETH_REMAP_ROUTE_GATHER; }
size_t aeth_remap_tile(const aeth_remap *rm) { return rm ? rm->g : 0; }

size_t aeth_remap_in_count(const aeth_remap *rm, size_t n_out)
{
    if (!rm) return 0;
    const size_t q = n_out / rm->r_out, rem = n_out % rm->r_out;
    if (q > (SIZE_MAX - rm->r_in) / rm->r_in) return SIZE_MAX;
    return q * rm->r_in + (rem ? rm->reach[rem - 1] : 0);
}

int aeth_remap_exec(aeth_remap *rm, const void *in_dev, size_t n_in, void *out_dev, size_t n_out, uint8_t fill)
{
    AETH_REQUIRE(rm, AETH_E_ARG, "rm is null");
    AETH_REQUIRE((uint64_t)n_out < kMaxLen, AETH_E_UNSUPPORTED, "n_out %zu: 2^32 or more in one call (cut the stream at a period)", n_out);
    AETH_REQUIRE((uint64_t)n_in < kMaxLen, AETH_E_UNSUPPORTED, "n_in %zu: 2^32 or more in one call (cut the stream at a period)", n_in);
    const size_t need = aeth_remap_in_count(rm, n_out);
    AETH_REQUIRE(n_in >= need, AETH_E_LEN, "input holds %zu bytes, %zu outputs read %zu", n_in, n_out, need);
    if (n_out == 0) return AETH_OK;
    AETH_REQUIRE(out_dev && (in_dev || need == 0), AETH_E_ARG, "null pointer");
    if (int rc = aeth::check_disjoint({{in_dev, n_in}}, {{out_dev, n_out}})) return rc;
    aeth::DeviceGuard dg(rm->ctx->device);
    const bool nt = aeth::streams_past_cache(need + n_out);
    hipStream_t st = aeth::ctx_stream(rm->ctx);
    const size_t cus = (size_t)std::max(rm->ctx->num_cus, 1);
    if (rm->g) {
        TileCall a{};
        a.in = static_cast<const uint8_t *>(in_dev);
        a.out = static_cast<uint8_t *>(out_dev);
        a.tab = static_cast<const uint16_t *>(rm->tab_dev);
        a.n_out = n_out;
        a.need = need;
        a.t_in = rm->g * rm->r_in;
        a.t_out = rm->g * rm->r_out;
        a.ntiles = (n_out + a.t_out - 1) / a.t_out;
        a.tab_base = stage_bytes(a.t_in);
        a.fill = fill;
        const dim3 grid((unsigned)std::min<uint64_t>(a.ntiles, cus * 4)), block(kBlock);
        if (nt) hipLaunchKernelGGL(remap_tile_kernel<true>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(remap_tile_kernel<false>, grid, block, 0, st, a);
    } else {
        GatherCall a{};
        a.in = static_cast<const uint8_t *>(in_dev);
        a.out = static_cast<uint8_t *>(out_dev);
        a.map = static_cast<const int32_t *>(rm->tab_dev);
        a.n_out = n_out;
        a.r_in = rm->r_in;
        a.r_out = rm->r_out;
        a.div = aeth::make_fastdiv(rm->r_out);
        a.fill = fill;
        const uint64_t blocks = ((n_out + 15 + 15) / 16 + kBlock - 1) / kBlock;
        const dim3 grid((unsigned)std::min<uint64_t>(blocks, cus * 8)), block(kBlock);
        if (nt) hipLaunchKernelGGL(remap_gather_kernel<true>, grid, block, 0, st, a);
        else hipLaunchKernelGGL(remap_gather_kernel<false>, grid, block, 0, st, a);
    }
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

/* ---- host-only table builders: integer arithmetic, no context ---- */

int aeth_remap_puncture(const uint8_t *keep, size_t p, int32_t *map, size_t cap, size_t *r_out)
{
    AETH_REQUIRE(keep && map && r_out, AETH_E_ARG, "null pointer");
    AETH_REQUIRE(p >= 1 && p <= kMaxPeriod, AETH_E_ARG, "period %zu outside 1 .. 2^20", p);
    size_t n = 0;
    for (size_t i = 0; i < p; i++) n += keep[i] & 1u;
    AETH_REQUIRE(n > 0, AETH_E_ARG, "keep sends none of its %zu bits", p);
    AETH_REQUIRE(cap >= n, AETH_E_LEN, "map holds %zu entries, the pattern keeps %zu", cap, n);
    size_t o = 0;
    for (size_t i = 0; i < p; i++)
        if (keep[i] & 1u) map[o++] = (int32_t)i;
    *r_out = n;
    return AETH_OK;
}

int aeth_remap_invert(const int32_t *map, size_t r_out, size_t r_in, int32_t *inv)
{
    AETH_REQUIRE(inv, AETH_E_ARG, "inv is null");
    int rc = check_map("map", map, r_out, r_in);
    if (rc) return rc;
    for (size_t j = 0; j < r_in; j++) inv[j] = -1;
    for (size_t i = r_out; i-- > 0;)
        if (map[i] >= 0) inv[map[i]] = (int32_t)i;
    return AETH_OK;
}

int aeth_remap_compose(const int32_t *a, size_t a_out, size_t a_in, const int32_t *b, size_t b_out, size_t b_in, int32_t *map, size_t cap,
                       size_t *r_out, size_t *r_in)
{
    AETH_REQUIRE(map && r_out && r_in, AETH_E_ARG, "null pointer");
    int rc = check_map("a", a, a_out, a_in);
    if (rc) return rc;
    rc = check_map("b", b, b_out, b_in);
    if (rc) return rc;
    const uint64_t m = std::lcm<uint64_t>(a_out, b_in);                   // below 2^40
    const uint64_t ri = a_in * (m / a_out), ro = b_out * (m / b_in);      // below 2^60
    AETH_REQUIRE(ri <= kMaxPeriod && ro <= kMaxPeriod, AETH_E_UNSUPPORTED, "composed periods %llu in, %llu out: above 2^20",
                 (unsigned long long)ri, (unsigned long long)ro);
    AETH_REQUIRE(cap >= ro, AETH_E_LEN, "map holds %zu entries, the composition has %llu", cap, (unsigned long long)ro);
    for (uint64_t i = 0; i < ro; i++) {
        const int32_t t = b[i % b_out];
        int32_t v = -1;
        if (t >= 0) {
            const uint64_t mid = (i / b_out) * b_in + (uint64_t)t;
            const int32_t s = a[mid % a_out];
            if (s >= 0) v = (int32_t)((mid / a_out) * a_in + (uint64_t)s);
        }
        map[i] = v;
    }
    *r_out = (size_t)ro;
    *r_in = (size_t)ri;
    return AETH_OK;
}

int aeth_remap_rows_cols(size_t rows, size_t cols, int32_t *map)
{
    AETH_REQUIRE(map, AETH_E_ARG, "map is null");
    AETH_REQUIRE(rows >= 1 && rows <= kMaxPeriod, AETH_E_ARG, "rows %zu outside 1 .. 2^20", rows);
    AETH_REQUIRE(cols >= 1 && cols <= kMaxPeriod, AETH_E_ARG, "cols %zu outside 1 .. 2^20", cols);
    AETH_REQUIRE(rows * cols <= kMaxPeriod, AETH_E_ARG, "%zu rows x %zu cols = %zu: above 2^20", rows, cols, rows * cols);
    for (size_t c = 0; c < cols; c++)
        for (size_t r = 0; r < rows; r++) map[c * rows + r] = (int32_t)(r * cols + c);
    return AETH_OK;
}

int aeth_remap_bicm16(size_t n_cbps, size_t n_bpsc, int32_t *map)
{
    AETH_REQUIRE(map, AETH_E_ARG, "map is null");
    AETH_REQUIRE(n_bpsc >= 1 && n_bpsc <= kMaxPeriod, AETH_E_ARG, "n_bpsc %zu outside 1 .. 2^20", n_bpsc);
    AETH_REQUIRE(n_cbps >= 1 && n_cbps <= kMaxPeriod, AETH_E_ARG, "n_cbps %zu outside 1 .. 2^20", n_cbps);
    const size_t s = std::max<size_t>(n_bpsc / 2, 1);
    AETH_REQUIRE(n_cbps % (16 * s) == 0, AETH_E_ARG, "n_cbps %zu is no multiple of 16 s = %zu (n_bpsc %zu)", n_cbps, 16 * s, n_bpsc);
    AETH_REQUIRE(n_cbps % n_bpsc == 0, AETH_E_ARG, "n_cbps %zu is no multiple of n_bpsc %zu", n_cbps, n_bpsc);
    for (size_t k = 0; k < n_cbps; k++) {
        const size_t i = (n_cbps / 16) * (k % 16) + k / 16;
        const size_t j = s * (i / s) + (i + n_cbps - (16 * i) / n_cbps) % s;
        map[j] = (int32_t)k;
    }
    return AETH_OK;
}

}  // extern "C"
