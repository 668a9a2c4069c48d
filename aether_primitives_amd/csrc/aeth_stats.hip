// aeth_stats.hip -- numbers and levels out of a device-resident signal: aeth_vec_stats (the reference's open item
// "Add VecStats (f32, cf32): Min(index), Max(index), Mean(index), Power", README.md:90-91) and aeth_vec_levels (what
// util/plot.rs:65,127 does with every bin of a spectrum).  The arithmetic is aeth_levels.h; compiled with
// -ffp-contract=off like the other bit-exact kernels.
//
// aeth_vec_stats is REPRODUCIBLE BY CONSTRUCTION: no floating-point atomics, and the order in which the f64 sums are
// combined is a function of the element index and n only --
//   sample i belongs to chunk i / 8192 (one workgroup), inside it to item (i % 8192) / 2, lane = item % 256,
//   round = item / 256;
//   a lane adds its 16 items in round order (first sample, then second), starting from 0;
//   the 256 lanes' results become the chunk's record, written to a slab, and a second launch of ONE workgroup folds the
//   chunk records from 0, both by THE TREE of aeth_reduce.h (a + b == b + a bit for bit).
// Neither the CU count, nor the pointer's alignment (accesses are 16 bytes per lane at ANY 8-byte-aligned base: global
// memory takes dword-aligned wide accesses, so there is no head / body / tail split to reorder anything), nor the
// non-temporal choice enters.  min / max order by q (f64), ties to the lowest index: that choice is associative and
// commutative, so it does not depend on the tree at all.
#include "aeth_internal.h"
#include "aeth_levels.h"
#include "aeth_reduce.h"

#include <cmath>
#include <cstring>

namespace {

constexpr int kBlock = aeth::red::kBlock;
constexpr int kItems = 16;                                           // items (two samples, 16 bytes) per lane
constexpr size_t kChunk = (size_t)kBlock * kItems * 2;               // 8192 samples, 64 KiB per workgroup
constexpr unsigned long long kNone = ~0ull;

// 16 / 8 bytes per lane at 8- / 4-byte alignment
typedef float f4u __attribute__((ext_vector_type(4), aligned(8)));
typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));

// (the pointer types are spelled out: a deduced template parameter would drop the typedef's alignment)
template <bool NT> __device__ __forceinline__ f4u ld4(const float2 *p)                  // two samples
{
    const f4u *q = reinterpret_cast<const f4u *>(p);
    if constexpr (NT) return __builtin_nontemporal_load(q);
    else return *q;
}
template <bool NT> __device__ __forceinline__ float2 ld2(const float2 *p)               // one sample
{
    typedef float f2a __attribute__((ext_vector_type(2)));
    const f2a *q = reinterpret_cast<const f2a *>(p);
    f2a v;
    if constexpr (NT) v = __builtin_nontemporal_load(q);
    else v = *q;
    return make_float2(v.x, v.y);
}
template <bool NT> __device__ __forceinline__ void st2(float *p, float a, float b)      // two levels
{
    f2u *q = reinterpret_cast<f2u *>(p);
    f2u v; v.x = a; v.y = b;
    if constexpr (NT) __builtin_nontemporal_store(v, q);
    else *q = v;
}
template <bool NT> __device__ __forceinline__ void st1(float *p, float a)
{
    if constexpr (NT) __builtin_nontemporal_store(a, p);
    else *p = a;
}

// one partial result; also the slab record (64 bytes)
struct __attribute__((aligned(16))) Rec {
    double sre, sim, sq;
    unsigned long long nnan;
    double minq;
    unsigned long long mini;
    double maxq;
    unsigned long long maxi;
};
static_assert(sizeof(Rec) == 64, "slab record");

__device__ __forceinline__ Rec rec_identity()
{
    Rec r;
    r.sre = 0.0; r.sim = 0.0; r.sq = 0.0; r.nnan = 0;
    r.minq = __builtin_inf(); r.mini = kNone;
    r.maxq = -1.0; r.maxi = kNone;                                   // q >= 0 for every candidate
    return r;
}

// a (+) b: sums in this order; min / max by (q, index), NaN samples never entered
__device__ __forceinline__ Rec rec_combine(const Rec &a, const Rec &b)
{
    Rec r;
    r.sre = a.sre + b.sre; r.sim = a.sim + b.sim; r.sq = a.sq + b.sq;
    r.nnan = a.nnan + b.nnan;
    const bool bmin = b.minq < a.minq || (b.minq == a.minq && b.mini < a.mini);
    r.minq = bmin ? b.minq : a.minq; r.mini = bmin ? b.mini : a.mini;
    const bool bmax = b.maxq > a.maxq || (b.maxq == a.maxq && b.maxi < a.maxi);
    r.maxq = bmax ? b.maxq : a.maxq; r.maxi = bmax ? b.maxi : a.maxi;
    return r;
}

template <bool NT>
__global__ __launch_bounds__(kBlock) void stats_partial_kernel(const float2 *__restrict__ x, size_t n, Rec *__restrict__ slab)
{
    __shared__ Rec lds[4];
    const size_t base = (size_t)blockIdx.x * kChunk;
    const size_t left = n - base;                                    // >= 1: the grid is ceil(n / kChunk)
    const float2 *p = x + base;
    f4u v[kItems];
    // every load of the chunk goes out before the first use
    if (left >= kChunk) {
#pragma unroll
        for (int k = 0; k < kItems; k++) v[k] = ld4<NT>(p + 2 * (k * kBlock + threadIdx.x));
    } else {
#pragma unroll
        for (int k = 0; k < kItems; k++) {
            const size_t s0 = 2 * (size_t)(k * kBlock + threadIdx.x);
            v[k] = (f4u)(0.f);
            if (s0 + 1 < left) v[k] = ld4<NT>(p + 2 * (k * kBlock + threadIdx.x));
            else if (s0 < left) { const float2 t = ld2<NT>(p + s0); v[k].x = t.x; v[k].y = t.y; }
        }
    }
    double sre = 0.0, sim = 0.0, sq = 0.0, minq = __builtin_inf(), maxq = -1.0;
    unsigned nnan = 0, mini = ~0u, maxi = ~0u;                       // indices inside the chunk until the end
    auto take = [&](float re, float im, unsigned li) {
        const double q = aeth::level_q(re, im);
        sre += (double)re; sim += (double)im; sq += q;
        if (q != q) nnan++;                                          // q is NaN exactly when a component is
        else {
            if (q < minq || mini == ~0u) { minq = q; mini = li; }    // a lane's indices ascend: the first of equals stays
            if (q > maxq) { maxq = q; maxi = li; }
        }
    };
#pragma unroll
    for (int k = 0; k < kItems; k++) {
        const unsigned s0 = 2u * (unsigned)(k * kBlock + threadIdx.x);
        if (s0 < left) take(v[k].x, v[k].y, s0);
        if (s0 + 1 < left) take(v[k].z, v[k].w, s0 + 1);
    }
    Rec a;
    a.sre = sre; a.sim = sim; a.sq = sq; a.nnan = nnan;
    a.minq = minq; a.mini = mini == ~0u ? kNone : base + mini;
    a.maxq = maxq; a.maxi = maxi == ~0u ? kNone : base + maxi;
    a = aeth::red::block_reduce(a, lds, rec_combine);
    if (threadIdx.x == 0) slab[blockIdx.x] = a;
}

__global__ __launch_bounds__(kBlock) void stats_final_kernel(const Rec *__restrict__ slab, size_t nrec, Rec *__restrict__ out)
{
    __shared__ Rec lds[4];
    const Rec a = aeth::red::fold(slab, nrec, nrec, rec_identity(), lds, rec_combine);
    if (threadIdx.x == 0) *out = a;
}

// two samples per lane: one 16-byte load, one 8-byte store; an odd n ends in a lane with one sample
template <int KIND, bool NT>
__global__ __launch_bounds__(kBlock) void levels_kernel(const float2 *__restrict__ x, float *__restrict__ lv, size_t n)
{
    const size_t s0 = 2 * ((size_t)blockIdx.x * kBlock + threadIdx.x);
    if (s0 + 1 < n) {
        const f4u v = ld4<NT>(x + s0);
        st2<NT>(lv + s0, aeth::level_of<KIND>(v.x, v.y), aeth::level_of<KIND>(v.z, v.w));
    } else if (s0 < n) {
        const float2 v = ld2<NT>(x + s0);
        st1<NT>(lv + s0, aeth::level_of<KIND>(v.x, v.y));
    }
}

// x_dev: device-visible memory; io.buf[1] receives the final record (pinned host memory or the context's staging)
int stats_run(aeth_ctx *ctx, aeth::HostIO &io, const aeth_cf32 *x_dev, size_t n, struct aeth_vec_stats *out)
{
    const size_t nrec = (n + kChunk - 1) / kChunk;
    AETH_REQUIRE(nrec <= 0x7fffffffu, AETH_E_UNSUPPORTED, "%zu samples", n);
    int rc = aeth::scratch_ensure(ctx, ctx->stats_slab, nrec * sizeof(Rec)); if (rc) return rc;
    Rec *slab = static_cast<Rec *>(ctx->stats_slab.p);
    const float2 *x = reinterpret_cast<const float2 *>(x_dev);
    const bool nt = aeth::streams_past_cache(n * sizeof(float2));
    hipStream_t s = aeth::ctx_stream(ctx);
    if (nt) hipLaunchKernelGGL(stats_partial_kernel<true>, dim3((unsigned)nrec), dim3(kBlock), 0, s, x, n, slab);
    else hipLaunchKernelGGL(stats_partial_kernel<false>, dim3((unsigned)nrec), dim3(kBlock), 0, s, x, n, slab);
    hipLaunchKernelGGL(stats_final_kernel, dim3(1), dim3(kBlock), 0, s, (const Rec *)slab, nrec, static_cast<Rec *>(io.buf[1]));
    AETH_HIP(hipGetLastError());
    Rec r;
    rc = io.get(&r, 1, sizeof(Rec)); if (rc) return rc;
    out->n = n;
    out->n_nan = (size_t)r.nnan;
    out->min_index = r.mini == kNone ? n : (size_t)r.mini;
    out->max_index = r.maxi == kNone ? n : (size_t)r.maxi;
    out->min_norm = r.mini == kNone ? NAN : (float)std::sqrt(r.minq);            /* norm() of that sample: aeth_levels.h */
    out->max_norm = r.maxi == kNone ? NAN : (float)std::sqrt(r.maxq);
    out->mean_re = r.sre / (double)n;
    out->mean_im = r.sim / (double)n;
    out->power = r.sq / (double)n;
    return AETH_OK;
}

template <int KIND>
void launch_levels(aeth_ctx *ctx, const float2 *x, float *lv, size_t n, bool nt)
{
    const size_t blocks = ((n + 1) / 2 + kBlock - 1) / kBlock;
    if (nt) hipLaunchKernelGGL((levels_kernel<KIND, true>), dim3((unsigned)blocks), dim3(kBlock), 0, aeth::ctx_stream(ctx), x, lv, n);
    else hipLaunchKernelGGL((levels_kernel<KIND, false>), dim3((unsigned)blocks), dim3(kBlock), 0, aeth::ctx_stream(ctx), x, lv, n);
}

}  // namespace

extern "C" {

int aeth_vec_stats(aeth_ctx *ctx, const aeth_cf32 *x_dev, size_t n, struct aeth_vec_stats *out)
{
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    AETH_REQUIRE(out, AETH_E_ARG, "out is null");
    AETH_REQUIRE(n != 0, AETH_E_LEN, "statistics of an empty vector");
    AETH_REQUIRE(x_dev, AETH_E_ARG, "x is null");
    AETH_REQUIRE(aeth::aligned8(x_dev), AETH_E_ALIGN, "x not 8-byte aligned");
    aeth::DeviceGuard dev_guard(ctx->device);
    aeth::HostIO io;
    int rc = io.open(ctx, 0, sizeof(Rec)); if (rc) return rc;        // the pinned bounce buffer: the record lands in host memory
    return stats_run(ctx, io, x_dev, n, out);
}

int aeth_host_vec_stats(aeth_ctx *ctx, const aeth_cf32 *x_host, size_t n, struct aeth_vec_stats *out)
{
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    AETH_REQUIRE(out, AETH_E_ARG, "out is null");
    AETH_REQUIRE(n != 0, AETH_E_LEN, "statistics of an empty vector");
    AETH_REQUIRE(x_host, AETH_E_ARG, "x is null");
    aeth::DeviceGuard dev_guard(ctx->device);
    const size_t bytes = n * sizeof(aeth_cf32);
    aeth::HostIO io;
    int rc = io.open(ctx, bytes, sizeof(Rec)); if (rc) return rc;
    rc = io.put(0, x_host, bytes); if (rc) return rc;
    return stats_run(ctx, io, (const aeth_cf32 *)io.buf[0], n, out);
}

int aeth_vec_levels(aeth_ctx *ctx, const aeth_cf32 *x_dev, size_t n, int kind, float *levels_dev, size_t n_levels)
{
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    AETH_REQUIRE(aeth::level_kind_ok(kind), AETH_E_ARG, "bad level kind %d", kind);
    AETH_REQUIRE(n_levels == n, AETH_E_LEN, "Levels and samples must have same length");
    if (n == 0) return AETH_OK;
    AETH_REQUIRE(x_dev && levels_dev, AETH_E_ARG, "null pointer");
    AETH_REQUIRE(aeth::aligned8(x_dev), AETH_E_ALIGN, "x not 8-byte aligned");
    AETH_REQUIRE(aeth::aligned4(levels_dev), AETH_E_ALIGN, "levels not 4-byte aligned");
    AETH_REQUIRE(!aeth::ranges_touch(x_dev, n * sizeof(aeth_cf32), levels_dev, n * sizeof(float)), AETH_E_ARG, "levels overlaps x");
    AETH_REQUIRE((n + 1) / 2 / kBlock < 0x7fffffffu, AETH_E_UNSUPPORTED, "%zu samples", n);
    aeth::DeviceGuard dev_guard(ctx->device);
    const float2 *x = reinterpret_cast<const float2 *>(x_dev);
    const bool nt = aeth::streams_past_cache(n * (sizeof(float2) + sizeof(float)));
    switch (kind) {
    case AETH_LEVEL_NORM: launch_levels<AETH_LEVEL_NORM>(ctx, x, levels_dev, n, nt); break;
    case AETH_LEVEL_DB: launch_levels<AETH_LEVEL_DB>(ctx, x, levels_dev, n, nt); break;
    default: launch_levels<AETH_LEVEL_POWER_DB>(ctx, x, levels_dev, n, nt); break;
    }
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

}  // extern "C"
