// aeth_sync.hip -- feed-forward synchronisation estimators over a device-resident stream (no body in the reference;
// definition in include/aether_hip.h, aeth_sync_*): the spectral line of a non-linearity of the samples (square law:
// symbol timing after Oerder and Meyr; M-th power: carrier phase) and the delay-and-multiply sum of the M-th power
// (carrier frequency).  Read-only reductions, 8 B per sample, in the shape of aeth_vec_stats (aeth_stats.hip): f64 sums,
// no floating-point atomics, the order of the additions a function of the index inside the block and of the block's
// length only.  The phasor is the oscillator's (aeth_nco_core.h), q() is aeth_levels.h's.  Compiled with
// -ffp-contract=off: the f32 powers are defined one rounding per operation.
//
// THE ORDER.  A block of `len` samples is cut into chunks of 4096 (aeth_sync_chunk), the last one short; one workgroup
// of 256 lanes per chunk.  Inside a chunk of `left` samples the pairs (2 p, 2 p + 1) with 2 p + 1 < left belong to
// lane p % 256, round p / 256; when `left` is odd its last sample belongs to lane ((left - 1) / 2) % 256.
//   a lane starts each sum from -0.0 (the identity of IEEE addition: the sum of ONE term is that term, sign of zero
//   included) and adds the terms of its pairs in round order, first sample then second, then the odd last sample if it
//   owns it: ascending index.  A term that does not exist (a lag term in front of the call without history) is skipped;
//   the 256 lanes' sums become the chunk's record, the chunk records the block's, the block records the total by THE TREE
//   of aeth_reduce.h (a + b == b + a bit for bit), every fold from -0.0; a block of one chunk is done with its chunk.
// A record without terms is written as +0.0 sums (only the records handed out; chunk records keep the identity).
// Neither the CU count, nor the pointer's alignment (16-byte buffer loads at ANY 8-byte-aligned base, so there is no
// head / body / tail split), nor the non-temporal choice enters.
//
// Loads go through a buffer descriptor over the chunk's valid range: a pair past the end gets an offset out of range and
// comes back as zeros without a branch, so every load of a lane is issued before the first use and the compiler can
// count them.  The lag kernel reads x[i - L] the same way; only the chunks that reach in front of the call (uniform
// per workgroup) read one sample per load from the history or from x, the address chosen by a select.
#include "aeth_internal.h"
#include "aeth_levels.h"
#include "aeth_nco_core.h"
#include "aeth_reduce.h"

#include <cmath>

namespace {

using aeth::FastDiv;
using aeth::nco::Phasor;
using aeth::nco::Words;
using aeth::red::Cut;
using aeth::red::Geo;

typedef aeth_sync_record Rec;
static_assert(sizeof(Rec) == 48, "record layout");

constexpr int kBlock = aeth::red::kBlock;
constexpr int kItems = 8;                                            // 16-byte loads (two samples) per lane
constexpr unsigned kChunk = kBlock * kItems * 2;                     // 4096 samples, 32 KiB per workgroup
constexpr int kFar = 0x7ffffff0;                                     // an offset no descriptor here covers
constexpr size_t kMaxLag = (size_t)1 << 20;

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct Cf { float re, im; };

// the definition's sq(): every product and the difference rounded on their own
__device__ __forceinline__ Cf sq(Cf a)
{
    const float p = a.re * a.im;
    return Cf{a.re * a.re - a.im * a.im, p + p};
}
template <int M> __device__ __forceinline__ Cf pw(Cf x)
{
    static_assert(M == 1 || M == 2 || M == 4 || M == 8, "power");
    if constexpr (M == 1) return x;
    else return sq(pw<M / 2>(x));
}

__device__ __forceinline__ Rec rec_identity()
{
    Rec r;
    r.re = -0.0; r.im = -0.0; r.mass = -0.0; r.n = 0; r.n_nonfinite = 0; r.reserved = 0;
    return r;
}
__device__ __forceinline__ Rec rec_combine(const Rec &a, const Rec &b)
{
    Rec r;
    r.re = a.re + b.re; r.im = a.im + b.im; r.mass = a.mass + b.mass;
    r.n = a.n + b.n; r.n_nonfinite = a.n_nonfinite + b.n_nonfinite; r.reserved = 0;
    return r;
}
// a record that is handed out: no terms -> +0.0 sums
__device__ __forceinline__ Rec rec_public(Rec a)
{
    if (a.n == 0) { a.re = 0.0; a.im = 0.0; a.mass = 0.0; }
    return a;
}

// one term into the lane's sums; `live` false adds the identity
__device__ __forceinline__ void take(Rec &a, double tre, double tim, double wt, bool live)
{
    a.re += live ? tre : -0.0;
    a.im += live ? tim : -0.0;
    a.mass += live ? wt : -0.0;
    a.n += live ? 1u : 0u;
    const bool fin = __builtin_isfinite(tre) && __builtin_isfinite(tim);
    a.n_nonfinite += (live && !fin) ? 1u : 0u;
}

template <int KIND, bool ZERO>
__device__ __forceinline__ void line_term(Rec &a, float xr, float xi, uint64_t w, bool live)
{
    double c = 1.0, d = 0.0;                                         // the phasor of the word 0, exactly
    if constexpr (!ZERO) {
        const Phasor p = aeth::nco::phasor(w);
        c = (double)p.c; d = (double)p.d;
    }
    if constexpr (KIND == AETH_SYNC_SQUARE) {
        const double f = aeth::level_q(xr, xi);
        take(a, f * c, f * d, f, live);
    } else {
        const Cf z = pw<KIND>(Cf{xr, xi});
        const double zr = (double)z.re, zi = (double)z.im;           // products of two f32 values: exact, one rounding each line
        take(a, zr * c - zi * d, zr * d + zi * c, aeth::level_q(z.re, z.im), live);
    }
}

template <int M>
__device__ __forceinline__ void lag_term(Rec &acc, float xr, float xi, float pr, float pi, bool live)
{
    const Cf a = pw<M>(Cf{xr, xi}), b = pw<M>(Cf{pr, pi});
    const double ar = (double)a.re, ai = (double)a.im, br = (double)b.re, bi = (double)b.im;
    take(acc, ar * br + ai * bi, ai * br - ar * bi, aeth::level_q(a.re, a.im), live);
}

template <bool NT> __device__ __forceinline__ f32x4 ld16(__amdgpu_buffer_rsrc_t rs, int off)
{
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, NT ? 2 : 0));
}
template <bool NT> __device__ __forceinline__ f32x2 ld8(__amdgpu_buffer_rsrc_t rs, int off)
{
    return __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, NT ? 2 : 0));
}

// the chunk's own samples: v[i] = the pair of round i (zeros when it is not whole inside the chunk), t = the odd last
// sample in the lane that owns it (zeros elsewhere)
template <bool NT>
__device__ __forceinline__ void load_chunk(const float2 *p, unsigned left, f32x4 (&v)[kItems], f32x2 &t, bool own_tail)
{
    auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float2 *>(p), 0, (int)(left * 8u), 0x00020000);
#pragma unroll
    for (int i = 0; i < kItems; i++) {
        const unsigned s0 = 2u * (unsigned)(i * kBlock + threadIdx.x);
        v[i] = ld16<NT>(rs, s0 + 1 < left ? (int)(s0 * 8u) : kFar);
    }
    t = ld8<NT>(rs, own_tail ? (int)((left - 1) * 8u) : kFar);
}

__device__ __forceinline__ void write_record(const Rec &a, Rec *out, const Geo &g, int direct)
{
    if (threadIdx.x == 0) {
        if (direct) out[g.b] = rec_public(a);                        // the block is this one chunk
        else out[blockIdx.x] = a;
    }
}

template <int KIND, bool NT, bool ZERO>
__global__ __launch_bounds__(kBlock) void sync_line_kernel(const float2 *__restrict__ x, size_t n, size_t block, FastDiv cpb,
                                                           Words base, Rec *__restrict__ out, int direct)
{
    __shared__ Rec lds[4];
    const Geo g = aeth::red::geo_of<kChunk>(n, block, cpb);
    const bool own_tail = (g.left & 1u) && threadIdx.x == (((g.left - 1) >> 1) & (kBlock - 1));
    f32x4 v[kItems];
    f32x2 t;
    load_chunk<NT>(x + g.g, g.left, v, t, own_tail);
    Words o = base;
    if constexpr (!ZERO) o = aeth::nco::advance(base, g.g);          // wave-uniform: the oscillator counted from the chunk
    auto word = [&](unsigned j) { return o.phase + (uint64_t)j * o.step + (uint64_t)((j * (j - 1u)) >> 1) * o.rate; };   // T(j) < 2^23
    Rec a = rec_identity();
#pragma unroll
    for (int i = 0; i < kItems; i++) {
        const unsigned s0 = 2u * (unsigned)(i * kBlock + threadIdx.x);
        const bool live = s0 + 1 < g.left;
        uint64_t w0 = 0, w1 = 0;
        if constexpr (!ZERO) { w0 = word(s0); w1 = w0 + o.step + (uint64_t)s0 * o.rate; }
        line_term<KIND, ZERO>(a, v[i].x, v[i].y, w0, live);
        line_term<KIND, ZERO>(a, v[i].z, v[i].w, w1, live);
    }
    {
        uint64_t w = 0;
        if constexpr (!ZERO) w = word(g.left - 1);
        line_term<KIND, ZERO>(a, t.x, t.y, w, own_tail);
    }
    a = aeth::red::block_reduce(a, lds, rec_combine);
    write_record(a, out, g, direct);
}

template <int M, bool NT>
__global__ __launch_bounds__(kBlock) void sync_lag_kernel(const float2 *__restrict__ x, const float2 *__restrict__ hist, size_t n,
                                                          size_t block, FastDiv cpb, size_t lag, Rec *__restrict__ out, int direct)
{
    __shared__ Rec lds[4];
    const Geo g = aeth::red::geo_of<kChunk>(n, block, cpb);
    const bool own_tail = (g.left & 1u) && threadIdx.x == (((g.left - 1) >> 1) & (kBlock - 1));
    f32x4 v[kItems], p[kItems];
    f32x2 t, pt;
    load_chunk<NT>(x + g.g, g.left, v, t, own_tail);
    unsigned first = 0;                                              // the chunk's first sample that has a term
    if (g.g >= lag) {
        load_chunk<NT>(x + (g.g - lag), g.left, p, pt, own_tail);    // every partner lies in x
    } else {
        // the chunk reaches in front of the call: sample s < hb pairs with hist[g + s], the others with x[s - hb].  One
        // 8-byte load per sample from an address chosen per lane (a select, no branch); a sample without a partner reads
        // the chunk's own first sample and its term is dropped below
        const unsigned hb = lag - g.g < g.left ? (unsigned)(lag - g.g) : g.left;
        if (!hist) first = hb;
        const float2 *safe = x + g.g, *hp = hist ? hist + g.g : safe;
        auto one = [&](unsigned s, bool in) {
            const float2 *q = s < hb ? hp + s : x + (s - hb);
            return __builtin_bit_cast(f32x2, aeth::nt_load<NT>(in ? q : safe));
        };
#pragma unroll
        for (int i = 0; i < kItems; i++) {
            const unsigned s0 = 2u * (unsigned)(i * kBlock + threadIdx.x);
            const bool in = s0 + 1 < g.left;
            const f32x2 lo = one(s0, in), hi = one(s0 + 1, in);
            p[i].x = lo.x; p[i].y = lo.y; p[i].z = hi.x; p[i].w = hi.y;
        }
        pt = one(g.left - 1, own_tail);
    }
    Rec a = rec_identity();
#pragma unroll
    for (int i = 0; i < kItems; i++) {
        const unsigned s0 = 2u * (unsigned)(i * kBlock + threadIdx.x);
        const bool live = s0 + 1 < g.left;
        lag_term<M>(a, v[i].x, v[i].y, p[i].x, p[i].y, live && s0 >= first);
        lag_term<M>(a, v[i].z, v[i].w, p[i].z, p[i].w, live && s0 + 1 >= first);
    }
    lag_term<M>(a, t.x, t.y, pt.x, pt.y, own_tail && g.left - 1 >= first);
    a = aeth::red::block_reduce(a, lds, rec_combine);
    write_record(a, out, g, direct);
}

// workgroup b folds in[b * per .. min((b + 1) * per, total)) into out[b]
__global__ __launch_bounds__(kBlock) void sync_fold_kernel(const Rec *__restrict__ in, size_t per, size_t total, Rec *__restrict__ out)
{
    __shared__ Rec lds[4];
    const Rec a = aeth::red::fold(in, per, total, rec_identity(), lds, rec_combine);
    if (threadIdx.x == 0) out[blockIdx.x] = rec_public(a);
}

// what both device calls check, in this order, before any device work
int check_call(const aeth_cf32 *hist_dev, size_t lag, const aeth_cf32 *x_dev, size_t n, size_t block,
               const aeth_sync_record *rec_dev, const aeth_sync_record *total_host, Cut &c)
{
    AETH_REQUIRE(x_dev, AETH_E_ARG, "x is null");
    AETH_REQUIRE(aeth::aligned8(x_dev) && aeth::aligned8(hist_dev) && aeth::aligned8(rec_dev) && aeth::aligned8(total_host), AETH_E_ALIGN,
                 "pointer not 8-byte aligned");
    AETH_REQUIRE(aeth::red::cut_of(n, block, kChunk, c), AETH_E_UNSUPPORTED, "%zu samples in blocks of %zu need 2^31 workgroups or more", n, block);
    AETH_REQUIRE(!aeth::ranges_touch(rec_dev, c.nb * sizeof(Rec), x_dev, n * sizeof(aeth_cf32)) &&
                 !aeth::ranges_touch(rec_dev, c.nb * sizeof(Rec), hist_dev, lag * sizeof(aeth_cf32)), AETH_E_ARG,
                 "the records overlap the input (or its history)");
    return AETH_OK;
}

// behind the chunk kernel (`launch`): the per-block fold and the total
template <class L>
int run(aeth_ctx *ctx, const Cut &c, aeth_sync_record *rec_dev, aeth_sync_record *total_host, L launch)
{
    return aeth::red::run_blocks(ctx, ctx->sync_slab, c, rec_dev, total_host,
                                 [](hipStream_t s, unsigned nwg, const Rec *in, size_t per, size_t total, Rec *out) {
                                     hipLaunchKernelGGL(sync_fold_kernel, dim3(nwg), dim3(kBlock), 0, s, in, per, total, out);
                                 }, launch);
}

template <int KIND> auto line_kernel_of(bool nt, bool zero)
{
    return nt ? (zero ? sync_line_kernel<KIND, true, true> : sync_line_kernel<KIND, true, false>)
              : (zero ? sync_line_kernel<KIND, false, true> : sync_line_kernel<KIND, false, false>);
}
template <int M> auto lag_kernel_of(bool nt) { return nt ? sync_lag_kernel<M, true> : sync_lag_kernel<M, false>; }

inline bool power_ok(int m) { return m == 1 || m == 2 || m == 4 || m == 8; }

}  // namespace

extern "C" {

size_t aeth_sync_chunk(void) { return kChunk; }

int aeth_sync_line(aeth_ctx *ctx, int kind, const aeth_nco_words *w, uint64_t n0, const aeth_cf32 *x_dev, size_t n, size_t block,
                   aeth_sync_record *rec_dev, aeth_sync_record *total_host)
{
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    AETH_REQUIRE(rec_dev || total_host, AETH_E_ARG, "both outputs are null");
    AETH_REQUIRE(n != 0, AETH_E_LEN, "a spectral line of an empty vector");
    AETH_REQUIRE(kind == AETH_SYNC_SQUARE || power_ok(kind), AETH_E_ARG, "bad line kind %d", kind);
    Cut c;
    int rc = check_call(nullptr, 0, x_dev, n, block, rec_dev, total_host, c); if (rc) return rc;
    AETH_REQUIRE(n0 <= UINT64_MAX - (uint64_t)n, AETH_E_UNSUPPORTED, "position %llu + %zu samples passes 2^64", (unsigned long long)n0, n);
    const bool zero = !w || (w->phase == 0 && w->step == 0 && w->rate == 0);
    const Words base = zero ? Words{0, 0, 0} : aeth::nco::advance(Words{w->phase, w->step, w->rate}, n0);
    const bool nt = aeth::streams_past_cache(n * sizeof(float2));
    const float2 *x = reinterpret_cast<const float2 *>(x_dev);
    const FastDiv cpb = aeth::make_fastdiv((uint32_t)c.cpb);
    return run(ctx, c, rec_dev, total_host, [&](hipStream_t s, Rec *out, int direct) {
        auto go = [&](auto k) { hipLaunchKernelGGL(k, dim3((unsigned)c.nwg), dim3(kBlock), 0, s, x, n, c.block, cpb, base, out, direct); };
        switch (kind) {
        case AETH_SYNC_SQUARE: go(line_kernel_of<AETH_SYNC_SQUARE>(nt, zero)); break;
        case AETH_SYNC_POW1: go(line_kernel_of<AETH_SYNC_POW1>(nt, zero)); break;
        case AETH_SYNC_POW2: go(line_kernel_of<AETH_SYNC_POW2>(nt, zero)); break;
        case AETH_SYNC_POW4: go(line_kernel_of<AETH_SYNC_POW4>(nt, zero)); break;
        default: go(line_kernel_of<AETH_SYNC_POW8>(nt, zero)); break;
        }
    });
}

int aeth_sync_lag(aeth_ctx *ctx, int power, size_t lag, const aeth_cf32 *hist_dev, const aeth_cf32 *x_dev, size_t n, size_t block,
                  aeth_sync_record *rec_dev, aeth_sync_record *total_host)
{
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    AETH_REQUIRE(rec_dev || total_host, AETH_E_ARG, "both outputs are null");
    AETH_REQUIRE(n != 0, AETH_E_LEN, "a lag sum of an empty vector");
    AETH_REQUIRE(power_ok(power), AETH_E_ARG, "bad power %d", power);
    AETH_REQUIRE(lag >= 1 && lag <= kMaxLag, AETH_E_ARG, "lag %zu is not in 1 .. 2^20", lag);
    Cut c;
    int rc = check_call(hist_dev, lag, x_dev, n, block, rec_dev, total_host, c); if (rc) return rc;
    const bool nt = aeth::streams_past_cache(n * sizeof(float2));
    const float2 *x = reinterpret_cast<const float2 *>(x_dev), *hist = reinterpret_cast<const float2 *>(hist_dev);
    const FastDiv cpb = aeth::make_fastdiv((uint32_t)c.cpb);
    return run(ctx, c, rec_dev, total_host, [&](hipStream_t s, Rec *out, int direct) {
        auto go = [&](auto k) { hipLaunchKernelGGL(k, dim3((unsigned)c.nwg), dim3(kBlock), 0, s, x, hist, n, c.block, cpb, lag, out, direct); };
        switch (power) {
        case 1: go(lag_kernel_of<1>(nt)); break;
        case 2: go(lag_kernel_of<2>(nt)); break;
        case 4: go(lag_kernel_of<4>(nt)); break;
        default: go(lag_kernel_of<8>(nt)); break;
        }
    });
}

double aeth_sync_turns(const aeth_sync_record *r)
{
    if (!r || (r->re == 0.0 && r->im == 0.0)) return 0.0;
    return std::atan2(r->im, r->re) / 6.283185307179586476925286766559;
}

uint64_t aeth_sync_freq_step(const aeth_sync_record *r, int power, size_t lag)
{
    if (power <= 0 || lag == 0) return 0;
    return aeth_nco_word(-aeth_sync_turns(r) / ((double)power * (double)lag));
}

uint64_t aeth_sync_timing_phase(const aeth_sync_record *r, double sps)
{
    if (!(sps > 0.0) || !(sps <= 2147483648.0)) return 0;
    const double t = -aeth_sync_turns(r);
    if (!std::isfinite(t)) return 0;
    double f = t - std::floor(t);                                    // in [0, 1]: a tiny negative number rounds to 1.0
    if (!(f < 1.0)) f = 0.0;
    return (uint64_t)(f * sps * 4294967296.0);                       // the scaling by 2^32 is exact; truncated toward zero
}

}  // extern "C"
