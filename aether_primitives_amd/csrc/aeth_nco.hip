// aeth_nco.hip -- numerically controlled oscillator: frequency shift (mix), tone and chirp generated on the device
// (no body in the reference; definition in include/aether_hip.h, aeth_nco_*).  The phase of sample n is a 64-bit
// integer word, exact at every stream position; its phasor is a fixed sequence of rounded f32 operations
// (aeth_nco_core.h, shared with the host entry points).  Compiled with -ffp-contract=off like aeth_vecops.hip: the
// output is defined bit for bit, so the chunks of a stream concatenate exactly.
//
// HBM-streaming kernels in the launch shape aeth_vecops.hip measured as fastest: one 16-byte access (two samples) per
// lane where both pointers allow it, 8-byte otherwise, one tile per 256-lane workgroup, the grid covering the vector.
// No table and no LDS: a lane computes the phasors of its own samples.  The launch's first sample is the oscillator's
// origin (moved there on the host); a workgroup moves the origin to its tile with wave-uniform (scalar) arithmetic and a
// lane multiplies by an offset below 512.  RATE == false drops the chirp term from both.
#include "aeth_internal.h"
#include "aeth_nco_core.h"

#include <cmath>

namespace {

using aeth::nco::Phasor;
using aeth::nco::Words;

constexpr int kBlock = 256;

// the words of the lane's first sample and the first difference there: sample j + 1 is w + dw, the one after that
// w + 2 dw + rate
template <bool RATE, unsigned S> __device__ __forceinline__ void lane_words(const Words &base, uint64_t &w, uint64_t &dw)
{
    const uint64_t m = (uint64_t)blockIdx.x * (kBlock * S);               // wave-uniform: the tile's first sample
    const uint32_t j = threadIdx.x * S;
    if constexpr (RATE) {
        const Words t = aeth::nco::advance(base, m);
        w = t.phase + (uint64_t)j * t.step + (uint64_t)((j * (j - 1u)) >> 1) * t.rate;     // T(j) < 2^17
        dw = t.step + (uint64_t)j * t.rate;
    } else {
        w = base.phase + m * base.step + (uint64_t)j * base.step;
        dw = base.step;
    }
}

// V = float4 (two samples) or float2 (one sample); `in` may be `out` (in place): a lane reads only what it writes
template <typename V, bool NT, bool RATE>
__global__ __launch_bounds__(kBlock) void nco_mix_kernel(const V *in, V *out, size_t items, Words base)
{
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= items) return;
    const V x = aeth::nt_load<NT>(in + i);                                // in flight while the phasors are computed
    uint64_t w, dw;
    lane_words<RATE, sizeof(V) / 8>(base, w, dw);
    V r;
    aeth::nco::mix(x.x, x.y, aeth::nco::phasor(w), r.x, r.y);
    if constexpr (sizeof(V) == 16) aeth::nco::mix(x.z, x.w, aeth::nco::phasor(w + dw), r.z, r.w);
    aeth::nt_store<NT>(out + i, r);
}

template <typename V, bool NT, bool RATE>
__global__ __launch_bounds__(kBlock) void nco_tone_kernel(V *out, size_t items, Words base, float amp)
{
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= items) return;
    uint64_t w, dw;
    lane_words<RATE, sizeof(V) / 8>(base, w, dw);
    V r;
    const Phasor p = aeth::nco::phasor(w);
    r.x = amp * p.c; r.y = amp * p.d;
    if constexpr (sizeof(V) == 16) {
        const Phasor q = aeth::nco::phasor(w + dw);
        r.z = amp * q.c; r.w = amp * q.d;
    }
    aeth::nt_store<NT>(out + i, r);
}

// one launch over `cnt` samples that start `off` samples into the call
template <bool MIX, typename V>
void launch_part(aeth_ctx *ctx, const Words &w0, bool nt, const float2 *in, float2 *out, size_t off, size_t cnt, float amp)
{
    constexpr size_t S = sizeof(V) / sizeof(float2);
    const size_t items = cnt / S;
    const dim3 grid((unsigned)((items + kBlock - 1) / kBlock)), block(kBlock);
    const Words base = aeth::nco::advance(w0, off);
    const bool rate = base.rate != 0;
    hipStream_t st = aeth::ctx_stream(ctx);
    if constexpr (MIX) {
        auto k = nt ? (rate ? nco_mix_kernel<V, true, true> : nco_mix_kernel<V, true, false>)
                    : (rate ? nco_mix_kernel<V, false, true> : nco_mix_kernel<V, false, false>);
        hipLaunchKernelGGL(k, grid, block, 0, st, reinterpret_cast<const V *>(in + off), reinterpret_cast<V *>(out + off), items, base);
    } else {
        auto k = nt ? (rate ? nco_tone_kernel<V, true, true> : nco_tone_kernel<V, true, false>)
                    : (rate ? nco_tone_kernel<V, false, true> : nco_tone_kernel<V, false, false>);
        hipLaunchKernelGGL(k, grid, block, 0, st, reinterpret_cast<V *>(out + off), items, base, amp);
    }
}

// the split of a call into launches: (head, body, tail) samples on the 16-byte route, or everything on the 8-byte one
struct Split { bool wide; size_t head, body, tail; };

Split split_of(const void *in, const void *out, size_t n)
{
    const uintptr_t mo = reinterpret_cast<uintptr_t>(out) & 15u;
    const uintptr_t mi = in ? (reinterpret_cast<uintptr_t>(in) & 15u) : mo;
    if (mi != mo) return Split{false, 0, n, 0};
    const size_t head = mo != 0 ? 1 : 0, pairs = (n - head) / 2;
    return Split{true, head, 2 * pairs, (n - head) - 2 * pairs};
}

// what both device calls check, in this order, before any device work (`in` is NULL for the tone)
int check_call(aeth_ctx *ctx, const aeth_nco_words *w, uint64_t n0, bool mix, const aeth_cf32 *in, aeth_cf32 *out, size_t n, bool &run)
{
    run = false;
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    AETH_REQUIRE(w, AETH_E_ARG, "words is null");
    if (n == 0) return AETH_OK;
    AETH_REQUIRE(out && (in || !mix), AETH_E_ARG, "null pointer");
    AETH_REQUIRE(aeth::aligned8(out) && aeth::aligned8(in), AETH_E_ALIGN, "pointer not 8-byte aligned");
    AETH_REQUIRE(n0 <= UINT64_MAX - (uint64_t)n, AETH_E_UNSUPPORTED, "position %llu + %zu samples passes 2^64",
                 (unsigned long long)n0, n);
    const Split s = split_of(in, out, n);
    const size_t items = s.wide ? s.body / 2 : s.body;
    AETH_REQUIRE((items + kBlock - 1) / kBlock < ((size_t)1 << 31), AETH_E_UNSUPPORTED, "%zu samples need 2^31 workgroups or more", n);
    AETH_REQUIRE(!mix || in == out || !aeth::ranges_touch(in, n * sizeof(aeth_cf32), out, n * sizeof(aeth_cf32)), AETH_E_ARG,
                 "the output overlaps the input (only out == in runs in place)");
    run = true;
    return AETH_OK;
}

template <bool MIX>
int launch(aeth_ctx *ctx, const aeth_nco_words *words, uint64_t n0, float amp, const aeth_cf32 *in_dev, aeth_cf32 *out_dev, size_t n)
{
    aeth::DeviceGuard dev_guard(ctx->device);
    const float2 *in = reinterpret_cast<const float2 *>(in_dev);
    float2 *out = reinterpret_cast<float2 *>(out_dev);
    const Words w0 = aeth::nco::advance(Words{words->phase, words->step, words->rate}, n0);
    const bool nt = aeth::streams_past_cache(n * sizeof(float2) * (MIX ? 2 : 1));
    const Split s = split_of(in, out, n);
    if (s.wide) {
        // same phase: peel one sample if the base sits on an odd 8-byte slot, then the 16-byte body
        if (s.head) launch_part<MIX, float2>(ctx, w0, nt, in, out, 0, 1, amp);
        if (s.body) launch_part<MIX, float4>(ctx, w0, nt, in, out, s.head, s.body, amp);
        if (s.tail) launch_part<MIX, float2>(ctx, w0, nt, in, out, s.head + s.body, 1, amp);
    } else {
        launch_part<MIX, float2>(ctx, w0, nt, in, out, 0, n, amp);
    }
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

}  // namespace

extern "C" {

uint64_t aeth_nco_word(double cycles)
{
    if (!std::isfinite(cycles)) return 0;
    const double x = cycles - std::floor(cycles);              // in [0, 1]: a tiny negative number rounds to 1.0
    if (!(x < 1.0)) return 0;
    return (uint64_t)(x * 18446744073709551616.0);             // the scaling by 2^64 is exact; truncated toward zero
}

uint64_t aeth_nco_word_at(const aeth_nco_words *w, uint64_t n)
{
    if (!w) return 0;
    return aeth::nco::word_at(Words{w->phase, w->step, w->rate}, n);
}

int aeth_nco_phasor(uint64_t word, aeth_cf32 *out_host)
{
    AETH_REQUIRE(out_host, AETH_E_ARG, "out is null");
    const Phasor p = aeth::nco::phasor(word);
    out_host->re = p.c;
    out_host->im = p.d;
    return AETH_OK;
}

int aeth_nco_mix(aeth_ctx *ctx, const aeth_nco_words *w, uint64_t n0, const aeth_cf32 *in_dev, aeth_cf32 *out_dev, size_t n)
{
    bool run;
    int rc = check_call(ctx, w, n0, true, in_dev, out_dev, n, run); if (rc || !run) return rc;
    return launch<true>(ctx, w, n0, 0.f, in_dev, out_dev, n);
}

int aeth_nco_tone(aeth_ctx *ctx, const aeth_nco_words *w, uint64_t n0, float amp, aeth_cf32 *out_dev, size_t n)
{
    bool run;
    int rc = check_call(ctx, w, n0, false, nullptr, out_dev, n, run); if (rc || !run) return rc;
    return launch<false>(ctx, w, n0, amp, nullptr, out_dev, n);
}

}  // extern "C"
