// aeth_resamp.hip -- polyphase rational resampler: up U (zero stuffing), real FIR h, down Q, in one pass (the reference's
// rate changes are linear interpolation and sample picking: src/sampling.rs:7-62).
// out[k] = sum over p = 0 .. P - 1 ascending of h[p U + r] * s[a - p], a = floor(k Q / U), r = (k Q) mod U, every product
// and every sum rounded (EXACT flags), the sum started from the p = 0 product.  The taps lie phase-major on the device,
// g[r][p] = h[p U + r], rows padded to a multiple of four floats: a lane reads its P taps with 16-byte loads.  Two routes:
//   staged   a workgroup makes `tile` consecutive outputs; the inputs they need are ONE contiguous span
//            s[a0 - (P - 1) .. a_last], loaded coalesced into LDS once (history / zeros resolved there); lanes take
//            consecutive k, every re-read of an input (about P U / Q per input) is an LDS read.
//            A lane issues all its span loads before the first LDS write and sums kOuts outputs side by side:
//            one load or one LDS read in flight per lane ran 1.7 .. 2.9 x slower.
//   direct   the staged tile would fall below one output per lane (Q / U above about 16): a lane reads its own P
//            samples from memory; a workgroup makes kBlock outputs.
// U == 1: the one tap row is the same for every lane (template flag: scalar loads).
// What this file shares with aeth_arb.hip is in aeth_polyphase.h: the shape constants, the span load, the direct route's
// sample fetch, the tile rule and the host side of create, destroy and a launch.  Here: the kernels, the tap sum, the lengths.
#include "aeth_polyphase.h"

#include <cmath>

namespace {

using namespace aeth::poly;

constexpr unsigned kMaxRatio = 4096;

struct ResampCall {
    const float2 *in, *hist;   // hist: P - 1 samples in front of in[0], or null (zeros)
    float2 *out;
    const float *g;            // U rows of Pp taps
    size_t n_out;
    unsigned U, Q, P, Pp;
    unsigned tile;             // outputs per workgroup
    aeth::FastDiv fd_U;
};

// N outputs at once: acc[j] = sum over p ascending of row[j][p] * s(j, p).  The N sums are independent, so N LDS (or
// memory) reads are in flight where one output alone would wait for each of its own.
template <int N, class S> __device__ __forceinline__ void dot_taps(const float *const (&row)[N], unsigned P, S s, float2 (&acc)[N])
{
    unsigned p;
    if (P >= 4) {
#pragma unroll
        for (int j = 0; j < N; j++) {
            const float4 t = *reinterpret_cast<const float4 *>(row[j]);
            acc[j] = mulr(t.x, s(j, 0u));
            acc[j] = add2(acc[j], mulr(t.y, s(j, 1u)));
            acc[j] = add2(acc[j], mulr(t.z, s(j, 2u)));
            acc[j] = add2(acc[j], mulr(t.w, s(j, 3u)));
        }
        for (p = 4; p + 4 <= P; p += 4) {
#pragma unroll
            for (int j = 0; j < N; j++) {
                const float4 u = *reinterpret_cast<const float4 *>(row[j] + p);
                acc[j] = add2(acc[j], mulr(u.x, s(j, p)));
                acc[j] = add2(acc[j], mulr(u.y, s(j, p + 1)));
                acc[j] = add2(acc[j], mulr(u.z, s(j, p + 2)));
                acc[j] = add2(acc[j], mulr(u.w, s(j, p + 3)));
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < N; j++) acc[j] = mulr(row[j][0], s(j, 0u));
        p = 1;
    }
    for (; p < P; p++) {                                      // at most three: the padding is never multiplied
#pragma unroll
        for (int j = 0; j < N; j++) acc[j] = add2(acc[j], mulr(row[j][p], s(j, p)));
    }
}

// where the workgroup's first output k0 stands in the input: a0 = floor(k0 Q / U), r0 = (k0 Q) mod U.  64-bit, once.
__device__ __forceinline__ void tile_origin(const ResampCall &a, size_t k0, size_t *a0, unsigned *r0)
{
    const uint64_t t0 = (uint64_t)k0 * a.Q;
    const uint64_t q = t0 / a.U;
    *a0 = (size_t)q;
    *r0 = (unsigned)(t0 - q * a.U);
}

// ---- staged: the tile's input span in LDS ---------------------------------------------------------------------------
// lds[i] = s[a0 - (P - 1) + i], i = 0 .. a_last - a0 + P - 1 < kSpan (tile_of).  Output k0 + e stands at
// t = r0 + e Q < 2^12 + 2^12 * 2^12 < 2^25: da = t / U by FastDiv, its newest sample is lds[da + P - 1].
template <bool U1, bool NT> __global__ __launch_bounds__(kBlock, 4) void resamp_staged_kernel(ResampCall a)
{
    __shared__ float2 lds[kSpan];
    const size_t k0 = (size_t)blockIdx.x * a.tile;
    const unsigned nk = a.n_out - k0 < a.tile ? (unsigned)(a.n_out - k0) : a.tile;
    const unsigned P = a.P, U = a.U, Q = a.Q;
    size_t a0;
    unsigned r0;
    tile_origin(a, k0, &a0, &r0);
    const unsigned t_last = r0 + (nk - 1) * Q;
    const unsigned span = (U1 ? t_last : aeth::fdiv(t_last, a.fd_U)) + P;
    const ptrdiff_t first = (ptrdiff_t)a0 - (ptrdiff_t)(P - 1);
    load_span<NT>(lds, a.in, a.hist, first, span, P);
    __syncthreads();
    for (unsigned e = threadIdx.x; e < nk; e += kOuts * kBlock) {
        const float *row[kOuts];
        const float2 *top[kOuts];
#pragma unroll
        for (int j = 0; j < kOuts; j++) {
            const unsigned t = r0 + out_of(e, j, nk) * Q;
            const unsigned da = U1 ? t : aeth::fdiv(t, a.fd_U);
            row[j] = a.g + (size_t)(U1 ? 0u : t - da * U) * a.Pp;
            top[j] = lds + da + (P - 1);
        }
        float2 acc[kOuts];
        dot_taps<kOuts>(row, P, SpanTaps{top}, acc);
#pragma unroll
        for (int j = 0; j < kOuts; j++)
            if (e + j * kBlock < nk) aeth::nt_store<NT>(a.out + k0 + e + j * kBlock, acc[j]);
    }
}

// ---- direct: strong decimation, a lane gathers its own samples ---------------------------------------------------------
template <bool U1, bool NT> __global__ __launch_bounds__(kBlock, 4) void resamp_direct_kernel(ResampCall a)
{
    const size_t k0 = (size_t)blockIdx.x * kBlock;
    if (k0 + threadIdx.x >= a.n_out) return;
    const unsigned P = a.P, U = a.U;
    size_t a0;
    unsigned r0;
    tile_origin(a, k0, &a0, &r0);
    const unsigned t = r0 + threadIdx.x * a.Q;               // < 2^12 + 2^8 * 2^12
    const unsigned da = U1 ? t : aeth::fdiv(t, a.fd_U);
    const unsigned r = U1 ? 0u : t - da * U;
    const ptrdiff_t top = (ptrdiff_t)(a0 + da);              // <= n - 1
    const float *row[1] = {a.g + (size_t)r * a.Pp};
    float2 acc[1];
    dot_taps<1>(row, P, Fetch<NT>{a.in, a.hist, top, P}, acc);
    aeth::nt_store<NT>(a.out + k0 + threadIdx.x, acc[0]);
}

// tile_for: the span fits kSpan whatever r0 is, floor((U - 1 + (tile - 1) Q) / U) + P <= kSpan, when
// U - 1 + (tile - 1) Q < (kSpan - P + 1) U
size_t tile_of(size_t U, size_t Q, size_t P) { return tile_for((kSpan - P) * U, Q); }

enum { ROUTE_STAGED = 0, ROUTE_DIRECT = 1 };

}  // namespace

struct aeth_resamp : aeth::poly::Resampler {     // taps: U rows of Pp floats
    size_t U = 0, Q = 0;
    size_t tile = 0;
    int kind = ROUTE_STAGED;
    char route[32] = {0};
};

namespace {

typedef void (*ResampKernel)(ResampCall);

ResampKernel kernel_of(int kind, bool u1, bool nt)
{
    if (kind == ROUTE_STAGED)
        return u1 ? (nt ? resamp_staged_kernel<true, true> : resamp_staged_kernel<true, false>)
                  : (nt ? resamp_staged_kernel<false, true> : resamp_staged_kernel<false, false>);
    return u1 ? (nt ? resamp_direct_kernel<true, true> : resamp_direct_kernel<true, false>)
              : (nt ? resamp_direct_kernel<false, true> : resamp_direct_kernel<false, false>);
}

// does a call over n input samples keep every element count and k Q clear of overflow?
bool samples_fit(const aeth_resamp &r, size_t n) { return n <= SIZE_MAX / 16 / r.U; }

}  // namespace

extern "C" {

int aeth_resamp_create(aeth_ctx *ctx, const float *taps_host, size_t ntaps, size_t up, size_t down, aeth_resamp **out)
{
    AETH_REQUIRE(out, AETH_E_ARG, "out is null");
    *out = nullptr;
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    AETH_REQUIRE(taps_host, AETH_E_ARG, "taps are null");
    AETH_REQUIRE(up >= 1 && down >= 1, AETH_E_ARG, "up %zu, down %zu: both at least 1", up, down);
    AETH_REQUIRE(up <= kMaxRatio, AETH_E_UNSUPPORTED, "up %zu: at most %u", up, kMaxRatio);
    AETH_REQUIRE(down <= kMaxRatio, AETH_E_UNSUPPORTED, "down %zu: at most %u", down, kMaxRatio);
    AETH_REQUIRE(ntaps >= 1 && ntaps % up == 0, AETH_E_ARG, "%zu taps are not a multiple (at least one) of up %zu", ntaps, up);
    AETH_REQUIRE(ntaps / up <= kMaxP, AETH_E_UNSUPPORTED, "%zu taps per phase: at most %u", ntaps / up, kMaxP);
    aeth_resamp *r = new (std::nothrow) aeth_resamp();
    AETH_REQUIRE(r, AETH_E_NOMEM, "out of host memory");
    r->ctx = ctx;
    r->U = up; r->Q = down; r->T = ntaps; r->P = ntaps / up; r->Pp = (r->P + 3) / 4 * 4;
    r->tile = tile_of(up, down, r->P);
    r->kind = r->tile ? ROUTE_STAGED : ROUTE_DIRECT;
    if (!r->tile) r->tile = kBlock;
    snprintf(r->route, sizeof r->route, "%s%s", r->kind == ROUTE_STAGED ? "staged" : "direct", up == 1 ? " u1" : "");
    const size_t nt = r->U * r->Pp;
    float *g = new (std::nothrow) float[nt]();
    if (!g) { delete r; return aeth::set_error(AETH_E_NOMEM, "out of host memory"); }
    for (size_t p = 0; p < r->P; p++)
        for (size_t q = 0; q < up; q++) g[q * r->Pp + p] = taps_host[p * up + q];
    return create_finish(r, g, nt, "aeth_resamp_create: tap upload", out);
}

int aeth_resamp_destroy(aeth_resamp *r) { return destroy(r); }

size_t aeth_resamp_up(const aeth_resamp *r) { return r ? r->U : 0; }
size_t aeth_resamp_down(const aeth_resamp *r) { return r ? r->Q : 0; }
size_t aeth_resamp_ntaps(const aeth_resamp *r) { return r ? r->T : 0; }
size_t aeth_resamp_history(const aeth_resamp *r) { return r ? r->P - 1 : 0; }
size_t aeth_resamp_tile(const aeth_resamp *r) { return r ? r->tile : 0; }
const char *aeth_resamp_route(const aeth_resamp *r) { return r ? r->route : ""; }
size_t aeth_resamp_out_count(const aeth_resamp *r, size_t n_in)
{
    return r && n_in % r->Q == 0 && samples_fit(*r, n_in) ? n_in / r->Q * r->U : 0;
}

int aeth_resamp_exec(aeth_resamp *r, const aeth_cf32 *hist, const aeth_cf32 *in, size_t n, aeth_cf32 *out, size_t n_out)
{
    AETH_REQUIRE(r, AETH_E_ARG, "resamp is null");
    AETH_REQUIRE(in && out, AETH_E_ARG, "null pointer");
    AETH_REQUIRE(n > 0, AETH_E_LEN, "0 input samples: a call takes at least one period of %zu", r->Q);
    AETH_REQUIRE(n % r->Q == 0, AETH_E_LEN, "%zu input samples are not a multiple of down %zu", n, r->Q);
    AETH_REQUIRE(samples_fit(*r, n), AETH_E_UNSUPPORTED, "%zu input samples at up %zu: the element counts overflow", n, r->U);
    const size_t B = n / r->Q, want = B * r->U;
    AETH_REQUIRE(n_out == want, AETH_E_LEN, "output holds %zu elements, %zu periods x up %zu give %zu", n_out, B, r->U, want);

    ResampCall a{};
    a.g = (const float *)r->taps;
    a.U = (unsigned)r->U; a.Q = (unsigned)r->Q;
    a.fd_U = aeth::make_fastdiv(a.U);
    return launch(*r, hist, in, n, out, n_out, r->tile, a, [r](bool nt) { return kernel_of(r->kind, r->U == 1, nt); });
}

int aeth_resamp_prototype(size_t up, size_t down, size_t taps_per_phase, float *out_host)
{
    AETH_REQUIRE(up >= 1 && down >= 1 && taps_per_phase >= 1, AETH_E_ARG,
                 "prototype of up %zu, down %zu, %zu taps per phase: all at least 1", up, down, taps_per_phase);
    AETH_REQUIRE(up <= (SIZE_MAX / sizeof(double)) / taps_per_phase, AETH_E_ARG, "up %zu x %zu taps per phase overflow", up, taps_per_phase);
    AETH_REQUIRE(out_host, AETH_E_ARG, "out is null");
    const size_t L = up * taps_per_phase;
    if (L == 1) { out_host[0] = 1.0f; return AETH_OK; }
    const double pi = 3.14159265358979323846, dL = (double)L, c = (double)(up > down ? up : down);
    double *h = new (std::nothrow) double[L];
    AETH_REQUIRE(h, AETH_E_NOMEM, "out of host memory");
    double sum = 0.0;
    for (size_t n = 0; n < (L + 1) / 2; n++) {               // the first half; the second is its mirror, bit for bit
        const double t = ((double)n - (dL - 1.0) / 2.0) / c, x = pi * t;
        const double sinc = t == 0.0 ? 1.0 : std::sin(x) / x;
        h[n] = h[L - 1 - n] = sinc * (0.54 - 0.46 * std::cos(2.0 * pi * (double)n / (dL - 1.0)));
    }
    for (size_t n = 0; n < L; n++) sum += h[n];
    for (size_t n = 0; n < L; n++) out_host[n] = (float)(h[n] * (double)up / sum);
    delete[] h;
    return AETH_OK;
}

}  // extern "C"
