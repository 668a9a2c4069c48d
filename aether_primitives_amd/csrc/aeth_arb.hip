// aeth_arb.hip -- arbitrary-ratio resampler: a polyphase bank of L = 2^b phases whose taps are linearly interpolated
// between neighbouring phases, addressed by an unsigned Q32.32 time word (the reference's rate changes are linear
// interpolation and sample picking: src/sampling.rs:7-62).
// Output m of a call stands at t = phase + m step (input samples, 32 fraction bits).  a = t >> 32, f = (uint32)t,
// r = f >> (32 - b), mu = the next 24 bits of f, scaled by 2^-24 (exact in f32):
//     out[m] = sum over p = 0 .. P - 1 ascending of (h[p L + r] + mu d[p L + r]) * s[a - p],     d[j] = h[j + 1] - h[j]
// every product and every sum rounded (EXACT flags), the sum started from the p = 0 product.  The taps lie phase-major
// on the device as (h, d) pairs, g[r][p] = (h[p L + r], d[p L + r]), rows padded to an even number of pairs: a lane
// reads two taps with one 16-byte load.  The routes are those of aeth_resamp.hip, and what the two files share (shape
// constants, span load, direct fetch, tile rule, the host side of create, destroy and a launch) is in aeth_polyphase.h:
//   staged   a workgroup makes `tile` consecutive outputs; their inputs are ONE contiguous span s[a0 - (P - 1) .. a_last],
//            loaded coalesced into LDS once (history / zeros resolved there).  A lane issues all its span loads before
//            the first LDS write and sums kOuts outputs side by side.  A table of at most kTabSlots 16-byte slots is
//            copied into LDS as well ("staged tab"): consecutive lanes hit unrelated rows, and from memory that gather ran
//            the small-table cases 1.3 .. 1.8 x slower.
//   direct   not even 256 outputs fit the span (step above about (4096 - P) / 255, which includes every step that skips
//            inputs): a lane reads its own P samples from memory; a workgroup makes kBlock outputs.
// The word of a workgroup's first output is one 64-bit multiply of uniform values; a lane adds e * step.  Wrap-around
// arithmetic is exact, because the true value stays below n * 2^32 <= 2^63.
#include "aeth_polyphase.h"

namespace {

using namespace aeth::poly;

constexpr unsigned kMaxLog2 = 12;
constexpr unsigned kTabSlots = 512;          // 16-byte slots of tap table a staged workgroup keeps in LDS: 8 KiB, 40 KiB with the span
constexpr uint64_t kMinStep = (uint64_t)1 << 20, kMaxStep = (uint64_t)1 << 44;

struct ArbCall {
    const float2 *in, *hist;   // hist: P - 1 samples in front of in[0], or null (zeros)
    float2 *out;
    const float2 *g;           // L rows of Pp (h, d) pairs
    size_t n_out;
    uint64_t step, phase;
    unsigned P, Pp, b;
    unsigned tile;             // outputs per workgroup
};

// the interpolated tap: the product rounded, then the sum rounded
__device__ __forceinline__ float tap(float h, float d, float mu) { const float md = mu * d; return h + md; }

// the table row and the interpolation weight of a fraction f
__device__ __forceinline__ void row_of(const ArbCall &a, unsigned f, unsigned *r, float *mu)
{
    *r = a.b ? f >> (32 - a.b) : 0u;
    const unsigned mu24 = (f << a.b) >> 8;
    *mu = (float)mu24 * 0x1p-24f;                            // 24 bits: the conversion and the product are exact
}

// N outputs at once: acc[j] = sum over p ascending of tap(h, d, mu[j]) * s(j, p), the pairs (h, d) of taps 2 q and 2 q + 1
// coming as one 16-byte slot g(j, q).  The N sums are independent, so N LDS (or memory) reads are in flight where one
// output alone would wait for each of its own.  Of the last slot of an odd P only the first pair is used: the padding is
// never multiplied.
template <int N, class G, class S>
__device__ __forceinline__ void dot_taps(unsigned P, const float (&mu)[N], G g, S s, float2 (&acc)[N])
{
#pragma unroll
    for (int j = 0; j < N; j++) {
        const float4 t = g(j, 0u);
        acc[j] = mulr(tap(t.x, t.y, mu[j]), s(j, 0u));
        if (P >= 2) acc[j] = add2(acc[j], mulr(tap(t.z, t.w, mu[j]), s(j, 1u)));
    }
    unsigned p;
    for (p = 2; p + 2 <= P; p += 2) {
#pragma unroll
        for (int j = 0; j < N; j++) {
            const float4 u = g(j, p >> 1);
            acc[j] = add2(acc[j], mulr(tap(u.x, u.y, mu[j]), s(j, p)));
            acc[j] = add2(acc[j], mulr(tap(u.z, u.w, mu[j]), s(j, p + 1)));
        }
    }
    if (p < P) {                                             // P odd and above 1: the last pair alone
#pragma unroll
        for (int j = 0; j < N; j++) {
            const float4 u = g(j, p >> 1);
            acc[j] = add2(acc[j], mulr(tap(u.x, u.y, mu[j]), s(j, p)));
        }
    }
}

// ---- staged: the tile's input span in LDS ---------------------------------------------------------------------------
// lds[i] = s[a0 - (P - 1) + i], i = 0 .. a_last - a0 + P - 1 < kSpan (tile_of).  Output k0 + e stands at
// f0 + e step < 2^32 + 2^12 * 2^44 relative to a0: its newest sample is lds[(that >> 32) + P - 1].
// TAB: the table is at most kTabSlots slots and lies in LDS as well, slot q of row r at place (q + r) mod slots of its
// row: lanes of a wave read unrelated rows at the same q, and unrotated those all fall on the banks of slot q.
template <bool NT, bool TAB> __global__ __launch_bounds__(kBlock, 4) void arb_staged_kernel(ArbCall a)
{
    __shared__ float2 lds[kSpan];
    const unsigned slots = a.Pp >> 1;
    const float4 *tab = nullptr;
    if constexpr (TAB) {
        __shared__ float4 tab_s[kTabSlots];
        const unsigned total = slots << a.b;
        for (unsigned i = threadIdx.x; i < total; i += kBlock) {
            const unsigned row = i / slots, q = i - row * slots;
            unsigned at = q + row % slots;
            if (at >= slots) at -= slots;
            tab_s[row * slots + at] = reinterpret_cast<const float4 *>(a.g)[i];
        }
        tab = tab_s;
    }
    const size_t k0 = (size_t)blockIdx.x * a.tile;
    const unsigned nk = a.n_out - k0 < a.tile ? (unsigned)(a.n_out - k0) : a.tile;
    const unsigned P = a.P;
    const uint64_t step = a.step;
    const uint64_t t0 = a.phase + (uint64_t)k0 * step;       // uniform: one 64-bit multiply per workgroup
    const size_t a0 = (size_t)(t0 >> 32);
    const uint64_t f0 = t0 & 0xffffffffu;
    const unsigned span = (unsigned)((f0 + (uint64_t)(nk - 1) * step) >> 32) + P;
    const ptrdiff_t first = (ptrdiff_t)a0 - (ptrdiff_t)(P - 1);
    load_span<NT>(lds, a.in, a.hist, first, span, P);
    __syncthreads();
    for (unsigned e = threadIdx.x; e < nk; e += kOuts * kBlock) {
        const float4 *row[kOuts];                            // the row's first slot, in memory or in LDS
        unsigned rot[kOuts];                                 // TAB: where the row's slot 0 lies
        const float2 *top[kOuts];
        float mu[kOuts];
#pragma unroll
        for (int j = 0; j < kOuts; j++) {
            const uint64_t t = f0 + (uint64_t)out_of(e, j, nk) * step;
            unsigned r;
            row_of(a, (unsigned)t, &r, &mu[j]);
            row[j] = (TAB ? tab : reinterpret_cast<const float4 *>(a.g)) + (size_t)r * slots;
            rot[j] = TAB ? r % slots : 0u;
            top[j] = lds + (unsigned)(t >> 32) + (P - 1);
        }
        float2 acc[kOuts];
        dot_taps<kOuts>(P, mu, [&](int j, unsigned q) {
            if constexpr (TAB) {
                unsigned at = q + rot[j];
                if (at >= slots) at -= slots;
                return row[j][at];
            } else return row[j][q];
        }, SpanTaps{top}, acc);
#pragma unroll
        for (int j = 0; j < kOuts; j++)
            if (e + j * kBlock < nk) aeth::nt_store<NT>(a.out + k0 + e + j * kBlock, acc[j]);
    }
}

// ---- direct: a lane gathers its own samples --------------------------------------------------------------------------
template <bool NT> __global__ __launch_bounds__(kBlock, 4) void arb_direct_kernel(ArbCall a)
{
    const size_t k0 = (size_t)blockIdx.x * kBlock;
    if (k0 + threadIdx.x >= a.n_out) return;
    const unsigned P = a.P;
    const uint64_t t0 = a.phase + (uint64_t)k0 * a.step;     // uniform
    const uint64_t t = t0 + (uint64_t)threadIdx.x * a.step;
    const ptrdiff_t top = (ptrdiff_t)(t >> 32);              // <= n - 1
    unsigned r;
    float mu[1];
    row_of(a, (unsigned)t, &r, &mu[0]);
    const float4 *row = reinterpret_cast<const float4 *>(a.g) + (size_t)r * (a.Pp >> 1);
    float2 acc[1];
    dot_taps<1>(P, mu, [=](int, unsigned q) { return row[q]; }, Fetch<NT>{a.in, a.hist, top, P}, acc);
    aeth::nt_store<NT>(a.out + k0 + threadIdx.x, acc[0]);
}

bool step_ok(uint64_t step) { return step >= kMinStep && step <= kMaxStep; }

// tile_for: the span fits kSpan whatever the fraction of t(k0) is, floor((2^32 - 1 + (tile - 1) step) / 2^32) + P <= kSpan,
// when (tile - 1) step <= (kSpan - P) 2^32
size_t tile_of(uint64_t step, size_t P) { return tile_for((uint64_t)(kSpan - P) << 32, step); }

}  // namespace

struct aeth_arb : aeth::poly::Resampler {        // taps: L rows of Pp (h, d) pairs
    size_t L = 0, b = 0;
};

namespace {

typedef void (*ArbKernel)(ArbCall);

// the staged route keeps the table in LDS when its 16-byte slots fit beside the span
bool table_fits_lds(const aeth_arb &r) { return r.L * (r.Pp / 2) <= kTabSlots; }

ArbKernel kernel_of(bool staged, bool tab, bool nt)
{
    if (staged && tab) return nt ? arb_staged_kernel<true, true> : arb_staged_kernel<false, true>;
    if (staged) return nt ? arb_staged_kernel<true, false> : arb_staged_kernel<false, false>;
    return nt ? arb_direct_kernel<true> : arb_direct_kernel<false>;
}

}  // namespace

extern "C" {

int aeth_arb_advance(uint64_t step, uint64_t phase, size_t n, size_t *count, uint64_t *next_phase)
{
    typedef unsigned __int128 u128;
    AETH_REQUIRE(count && next_phase, AETH_E_ARG, "count or next_phase is null");
    AETH_REQUIRE(step_ok(step), AETH_E_UNSUPPORTED, "step %llu: from 2^20 to 2^44 (1/4096 to 4096 input samples per output)",
                 (unsigned long long)step);
    AETH_REQUIRE(phase < ((uint64_t)1 << 63), AETH_E_UNSUPPORTED, "phase %llu: below 2^63", (unsigned long long)phase);
    AETH_REQUIRE((uint64_t)n <= ((uint64_t)1 << 31), AETH_E_UNSUPPORTED, "%zu input samples in one call: at most 2^31", n);
    const u128 end = (u128)n << 32, lim = (u128)1 << 64;
    u128 c = 0;
    if ((u128)phase < end) c = (end - phase + step - 1) / step;
    const u128 reach = (u128)phase + c * step;               // the next call's first output, in this call's time
    AETH_REQUIRE(c < lim && reach < lim, AETH_E_UNSUPPORTED, "step %llu, phase %llu, %zu input samples: a time word of 2^64 or more",
                 (unsigned long long)step, (unsigned long long)phase, n);
    *count = (size_t)c;
    *next_phase = (uint64_t)(reach - end);
    return AETH_OK;
}

int aeth_arb_create(aeth_ctx *ctx, const float *taps_host, size_t ntaps, size_t log2_phases, aeth_arb **out)
{
    AETH_REQUIRE(out, AETH_E_ARG, "out is null");
    *out = nullptr;
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    AETH_REQUIRE(taps_host, AETH_E_ARG, "taps are null");
    AETH_REQUIRE(log2_phases <= kMaxLog2, AETH_E_UNSUPPORTED, "log2_phases %zu: at most %u", log2_phases, kMaxLog2);
    const size_t L = (size_t)1 << log2_phases;
    AETH_REQUIRE(ntaps >= 1 && ntaps % L == 0, AETH_E_ARG, "%zu taps are not a multiple (at least one) of %zu phases", ntaps, L);
    AETH_REQUIRE(ntaps / L <= kMaxP, AETH_E_UNSUPPORTED, "%zu taps per phase: at most %u", ntaps / L, kMaxP);
    aeth_arb *r = new (std::nothrow) aeth_arb();
    AETH_REQUIRE(r, AETH_E_NOMEM, "out of host memory");
    r->ctx = ctx;
    r->L = L; r->b = log2_phases; r->T = ntaps; r->P = ntaps / L; r->Pp = (r->P + 1) / 2 * 2;
    const size_t nt = r->L * r->Pp;
    float2 *g = new (std::nothrow) float2[nt]();
    if (!g) { delete r; return aeth::set_error(AETH_E_NOMEM, "out of host memory"); }
    for (size_t p = 0; p < r->P; p++)
        for (size_t q = 0; q < L; q++) {
            const size_t j = p * L + q;
            const float h = taps_host[j], hn = j + 1 < ntaps ? taps_host[j + 1] : 0.0f;      // h[T] = +0.0
            const float d = hn - h;
            g[q * r->Pp + p] = make_float2(h, d);
        }
    return create_finish(r, g, nt, "aeth_arb_create: tap upload", out);
}

int aeth_arb_destroy(aeth_arb *r) { return destroy(r); }

size_t aeth_arb_phases(const aeth_arb *r) { return r ? r->L : 0; }
size_t aeth_arb_ntaps(const aeth_arb *r) { return r ? r->T : 0; }
size_t aeth_arb_history(const aeth_arb *r) { return r ? r->P - 1 : 0; }
size_t aeth_arb_tile(const aeth_arb *r, uint64_t step)
{
    if (!r || !step_ok(step)) return 0;
    const size_t tile = tile_of(step, r->P);
    return tile ? tile : (size_t)kBlock;
}
const char *aeth_arb_route(const aeth_arb *r, uint64_t step)
{
    if (!r || !step_ok(step)) return "";
    if (!tile_of(step, r->P)) return "direct";
    return table_fits_lds(*r) ? "staged tab" : "staged";
}

int aeth_arb_exec(aeth_arb *r, const aeth_cf32 *hist, const aeth_cf32 *in, size_t n, uint64_t step, uint64_t phase,
                  aeth_cf32 *out, size_t n_out)
{
    AETH_REQUIRE(r, AETH_E_ARG, "arb is null");
    AETH_REQUIRE(in && out, AETH_E_ARG, "null pointer");
    size_t want = 0;
    uint64_t next = 0;
    const int rc = aeth_arb_advance(step, phase, n, &want, &next);
    if (rc != AETH_OK) return rc;
    AETH_REQUIRE(n_out == want, AETH_E_LEN, "output holds %zu elements, %zu input samples at step %llu from phase %llu give %zu",
                 n_out, n, (unsigned long long)step, (unsigned long long)phase, want);
    size_t tile = tile_of(step, r->P);
    const bool staged = tile != 0;
    if (!staged) tile = kBlock;

    ArbCall a{};
    a.g = (const float2 *)r->taps;
    a.step = step; a.phase = phase;
    a.b = (unsigned)r->b;
    return launch(*r, hist, in, n, out, n_out, tile, a, [=](bool nt) { return kernel_of(staged, table_fits_lds(*r), nt); });
}

}  // extern "C"
