// aeth_polyphase.h -- what the two polyphase resamplers share (aeth_resamp.hip: rational, aeth_arb.hip: arbitrary ratio):
// the shape constants, the staged route's span load and the small parts of its output loop, the direct route's sample
// fetch, the tile rule, and on the host what both keep, how both finish a create, are destroyed and launch.  The kernels,
// their argument structs, the tap sums (dot_taps) and the length rules of a call stay with each resampler; so do the
// guarded stores of the staged loop (a shared helper cost the non-temporal builds registers).
#pragma once
#include "aeth_internal.h"

#include <new>

namespace aeth {
namespace poly {

constexpr int kBlock = 256;
constexpr unsigned kMaxP = 64;
constexpr unsigned kSpan = 4096;             // samples of LDS per workgroup: 32 KiB, four workgroups in a CU's 160 KiB
constexpr unsigned kMaxTile = 4096;          // outputs per workgroup: 16 per lane
constexpr int kOuts = 4;                     // outputs a lane of the staged route sums side by side

__device__ __forceinline__ float2 mulr(float w, float2 x) { return make_float2(w * x.x, w * x.y); }
__device__ __forceinline__ float2 add2(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }

// ---- staged: lds[i] = s[first + i], i < span <= kSpan, s the input with its history (P - 1 samples, null: zeros) in
// front.  The caller puts the barrier behind it.
template <bool NT>
__device__ __forceinline__ void load_span(float2 *lds, const float2 *in, const float2 *hist, ptrdiff_t first, unsigned span, unsigned P)
{
    if (first >= 0) {
        // the whole span lies in the input: all of a lane's loads (kSpan / kBlock at most) are issued before the first is used
        const float2 *src = in + first;
        float2 v[kSpan / kBlock];
#pragma unroll
        for (unsigned j = 0; j < kSpan / kBlock; j++) {
            const unsigned i = threadIdx.x + j * kBlock;
            if (i < span) v[j] = nt_load<NT>(src + i);
        }
#pragma unroll
        for (unsigned j = 0; j < kSpan / kBlock; j++) {
            const unsigned i = threadIdx.x + j * kBlock;
            if (i < span) lds[i] = v[j];
        }
    } else {
        // the stream's first tiles: the span reaches into the history
        for (unsigned i = threadIdx.x; i < span; i += kBlock) {
            const ptrdiff_t idx = first + (ptrdiff_t)i;
            float2 v = make_float2(0.f, 0.f);                // a history of zeros is multiplied like any other sample
            if (idx >= 0) v = nt_load<NT>(in + idx);
            else if (hist) v = hist[idx + (ptrdiff_t)(P - 1)];
            lds[i] = v;
        }
    }
}

// the j-th of the kOuts outputs a lane makes from e on; past the tile: an output that exists, never stored
__device__ __forceinline__ unsigned out_of(unsigned e, int j, unsigned nk) { return e + j * kBlock < nk ? e + j * kBlock : nk - 1; }

// sample p behind top[j], the newest sample of the lane's output j, in LDS
struct SpanTaps {
    const float2 *const (&top)[kOuts];
    __device__ __forceinline__ float2 operator()(int j, unsigned p) const { return top[j][-(int)p]; }
};

// ---- direct: sample p behind in[top], from the input, the history (P - 1 samples) or zeros
template <bool NT> struct Fetch {
    const float2 *in, *hist;
    ptrdiff_t top;
    unsigned P;
    __device__ __forceinline__ float2 operator()(int, unsigned p) const
    {
        const ptrdiff_t idx = top - (ptrdiff_t)p;
        if (idx >= 0) return nt_load<NT>(in + idx);
        return hist ? hist[idx + (ptrdiff_t)(P - 1)] : make_float2(0.f, 0.f);
    }
};

// The largest tile (a multiple of kBlock, at most kMaxTile) whose span fits kSpan wherever its first output stands between
// two inputs: num / den is how many steps from one output to the next advance by at most kSpan - P inputs, and a tile has
// one output more than steps.  0: not even kBlock outputs fit, the direct route.
inline size_t tile_for(uint64_t num, uint64_t den)
{
    uint64_t tile = num / den + 1;
    if (tile > kMaxTile) tile = kMaxTile;
    return (size_t)(tile / kBlock * kBlock);
}

// ---- host: what both resamplers keep; aeth_resamp and aeth_arb derive from it -----------------------------------------
struct Resampler {
    aeth_ctx *ctx = nullptr;
    size_t T = 0, P = 0, Pp = 0;
    void *taps = nullptr;        // phase-major on the device, rows of Pp
};

// the phase-major table g (count elements from new[]) goes up and is deleted, *out takes the object; on a failure the
// object is deleted.  `what` names the upload in a HIP error's text.
template <class R, class E> int create_finish(R *r, E *g, size_t count, const char *what, R **out)
{
    const int rc = upload_table(r->ctx, g, count * sizeof(E), &r->taps, what);
    delete[] g;
    if (rc) { delete r; return rc; }
    *out = r;
    return AETH_OK;
}

template <class R> int destroy(R *r)
{
    if (!r) return AETH_OK;
    DeviceGuard dg(r->ctx->device);
    (void)hipStreamSynchronize(ctx_stream(r->ctx));
    if (r->taps) (void)hipFree(r->taps);
    delete r;
    return AETH_OK;
}

// What both exec calls do behind their length checks: the refusals that are left, then n_out outputs in tiles of `tile`
// by the kernel kernel_of(nt).  in, hist, out, n_out, P, Pp and tile of `a` are filled here.
template <class Call, class Pick>
int launch(const Resampler &r, const aeth_cf32 *hist, const aeth_cf32 *in, size_t n, aeth_cf32 *out, size_t n_out, size_t tile, Call &a, Pick kernel_of)
{
    if (r.P == 1) hist = nullptr;
    const size_t grid = (n_out + tile - 1) / tile;
    const int rc = check_buffers(hist, r.P - 1, in, n, out, n_out, sizeof(aeth_cf32), grid, n_out, "outputs"); if (rc) return rc;
    if (!n_out) return AETH_OK;                              // a short chunk under strong decimation makes nothing
    a.in = (const float2 *)in;
    a.hist = (const float2 *)hist;
    a.out = (float2 *)out;
    a.n_out = n_out;
    a.P = (unsigned)r.P; a.Pp = (unsigned)r.Pp;
    a.tile = (unsigned)tile;
    const bool nt = streams_past_cache((n + n_out) * sizeof(float2));
    DeviceGuard dg(r.ctx->device);
    hipLaunchKernelGGL(kernel_of(nt), dim3((unsigned)grid), dim3(kBlock), 0, ctx_stream(r.ctx), a);
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

}  // namespace poly
}  // namespace aeth
