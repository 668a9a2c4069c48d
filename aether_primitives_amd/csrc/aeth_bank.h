// aeth_bank.h -- the host core of the two filter banks (aeth_chan.hip: analysis, aeth_synth.hip: synthesis, its
// transpose): what both keep, how both are created and destroyed, what both check before a call, the launch geometry
// (the same in both with M and D swapped) and the device helpers of their ring kernels.  The kernels, their argument
// structs and the choice of a route stay with each bank.
#pragma once
#include "aeth_internal.h"

#include <new>

namespace aeth {
namespace bank {

constexpr int kBlock = 256;
constexpr unsigned kMaxP = 64;
constexpr unsigned kGenElems = 4096;         // outputs one workgroup of a general kernel makes: 16 per lane

// what both banks keep; aeth_chan and aeth_synth derive from it
struct Bank {
    aeth_ctx *ctx = nullptr;
    size_t M = 0, L = 0, P = 0, D = 0;
    int phase = 0;
    size_t tile = 0;
    float *taps = nullptr;       // the prototype on the device (the synthesis bank's fold route: its rows reversed)
    aeth_fft *fft = nullptr;
    DevScratch scratch;          // the frames between the fold / unfold and the plan, grown on demand to the exact size;
                                 // not one of ctx_scratch: aeth_ctx_trim leaves it alone
};

// ---- device helpers of the ring kernels: a lane owns one column (8-byte accesses) or two (16-byte accesses) -----------
template <int CW> struct Row;
template <> struct Row<1> { typedef float2 T; };
template <> struct Row<2> { typedef float4 T; };

__device__ __forceinline__ float2 mulw(float2 x, const float *w) { return make_float2(w[0] * x.x, w[0] * x.y); }
__device__ __forceinline__ float4 mulw(float4 x, const float *w) { return make_float4(w[0] * x.x, w[0] * x.y, w[1] * x.z, w[1] * x.w); }
__device__ __forceinline__ float2 addv(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float4 addv(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// ---- geometry: `width` is what the lanes run along (analysis: the M columns, synthesis: the D offsets of a hop), a tile
// is what a lane (ring) or a workgroup (general) walks along the frames ---------------------------------------------------
// ring: depth - 1 halo rows per tile, a sixteenth of the tile at most (depth 2: 1 of 16, depth 8: 7 of 128)
inline size_t ring_tile(size_t depth)
{
    size_t tile = 16;
    while (tile < 16 * (depth - 1)) tile *= 2;
    return tile;
}
// general: a workgroup makes `tile` whole rows (width <= 2048: tile * width <= kGenElems) or kGenElems elements of one
inline size_t gen_tile(size_t width) { return width <= kGenElems / 2 ? kGenElems / width : 1; }
inline size_t gen_ncb(size_t width) { return (width + kGenElems - 1) / kGenElems; }

// ring: 1 << lx_log2 lanes of a workgroup along the width, the rest along the tiles; ncb blocks cover the width
struct RingShape {
    unsigned lx_log2 = 0, ncb = 0;
    size_t grid = 0;
};
inline RingShape ring_shape(size_t lanes, size_t ntiles)
{
    RingShape r;
    while ((1u << r.lx_log2) < kBlock && ((size_t)1 << r.lx_log2) < lanes) r.lx_log2++;
    r.ncb = (unsigned)((lanes + (1u << r.lx_log2) - 1) >> r.lx_log2);
    const size_t ly = kBlock >> r.lx_log2;
    r.grid = ((ntiles + ly - 1) / ly) * r.ncb;
    return r;
}
inline size_t ntiles_of(const Bank &b, size_t F) { return (F + b.tile - 1) / b.tile; }
// workgroups of a launch over F frames, at most (the ring kernel with one element per lane)
inline size_t grid_bound(bool ring, size_t width, size_t ntiles) { return ring ? ring_shape(width, ntiles).grid : ntiles * gen_ncb(width); }

// does a call over F frames (+ K in front of them) keep every element count clear of overflow?
inline bool frames_fit(const Bank &b, size_t F, size_t K = 0) { return F <= SIZE_MAX / 16 / b.M - K; }

inline int ensure_elems(Bank &b, size_t elems) { return scratch_ensure(b.ctx, b.scratch, elems * sizeof(float2), false); }

// the launch of either bank's kernel on the context's stream
template <class Call> int launch(const Bank &b, void (*k)(Call), size_t grid, Call &a)
{
    a.fd_ncb = make_fastdiv(a.ncb);
    DeviceGuard dg(b.ctx->device);
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(kBlock), 0, ctx_stream(b.ctx), a);
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

// ---- create and destroy -------------------------------------------------------------------------------------------------
// what both create calls refuse, in this order
template <class T> int create_checks(T **out, const aeth_ctx *ctx, const float *proto_host, size_t ntaps, size_t channels, size_t hop, int phase)
{
    AETH_REQUIRE(out, AETH_E_ARG, "out is null");
    *out = nullptr;
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    AETH_REQUIRE(proto_host, AETH_E_ARG, "prototype is null");
    AETH_REQUIRE(channels >= 1, AETH_E_ARG, "0 channels");
    AETH_REQUIRE(ntaps >= 1 && ntaps % channels == 0, AETH_E_ARG, "%zu taps are not a multiple (at least one) of %zu channels", ntaps, channels);
    AETH_REQUIRE(ntaps / channels <= kMaxP, AETH_E_UNSUPPORTED, "%zu taps per channel: at most %u", ntaps / channels, kMaxP);
    AETH_REQUIRE(hop >= 1 && hop <= channels, AETH_E_ARG, "hop %zu outside 1 .. %zu channels", hop, channels);
    AETH_REQUIRE(phase == AETH_CHAN_PHASE_FRAME || phase == AETH_CHAN_PHASE_STREAM, AETH_E_ARG, "bad phase mode %d", phase);
    return AETH_OK;
}

template <class T> int destroy(T *b)
{
    if (!b) return AETH_OK;
    (void)aeth_fft_destroy(b->fft);          // waits for the context's stream
    DeviceGuard dg(b->ctx->device);
    if (b->taps) (void)hipFree(b->taps);
    (void)scratch_release(b->scratch);
    delete b;
    return AETH_OK;
}

// the plan first (a refused transform length leaves nothing allocated), then the object with its sizes
template <class T> int create_planned(aeth_ctx *ctx, size_t ntaps, size_t channels, size_t hop, int phase, size_t max_frames, T **obj)
{
    aeth_fft *fft = nullptr;
    int rc = aeth_fft_create(ctx, channels, max_frames, &fft); if (rc) return rc;      // names the refused length
    T *b = new (std::nothrow) T();
    if (!b) { (void)aeth_fft_destroy(fft); return set_error(AETH_E_NOMEM, "out of host memory"); }
    b->ctx = ctx; b->fft = fft;
    b->M = channels; b->L = ntaps; b->P = ntaps / channels; b->D = hop; b->phase = phase;
    *obj = b;
    return AETH_OK;
}

// the taps go up, the scratch is sized for `scratch_elems` (0: on the first call), *out takes the object; on a failure
// the object is destroyed.  `what` names the upload in a HIP error's text.
template <class T> int create_finish(T *b, const float *taps_host, size_t scratch_elems, const char *what, T **out)
{
    int rc = upload_table(b->ctx, taps_host, b->L * sizeof(float), &b->taps, what);
    if (!rc && scratch_elems) rc = ensure_elems(*b, scratch_elems);
    if (rc) { (void)destroy(b); return rc; }
    *out = b;
    return AETH_OK;
}

// ---- the analysis bank's fold, which is also the synthesis bank's route for hop == M (aeth_chan.hip) ---------------------
// They read M, L, P, D, tile, taps and ctx of `b`, whichever bank it belongs to.
bool chan_ring(const Bank &b);               // hop == M and P <= 8: the ring kernel
size_t chan_tile(const Bank &b);
// the fold of F frames into out on the context's stream; `stream`: the phase refers to the first sample ever fed; every
// argument has been checked
int chan_launch_fold(const Bank &b, bool stream, const aeth_cf32 *hist, const aeth_cf32 *in, size_t F, uint64_t first_frame, float2 *out);

}  // namespace bank
}  // namespace aeth

// the analysis bank's object: its calls are in aeth_chan.hip, its averaged spectra in aeth_spec.hip
struct aeth_chan : aeth::bank::Bank {};
