// aeth_chan.hip -- polyphase analysis filter bank: windowed, overlapped frames in front of the batched FFT
// (the reference frames a stream with chunks_mut(fft_len), src/util/plot.rs:46-68: disjoint rectangular frames; it has
// no window, no overlap and no prototype filter).
// Frame m weights the L = P * M newest samples up to (m + 1) * D with the real prototype w, folds them modulo M
// (P products per output, summed in ascending p, every product and every sum rounded: EXACT flags) and hands the M
// folded points to the plan.  Two kernels:
//   ring     hop == M, P <= 8: the stream is rows of M; a lane owns one column (8-byte accesses) or two adjacent ones
//            (16-byte accesses), keeps the last P rows in registers and walks a tile of frames: one load and one store
//            per folded row, P - 1 halo rows per tile.
//   general  everything else: a lane owns output q of frame m and reads its P inputs at r = (q - rot) mod M; the
//            M / D-fold (and, for hop == M with P > 8, the P-fold) overlap is served by L2.
#include "aeth_internal.h"
#include "aeth_chan_fold.h"
#include "aeth_fft_plan.h"
#include "aeth_levels.h"

#include <cmath>
#include <new>

namespace {

constexpr int kBlock = 256;
constexpr unsigned kMaxP = 64;
constexpr unsigned kRingMaxP = 8;            // the register ring: P rows + P rows in flight + P taps per column
constexpr unsigned kGenElems = 4096;         // outputs one workgroup of the general kernel folds: 16 per lane

struct ChanCall {
    const float2 *in, *hist;   // hist: L - D samples in front of in[0], or null (zeros)
    float2 *out;
    const float *w;            // L taps, device
    size_t nframes;
    unsigned M, D, P;
    unsigned tile;             // frames per tile
    unsigned lx_log2;          // ring: lanes of a workgroup along the columns = 1 << lx_log2, the rest along the tiles
    unsigned ncb;              // column blocks per tile (group); blockIdx.x = tile group * ncb + column block
    aeth::FastDiv fd_ncb, fd_M;
    unsigned stream;           // AETH_CHAN_PHASE_STREAM with D < M
    unsigned g1;               // (first_frame + 1) mod M
};

template <int CW> struct Row;
template <> struct Row<1> { typedef float2 T; };
template <> struct Row<2> { typedef float4 T; };

__device__ __forceinline__ float2 mulw(float2 x, const float *w) { return make_float2(w[0] * x.x, w[0] * x.y); }
__device__ __forceinline__ float4 mulw(float4 x, const float *w) { return make_float4(w[0] * x.x, w[0] * x.y, w[1] * x.z, w[1] * x.w); }
__device__ __forceinline__ float2 addv(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float4 addv(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// ---- hop == M, P <= kRingMaxP ----------------------------------------------------------------------------------------
// Stream row R (M samples) feeds frames R .. R + P - 1 with taps P - 1 .. 0.  Row k of the tile (k = 0 is stream row
// m0 + 1 - P) lives in ring slot k % P; the loop is unrolled over U steps (a multiple of P), so every slot is a
// register.  The U rows of a round are loaded before the first of them is used: U loads in flight per lane.
template <int P, int CW, bool NT> __global__ __launch_bounds__(kBlock, 4) void chan_ring_kernel(ChanCall a)
{
    typedef typename Row<CW>::T V;
    constexpr int U = P >= 4 ? P : (P == 3 ? 6 : 4);
    const unsigned tg = aeth::fdiv(blockIdx.x, a.fd_ncb), cb = blockIdx.x - tg * a.ncb;
    const unsigned lx = threadIdx.x & ((1u << a.lx_log2) - 1u), ly = threadIdx.x >> a.lx_log2;
    const size_t col = (((size_t)cb << a.lx_log2) + lx) * CW;
    const size_t M = a.M;
    const size_t m0 = ((size_t)tg * (kBlock >> a.lx_log2) + ly) * a.tile;
    if (col >= M || m0 >= a.nframes) return;
    const size_t m1 = m0 + a.tile < a.nframes ? m0 + a.tile : a.nframes;

    float wt[P][CW];
#pragma unroll
    for (int p = 0; p < P; p++)
#pragma unroll
        for (int c = 0; c < CW; c++) wt[p][c] = a.w[(size_t)p * M + col + c];

    V ring[P];
#pragma unroll
    for (int k = 0; k < P - 1; k++) {
        const ptrdiff_t R = (ptrdiff_t)m0 + 1 - P + k;
        V v = {};
        if (R >= 0) v = aeth::nt_load<NT>(reinterpret_cast<const V *>(a.in + (size_t)R * M + col));
        else if (a.hist) v = *reinterpret_cast<const V *>(a.hist + (size_t)(R + P - 1) * M + col);
        ring[k] = v;
    }
    for (size_t m = m0; m < m1; m += U) {
        V nw[U];
#pragma unroll
        for (int j = 0; j < U; j++) {
            const size_t R = m + j < m1 ? m + j : m1 - 1;          // past the tile: a row that exists, never stored
            nw[j] = aeth::nt_load<NT>(reinterpret_cast<const V *>(a.in + R * M + col));
        }
#pragma unroll
        for (int j = 0; j < U; j++) {
            ring[(P - 1 + j) % P] = nw[j];
            V acc = mulw(ring[j % P], wt[0]);
#pragma unroll
            for (int p = 1; p < P; p++) acc = addv(acc, mulw(ring[(j + p) % P], wt[p]));
            if (m + j < m1) aeth::nt_store<NT>(reinterpret_cast<V *>(a.out + (m + j) * M + col), acc);
        }
    }
}

// ---- every other shape -----------------------------------------------------------------------------------------------
// A workgroup folds `tile` whole frames (M <= 2048: tile * M <= kGenElems) or kGenElems columns of one frame.
template <bool NT> __global__ __launch_bounds__(kBlock, 4) void chan_gen_kernel(ChanCall a)
{
    const unsigned tg = aeth::fdiv(blockIdx.x, a.fd_ncb), cb = blockIdx.x - tg * a.ncb;
    const unsigned M = a.M, D = a.D, P = a.P;
    const size_t m0 = (size_t)tg * a.tile;
    const unsigned c0 = cb * kGenElems;
    const unsigned ncols = M - c0 < kGenElems ? M - c0 : kGenElems;          // == M when tile > 1
    const unsigned nfr = a.nframes - m0 < a.tile ? (unsigned)(a.nframes - m0) : a.tile;
    const unsigned total = nfr * ncols;
    const size_t L = (size_t)P * M;
    unsigned rot0 = 0;
    if (a.stream) {
        const uint64_t g = ((uint64_t)a.g1 + m0 % M) % M;                    // (first_frame + m0 + 1) mod M
        rot0 = (unsigned)((g * D) % M);
    }
    for (unsigned e = threadIdx.x; e < total; e += kBlock) {
        const unsigned lf = a.tile > 1 ? aeth::fdiv(e, a.fd_M) : 0u;         // frame of the tile
        const unsigned q = c0 + e - lf * ncols;
        unsigned rot = 0;
        if (a.stream) {
            const unsigned t = rot0 + lf * D;                                // < M + kGenElems
            rot = t - aeth::fdiv(t, a.fd_M) * M;
        }
        const unsigned r = q >= rot ? q - rot : q + M - rot;
        const size_t m = m0 + lf;
        ptrdiff_t i = (ptrdiff_t)((m + 1) * D) - (ptrdiff_t)L + r;           // s index of the p = 0 sample
        const float *w = a.w + r;
        float2 acc = make_float2(0.f, 0.f);
#pragma unroll 4
        for (unsigned p = 0; p < P; p++, i += M, w += M) {
            float2 x = make_float2(0.f, 0.f);
            if (i >= 0) x = a.in[i];
            else if (a.hist) x = a.hist[(ptrdiff_t)(L - D) + i];
            const float2 pr = mulw(x, w);
            acc = p == 0 ? pr : addv(acc, pr);
        }
        aeth::nt_store<NT>(a.out + m * M + q, acc);
    }
}

typedef void (*ChanKernel)(ChanCall);

template <int CW, bool NT> ChanKernel ring_kernel(unsigned P)
{
    switch (P) {
    case 1: return chan_ring_kernel<1, CW, NT>;
    case 2: return chan_ring_kernel<2, CW, NT>;
    case 3: return chan_ring_kernel<3, CW, NT>;
    case 4: return chan_ring_kernel<4, CW, NT>;
    case 5: return chan_ring_kernel<5, CW, NT>;
    case 6: return chan_ring_kernel<6, CW, NT>;
    case 7: return chan_ring_kernel<7, CW, NT>;
    default: return chan_ring_kernel<8, CW, NT>;
    }
}

bool touch_bytes(const void *a, size_t na, const void *b, size_t nb)
{
    if (!a || !b || !na || !nb) return false;
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + na, b0 = (uintptr_t)b, b1 = b0 + nb;
    return a0 < b1 && b0 < a1;
}

}  // namespace

namespace {

int ensure_scratch(aeth_chan *c, size_t elems)
{
    if (c->scratch_elems >= elems) return AETH_OK;
    aeth::DeviceGuard dg(c->ctx->device);
    if (c->scratch) {
        AETH_HIP(hipStreamSynchronize(aeth::ctx_stream(c->ctx)));
        AETH_HIP(hipFree(c->scratch));
        c->scratch = nullptr;
        c->scratch_elems = 0;
    }
    AETH_HIP(hipMalloc((void **)&c->scratch, elems * sizeof(float2)));
    c->scratch_elems = elems;
    return AETH_OK;
}

}  // namespace

// workgroups of a launch over F frames, at most (the ring kernel with one column per lane)
size_t aeth::chan_grid_bound(const aeth_chan *c, size_t F)
{
    const size_t ntiles = (F + c->tile - 1) / c->tile;
    if (!c->ring) return ntiles * ((c->M + kGenElems - 1) / kGenElems);
    size_t lx = 1;
    while (lx < (size_t)kBlock && lx < c->M) lx *= 2;
    return ((ntiles + kBlock / lx - 1) / (kBlock / lx)) * ((c->M + lx - 1) / lx);
}

void aeth::chan_geometry(aeth_chan *c)
{
    c->ring = c->D == c->M && c->P <= kRingMaxP;
    if (c->ring) {
        // P - 1 halo rows per tile: a sixteenth of the tile at most (P = 2: 1 of 16, P = 8: 7 of 128)
        c->tile = 16;
        while (c->tile < 16 * (c->P - 1)) c->tile *= 2;
    } else {
        c->tile = c->M <= kGenElems / 2 ? kGenElems / c->M : 1;
    }
}

namespace {

// what every exec call checks before any device work; out_elem_bytes: size of the caller's output range
int check_call(const aeth_chan *c, const aeth_cf32 *hist, const aeth_cf32 *in, size_t n, const void *out, size_t n_out,
               size_t out_elem_bytes, size_t *nframes)
{
    AETH_REQUIRE(c, AETH_E_ARG, "chan is null");
    AETH_REQUIRE(n > 0, AETH_E_LEN, "0 input samples: a call makes at least one frame of hop %zu", c->D);
    AETH_REQUIRE(n % c->D == 0, AETH_E_LEN, "%zu input samples are not a multiple of the hop %zu", n, c->D);
    const size_t F = n / c->D;
    AETH_REQUIRE(F <= SIZE_MAX / 16 / c->M && n_out == F * c->M, AETH_E_LEN, "output holds %zu elements, %zu frames x %zu channels give %zu",
                 n_out, F, c->M, F <= SIZE_MAX / 16 / c->M ? F * c->M : (size_t)0);
    AETH_REQUIRE(in && out, AETH_E_ARG, "null pointer");
    AETH_REQUIRE(aeth::aligned8(in) && aeth::aligned8(hist), AETH_E_ALIGN, "input or history pointer not 8-byte aligned");
    AETH_REQUIRE(((uintptr_t)out & (out_elem_bytes - 1)) == 0, AETH_E_ALIGN, "output pointer not %zu-byte aligned", out_elem_bytes);
    AETH_REQUIRE(!touch_bytes(out, n_out * out_elem_bytes, in, n * sizeof(aeth_cf32)) &&
                 !touch_bytes(out, n_out * out_elem_bytes, hist, (c->L - c->D) * sizeof(aeth_cf32)), AETH_E_ARG,
                 "the output range overlaps the input (or its history)");
    AETH_REQUIRE(aeth::chan_grid_bound(c, F) < ((size_t)1 << 31), AETH_E_UNSUPPORTED, "%zu frames in one call: more than 2^31 workgroups", F);
    *nframes = F;
    return AETH_OK;
}

}  // namespace

int aeth::chan_launch_fold(const aeth_chan *c, const aeth_cf32 *hist, const aeth_cf32 *in, size_t F, uint64_t first_frame, float2 *out)
{
    ChanCall a{};
    a.in = (const float2 *)in;
    a.hist = c->L > c->D ? (const float2 *)hist : nullptr;
    a.out = out;
    a.w = c->w_dev;
    a.nframes = F;
    a.M = (unsigned)c->M; a.D = (unsigned)c->D; a.P = (unsigned)c->P;
    a.tile = (unsigned)c->tile;
    a.fd_M = aeth::make_fastdiv(a.M);
    a.stream = c->phase == AETH_CHAN_PHASE_STREAM && c->D < c->M;
    a.g1 = (unsigned)((first_frame % c->M + 1) % c->M);
    const size_t ntiles = (F + c->tile - 1) / c->tile;
    const size_t moved = (F * c->M + F * c->D) * sizeof(float2);
    const bool nt = aeth::streams_past_cache(moved);
    ChanKernel k;
    size_t grid;
    if (c->ring) {
        const bool wide = c->M % 2 == 0 && aeth::aligned16(in) && aeth::aligned16(out) && aeth::aligned16(a.hist);
        const size_t lanes = wide ? c->M / 2 : c->M;                 // lanes along the columns
        while ((1u << a.lx_log2) < kBlock && ((size_t)1 << a.lx_log2) < lanes) a.lx_log2++;
        a.ncb = (unsigned)((lanes + (1u << a.lx_log2) - 1) >> a.lx_log2);
        const size_t ly = kBlock >> a.lx_log2;
        grid = ((ntiles + ly - 1) / ly) * a.ncb;
        k = wide ? (nt ? ring_kernel<2, true>(a.P) : ring_kernel<2, false>(a.P)) : (nt ? ring_kernel<1, true>(a.P) : ring_kernel<1, false>(a.P));
    } else {
        a.ncb = (unsigned)((c->M + kGenElems - 1) / kGenElems);
        grid = ntiles * a.ncb;
        k = nt ? chan_gen_kernel<true> : chan_gen_kernel<false>;
    }
    a.fd_ncb = aeth::make_fastdiv(a.ncb);
    aeth::DeviceGuard dg(c->ctx->device);
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(kBlock), 0, aeth::ctx_stream(c->ctx), a);
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

extern "C" {

int aeth_chan_prototype(int kind, size_t channels, size_t taps_per_channel, float *out_host)
{
    AETH_REQUIRE(kind >= AETH_CHAN_PROTO_RECT && kind <= AETH_CHAN_PROTO_SINC_HAMMING, AETH_E_ARG, "bad prototype kind %d", kind);
    AETH_REQUIRE(channels >= 1 && taps_per_channel >= 1, AETH_E_ARG, "prototype of %zu channels x %zu taps per channel: both at least 1",
                 channels, taps_per_channel);
    AETH_REQUIRE(channels <= (SIZE_MAX / sizeof(double)) / taps_per_channel, AETH_E_ARG, "%zu channels x %zu taps per channel overflow",
                 channels, taps_per_channel);
    AETH_REQUIRE(out_host, AETH_E_ARG, "out is null");
    const size_t L = channels * taps_per_channel;
    const double pi = 3.14159265358979323846, dL = (double)L, dM = (double)channels;
    if (kind == AETH_CHAN_PROTO_SINC_HAMMING) {
        if (L == 1) { out_host[0] = 1.0f; return AETH_OK; }
        double *h = new (std::nothrow) double[L];
        AETH_REQUIRE(h, AETH_E_NOMEM, "out of host memory");
        double sum = 0.0;
        for (size_t n = 0; n < L; n++) {
            const double t = ((double)n - (dL - 1.0) / 2.0) / dM, x = pi * t;
            const double sinc = t == 0.0 ? 1.0 : std::sin(x) / x;
            h[n] = sinc * (0.54 - 0.46 * std::cos(2.0 * pi * (double)n / (dL - 1.0)));
            sum += h[n];
        }
        for (size_t n = 0; n < L; n++) out_host[n] = (float)(h[n] / sum);
        delete[] h;
        return AETH_OK;
    }
    for (size_t n = 0; n < L; n++) {
        const double c = std::cos(2.0 * pi * (double)n / dL);
        out_host[n] = kind == AETH_CHAN_PROTO_RECT ? 1.0f : (float)(kind == AETH_CHAN_PROTO_HANN ? 0.5 - 0.5 * c : 0.54 - 0.46 * c);
    }
    return AETH_OK;
}

int aeth_chan_create(aeth_ctx *ctx, const float *proto_host, size_t ntaps, size_t channels, size_t hop, int phase,
                     size_t max_frames, aeth_chan **out)
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
    aeth_fft *fft = nullptr;
    int rc = aeth_fft_create(ctx, channels, max_frames, &fft); if (rc) return rc;      // names the refused length
    aeth_chan *c = new (std::nothrow) aeth_chan();
    if (!c) { (void)aeth_fft_destroy(fft); return aeth::set_error(AETH_E_NOMEM, "out of host memory"); }
    c->ctx = ctx; c->fft = fft;
    c->M = channels; c->L = ntaps; c->P = ntaps / channels; c->D = hop; c->phase = phase;
    aeth::chan_geometry(c);
    aeth::DeviceGuard dg(ctx->device);
    hipError_t e = hipMalloc((void **)&c->w_dev, ntaps * sizeof(float));
    if (e == hipSuccess) e = hipMemcpyAsync(c->w_dev, proto_host, ntaps * sizeof(float), hipMemcpyHostToDevice, aeth::ctx_stream(ctx));
    if (e == hipSuccess) e = hipStreamSynchronize(aeth::ctx_stream(ctx));
    if (e != hipSuccess) { (void)aeth_chan_destroy(c); return aeth::hip_fail(e, "aeth_chan_create: prototype upload"); }
    if (max_frames > 0 && max_frames <= SIZE_MAX / 16 / channels) {
        rc = ensure_scratch(c, max_frames * channels);
        if (rc) { (void)aeth_chan_destroy(c); return rc; }
    }
    *out = c;
    return AETH_OK;
}

int aeth_chan_destroy(aeth_chan *c)
{
    if (!c) return AETH_OK;
    (void)aeth_fft_destroy(c->fft);          // waits for the context's stream
    aeth::DeviceGuard dg(c->ctx->device);
    if (c->w_dev) (void)hipFree(c->w_dev);
    if (c->scratch) (void)hipFree(c->scratch);
    delete c;
    return AETH_OK;
}

size_t aeth_chan_channels(const aeth_chan *c) { return c ? c->M : 0; }
size_t aeth_chan_ntaps(const aeth_chan *c) { return c ? c->L : 0; }
size_t aeth_chan_hop(const aeth_chan *c) { return c ? c->D : 0; }
int aeth_chan_phase(const aeth_chan *c) { return c ? c->phase : 0; }
const char *aeth_chan_route(const aeth_chan *c) { return c ? aeth_fft_route(c->fft) : ""; }
size_t aeth_chan_tile(const aeth_chan *c) { return c ? c->tile : 0; }

int aeth_chan_fold(aeth_chan *c, const aeth_cf32 *hist, const aeth_cf32 *in, size_t n, uint64_t first_frame, aeth_cf32 *out,
                   size_t n_out)
{
    size_t F = 0;
    int rc = check_call(c, hist, in, n, out, n_out, sizeof(aeth_cf32), &F); if (rc) return rc;
    return aeth::chan_launch_fold(c, hist, in, F, first_frame, (float2 *)out);
}

int aeth_chan_exec(aeth_chan *c, const aeth_cf32 *hist, const aeth_cf32 *in, size_t n, uint64_t first_frame, int sign,
                   int scale_kind, float x, aeth_cf32 *out, size_t n_out)
{
    size_t F = 0;
    int rc = check_call(c, hist, in, n, out, n_out, sizeof(aeth_cf32), &F); if (rc) return rc;
    AETH_REQUIRE(sign == AETH_SIGN_REF_FWD || sign == AETH_SIGN_REF_BWD, AETH_E_ARG, "sign must be +1 or -1");
    AETH_REQUIRE(scale_kind >= AETH_SCALE_NONE && scale_kind <= AETH_SCALE_X, AETH_E_ARG, "bad scale kind %d", scale_kind);
    rc = ensure_scratch(c, n_out); if (rc) return rc;
    rc = aeth::chan_launch_fold(c, hist, in, F, first_frame, c->scratch); if (rc) return rc;
    return aeth_fft_exec(c->fft, (const aeth_cf32 *)c->scratch, n_out, out, F, sign, scale_kind, x);
}

int aeth_chan_exec_levels(aeth_chan *c, const aeth_cf32 *hist, const aeth_cf32 *in, size_t n, uint64_t first_frame, int sign,
                          int scale_kind, float x, int mirror, int level_kind, float *levels, size_t n_levels)
{
    size_t F = 0;
    int rc = check_call(c, hist, in, n, levels, n_levels, sizeof(float), &F); if (rc) return rc;
    AETH_REQUIRE(sign == AETH_SIGN_REF_FWD || sign == AETH_SIGN_REF_BWD, AETH_E_ARG, "sign must be +1 or -1");
    AETH_REQUIRE(scale_kind >= AETH_SCALE_NONE && scale_kind <= AETH_SCALE_X, AETH_E_ARG, "bad scale kind %d", scale_kind);
    AETH_REQUIRE(aeth::level_kind_ok(level_kind), AETH_E_ARG, "bad level kind %d", level_kind);
    rc = ensure_scratch(c, n_levels); if (rc) return rc;
    rc = aeth::chan_launch_fold(c, hist, in, F, first_frame, c->scratch); if (rc) return rc;
    return aeth_fft_exec_levels(c->fft, (const aeth_cf32 *)c->scratch, n_levels, F, sign, scale_kind, x, mirror, level_kind, levels,
                                n_levels);
}

}  // extern "C"
