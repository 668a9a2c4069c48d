// aeth_synth.hip -- polyphase synthesis filter bank: weighted overlap-add behind the batched inverse FFT, the transpose
// of aeth_chan.hip (the reference has no synthesis: src/util/plot.rs:46-68 only takes a stream apart).
// Frame m (M samples) is extended periodically to L = P * M, weighted by the real prototype g and added into the output
// at m * D: out[i] = sum over m ascending with 0 <= i - m D < L of g[j] * v_m[(j + rot_m) mod M], j = i - m D (every
// product and every sum rounded: EXACT flags).  K = ceil(L / D) frames touch one output.  Three routes:
//   fold     D == M: the sum is aeth_chan_fold of the row-reversed prototype; no kernel here (aeth_chan_fold.h).
//   ring     D < M, D divides L, K <= 8: a lane owns output offset d of every hop (8-byte accesses) or d and d + 1
//            (16-byte accesses), keeps the K - 1 open accumulators in registers and walks a tile of frames oldest
//            first: frame m gives g[k D + d] * v_m[..] to the accumulator of hop m + k, the first contribution assigns,
//            hop m is then complete and stored.  K - 1 halo frames per tile.
//   general  everything else: a lane owns output i and gathers its (at most K) terms in ascending m; absent terms are
//            skipped, never added as zeros; the P-fold re-read of a frame is served by L2.
#include "aeth_internal.h"
#include "aeth_chan_fold.h"
#include "aeth_fft_plan.h"

#include <new>

namespace {

constexpr int kBlock = 256;
constexpr unsigned kMaxP = 64;
constexpr unsigned kMaxK = 256;
constexpr unsigned kRingMaxK = 8;            // the register ring: K - 1 accumulators + K taps + K offsets per lane
constexpr unsigned kGenElems = 4096;         // outputs one workgroup of the general kernel gathers: 16 per lane
constexpr int kInFlight = 16;                // 8-byte words a lane of the ring loads before it uses the first

struct SynthCall {
    const float2 *in, *hist;   // hist: K - 1 frames in front of in[0] (oldest first), or null (zeros)
    float2 *out;
    const float *g;            // L taps, device
    size_t nframes;
    unsigned M, D, K;
    unsigned L;
    unsigned tile;             // hops per tile
    unsigned lx_log2;          // ring: lanes of a workgroup along the offsets = 1 << lx_log2, the rest along the tiles
    unsigned ncb;              // offset blocks per tile (group); blockIdx.x = tile group * ncb + offset block
    aeth::FastDiv fd_ncb, fd_M, fd_D;
    unsigned stream;           // AETH_CHAN_PHASE_STREAM (D < M on both routes here)
    unsigned g1;               // (first_frame + 1) mod M
};

template <int CW> struct Row;
template <> struct Row<1> { typedef float2 T; };
template <> struct Row<2> { typedef float4 T; };

__device__ __forceinline__ float2 mulw(float2 x, const float *w) { return make_float2(w[0] * x.x, w[0] * x.y); }
__device__ __forceinline__ float4 mulw(float4 x, const float *w) { return make_float4(w[0] * x.x, w[0] * x.y, w[1] * x.z, w[1] * x.w); }
__device__ __forceinline__ float2 addv(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float4 addv(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// ((g1 + m) mod M) * D mod M for any frame number m >= -(K - 1): rot of frame m when frame 0 is first_frame
__device__ __forceinline__ unsigned rot_of(const SynthCall &a, ptrdiff_t m)
{
    const ptrdiff_t M = (ptrdiff_t)a.M;
    ptrdiff_t r = m % M;
    if (r < 0) r += M;
    const uint64_t g = ((uint64_t)a.g1 + (uint64_t)r) % a.M;
    return (unsigned)((g * a.D) % a.M);
}

// ---- D < M, D | L, K <= kRingMaxK ------------------------------------------------------------------------------------
// Hop n = m + k takes g[k D + d] * v_m[(k D + d + rot_m) mod M], k = K - 1 (the hop's oldest frame: assigns) .. 0 (its
// newest: the hop is complete).  In front of frame m, acc[s] holds what the frames before m gave to hop m + s,
// s = 0 .. K - 2; frame m completes hop m from acc[0], moves the others one slot down and opens hop m + K - 1.  The loop
// takes R frames a round: their R * K loads are in flight before the first of them is used.
template <int K, int CW, bool NT> __global__ __launch_bounds__(kBlock, 4) void synth_ring_kernel(SynthCall a)
{
    typedef typename Row<CW>::T V;
    constexpr int R = kInFlight / (K * CW) < 1 ? 1 : (kInFlight / (K * CW) > 4 ? 4 : kInFlight / (K * CW));
    const unsigned tg = aeth::fdiv(blockIdx.x, a.fd_ncb), cb = blockIdx.x - tg * a.ncb;
    const unsigned lx = threadIdx.x & ((1u << a.lx_log2) - 1u), ly = threadIdx.x >> a.lx_log2;
    const unsigned d = ((cb << a.lx_log2) + lx) * CW;
    const unsigned M = a.M, D = a.D;
    const size_t n0 = ((size_t)tg * (kBlock >> a.lx_log2) + ly) * a.tile;
    if (d >= D || n0 >= a.nframes) return;
    const size_t n1 = n0 + a.tile < a.nframes ? n0 + a.tile : a.nframes;

    float gt[K][CW];
    unsigned off[K];           // (k D + d) mod M
#pragma unroll
    for (int k = 0; k < K; k++) {
        const unsigned j = (unsigned)k * D + d;
        off[k] = j - aeth::fdiv(j, a.fd_M) * M;
#pragma unroll
        for (int c = 0; c < CW; c++) gt[k][c] = a.g[j + c];
    }
    unsigned rot = a.stream ? rot_of(a, (ptrdiff_t)n0 - (K - 1)) : 0u;

    // the K - 1 frames in front of the tile open hops n0 .. n0 + K - 2; what they give to older hops leaves through
    // slot 0 unused.  A rolled loop: the tile's first loads are not held up behind K (K - 1) / 2 halo loads in flight.
    V acc[K - 1] = {};
#pragma unroll 1
    for (int h = 0; h < K - 1; h++) {
        const ptrdiff_t m = (ptrdiff_t)n0 - (K - 1) + h;
        const float2 *row = m >= 0 ? a.in + (size_t)m * M : (a.hist ? a.hist + (size_t)(m + (K - 1)) * M : nullptr);
        V v[K] = {};           // a history of zeros is multiplied like any other frame
        if (row) {
#pragma unroll
            for (int k = 1; k < K; k++) {
                unsigned e = off[k] + rot;
                if (e >= M) e -= M;
                v[k] = *reinterpret_cast<const V *>(row + e);
            }
        }
#pragma unroll
        for (int s = 0; s < K - 2; s++) acc[s] = addv(acc[s + 1], mulw(v[s + 1], gt[s + 1]));
        acc[K - 2] = mulw(v[K - 1], gt[K - 1]);
        if (a.stream) { rot += D; if (rot >= M) rot -= M; }
    }
#pragma unroll 1
    for (size_t n = n0; n < n1; n += R) {
        V nw[R][K];
#pragma unroll
        for (int jj = 0; jj < R; jj++) {
            const size_t m = n + jj < n1 ? n + jj : n1 - 1;          // past the tile: a frame that exists, never stored
            const float2 *row = a.in + m * M;
#pragma unroll
            for (int k = 0; k < K; k++) {
                unsigned e = off[k] + rot;
                if (e >= M) e -= M;
                nw[jj][k] = aeth::nt_load<NT>(reinterpret_cast<const V *>(row + e));
            }
            if (a.stream) { rot += D; if (rot >= M) rot -= M; }
        }
#pragma unroll
        for (int jj = 0; jj < R; jj++) {
            const V done = addv(acc[0], mulw(nw[jj][0], gt[0]));
#pragma unroll
            for (int s = 0; s < K - 2; s++) acc[s] = addv(acc[s + 1], mulw(nw[jj][s + 1], gt[s + 1]));
            acc[K - 2] = mulw(nw[jj][K - 1], gt[K - 1]);
            if (n + jj < n1) aeth::nt_store<NT>(reinterpret_cast<V *>(a.out + (n + jj) * D + d), done);
        }
    }
}

// ---- every other shape with D < M -----------------------------------------------------------------------------------
// A workgroup gathers `tile` whole hops (D <= 2048: tile * D <= kGenElems) or kGenElems offsets of one hop.
template <bool NT> __global__ __launch_bounds__(kBlock, 4) void synth_gen_kernel(SynthCall a)
{
    const unsigned tg = aeth::fdiv(blockIdx.x, a.fd_ncb), cb = blockIdx.x - tg * a.ncb;
    const unsigned M = a.M, D = a.D, K = a.K, L = a.L;
    const size_t n0 = (size_t)tg * a.tile;
    const unsigned c0 = cb * kGenElems;
    const unsigned ncols = D - c0 < kGenElems ? D - c0 : kGenElems;          // == D when tile > 1
    const unsigned nh = a.nframes - n0 < a.tile ? (unsigned)(a.nframes - n0) : a.tile;
    const unsigned total = nh * ncols;
    const unsigned rot0 = a.stream ? rot_of(a, (ptrdiff_t)n0 - (ptrdiff_t)(K - 1)) : 0u;   // of the oldest frame of hop n0
    for (unsigned e = threadIdx.x; e < total; e += kBlock) {
        const unsigned lf = a.tile > 1 ? aeth::fdiv(e, a.fd_D) : 0u;         // hop of the tile
        const unsigned d = c0 + e - lf * ncols;
        unsigned rot = 0;
        if (a.stream) {
            const unsigned t = rot0 + lf * D;                                // < M + kGenElems
            rot = t - aeth::fdiv(t, a.fd_M) * M;
        }
        unsigned j = (K - 1) * D + d;                                        // < L + D
        unsigned jm = j - aeth::fdiv(j, a.fd_M) * M;                         // j mod M
        ptrdiff_t m = (ptrdiff_t)(n0 + lf) - (ptrdiff_t)(K - 1);
        float2 acc = make_float2(0.f, 0.f);
        bool first = true;
#pragma unroll 4
        for (unsigned k = 0; k < K; k++, m++, j -= D) {
            if (j < L) {
                unsigned q = jm + rot;
                if (q >= M) q -= M;
                float2 x = make_float2(0.f, 0.f);
                if (m >= 0) x = a.in[(size_t)m * M + q];
                else if (a.hist) x = a.hist[(size_t)(m + (ptrdiff_t)(K - 1)) * M + q];
                const float2 pr = mulw(x, a.g + j);
                acc = first ? pr : addv(acc, pr);
                first = false;
            }
            jm = jm >= D ? jm - D : jm + M - D;
            if (a.stream) { rot += D; if (rot >= M) rot -= M; }
        }
        aeth::nt_store<NT>(a.out + (n0 + lf) * D + d, acc);
    }
}

typedef void (*SynthKernel)(SynthCall);

template <int CW, bool NT> SynthKernel ring_kernel(unsigned K)
{
    switch (K) {
    case 2: return synth_ring_kernel<2, CW, NT>;
    case 3: return synth_ring_kernel<3, CW, NT>;
    case 4: return synth_ring_kernel<4, CW, NT>;
    case 5: return synth_ring_kernel<5, CW, NT>;
    case 6: return synth_ring_kernel<6, CW, NT>;
    case 7: return synth_ring_kernel<7, CW, NT>;
    default: return synth_ring_kernel<8, CW, NT>;
    }
}

bool touch_bytes(const void *a, size_t na, const void *b, size_t nb)
{
    if (!a || !b || !na || !nb) return false;
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + na, b0 = (uintptr_t)b, b1 = b0 + nb;
    return a0 < b1 && b0 < a1;
}

enum { ROUTE_FOLD = 0, ROUTE_RING = 1, ROUTE_GEN = 2 };

}  // namespace

struct aeth_synth {
    aeth_ctx *ctx = nullptr;
    size_t M = 0, L = 0, P = 0, D = 0, K = 0;
    int phase = 0;
    int kind = ROUTE_GEN;
    size_t tile = 0;
    float *g_dev = nullptr;      // the prototype; on the fold route its rows reversed
    aeth_chan fold;              // the fold route's view of this object (owns nothing)
    aeth_fft *fft = nullptr;
    float2 *scratch = nullptr;   // the (K - 1 + F) * M time samples of exec, grown on demand
    size_t scratch_elems = 0;
};

namespace {

int ensure_scratch(aeth_synth *s, size_t elems)
{
    if (s->scratch_elems >= elems) return AETH_OK;
    aeth::DeviceGuard dg(s->ctx->device);
    if (s->scratch) {
        AETH_HIP(hipStreamSynchronize(aeth::ctx_stream(s->ctx)));
        AETH_HIP(hipFree(s->scratch));
        s->scratch = nullptr;
        s->scratch_elems = 0;
    }
    AETH_HIP(hipMalloc((void **)&s->scratch, elems * sizeof(float2)));
    s->scratch_elems = elems;
    return AETH_OK;
}

// workgroups of a launch over F frames, at most (the ring kernel with one offset per lane)
size_t grid_bound(const aeth_synth *s, size_t F)
{
    if (s->kind == ROUTE_FOLD) return aeth::chan_grid_bound(&s->fold, F);
    const size_t ntiles = (F + s->tile - 1) / s->tile;
    if (s->kind == ROUTE_GEN) return ntiles * ((s->D + kGenElems - 1) / kGenElems);
    size_t lx = 1;
    while (lx < (size_t)kBlock && lx < s->D) lx *= 2;
    return ((ntiles + kBlock / lx - 1) / (kBlock / lx)) * ((s->D + lx - 1) / lx);
}

// what unfold and exec check before any device work
int check_call(const aeth_synth *s, const aeth_cf32 *hist, const aeth_cf32 *in, size_t n, const aeth_cf32 *out, size_t n_out,
               size_t *nframes)
{
    AETH_REQUIRE(s, AETH_E_ARG, "synth is null");
    AETH_REQUIRE(n > 0, AETH_E_LEN, "0 input samples: a call takes at least one frame of %zu channels", s->M);
    AETH_REQUIRE(n % s->M == 0, AETH_E_LEN, "%zu input samples are not a multiple of the %zu channels", n, s->M);
    const size_t F = n / s->M;
    AETH_REQUIRE(F <= SIZE_MAX / 16 / s->M - s->K && n_out == F * s->D, AETH_E_LEN, "output holds %zu elements, %zu frames x hop %zu give %zu",
                 n_out, F, s->D, F <= SIZE_MAX / 16 / s->M - s->K ? F * s->D : (size_t)0);
    AETH_REQUIRE(in && out, AETH_E_ARG, "null pointer");
    AETH_REQUIRE(aeth::aligned8(in) && aeth::aligned8(hist), AETH_E_ALIGN, "input or history pointer not 8-byte aligned");
    AETH_REQUIRE(aeth::aligned8(out), AETH_E_ALIGN, "output pointer not 8-byte aligned");
    AETH_REQUIRE(!touch_bytes(out, n_out * sizeof(aeth_cf32), in, n * sizeof(aeth_cf32)) &&
                 !touch_bytes(out, n_out * sizeof(aeth_cf32), hist, (s->K - 1) * s->M * sizeof(aeth_cf32)), AETH_E_ARG,
                 "the output range overlaps the input (or its history)");
    AETH_REQUIRE(grid_bound(s, F) < ((size_t)1 << 31), AETH_E_UNSUPPORTED, "%zu frames in one call: more than 2^31 workgroups", F);
    *nframes = F;
    return AETH_OK;
}

int launch_unfold(aeth_synth *s, const aeth_cf32 *hist, const aeth_cf32 *in, size_t F, uint64_t first_frame, float2 *out)
{
    if (s->kind == ROUTE_FOLD) return aeth::chan_launch_fold(&s->fold, hist, in, F, first_frame, out);
    SynthCall a{};
    a.in = (const float2 *)in;
    a.hist = (const float2 *)hist;               // K >= 2 on both routes
    a.out = out;
    a.g = s->g_dev;
    a.nframes = F;
    a.M = (unsigned)s->M; a.D = (unsigned)s->D; a.K = (unsigned)s->K; a.L = (unsigned)s->L;
    a.tile = (unsigned)s->tile;
    a.fd_M = aeth::make_fastdiv(a.M);
    a.fd_D = aeth::make_fastdiv(a.D);
    a.stream = s->phase == AETH_CHAN_PHASE_STREAM;
    a.g1 = (unsigned)((first_frame % s->M + 1) % s->M);
    const size_t ntiles = (F + s->tile - 1) / s->tile;
    const size_t moved = (F * s->M + F * s->D) * sizeof(float2);
    const bool nt = aeth::streams_past_cache(moved);
    SynthKernel k;
    size_t grid;
    if (s->kind == ROUTE_RING) {
        // pairs need even offsets at even positions of 16-byte aligned rows: D and M even (rot is then even too)
        const bool wide = s->D % 2 == 0 && s->M % 2 == 0 && aeth::aligned16(in) && aeth::aligned16(out) && aeth::aligned16(hist);
        const size_t lanes = wide ? s->D / 2 : s->D;                 // lanes along the offsets
        while ((1u << a.lx_log2) < kBlock && ((size_t)1 << a.lx_log2) < lanes) a.lx_log2++;
        a.ncb = (unsigned)((lanes + (1u << a.lx_log2) - 1) >> a.lx_log2);
        const size_t ly = kBlock >> a.lx_log2;
        grid = ((ntiles + ly - 1) / ly) * a.ncb;
        k = wide ? (nt ? ring_kernel<2, true>(a.K) : ring_kernel<2, false>(a.K)) : (nt ? ring_kernel<1, true>(a.K) : ring_kernel<1, false>(a.K));
    } else {
        a.ncb = (unsigned)((s->D + kGenElems - 1) / kGenElems);
        grid = ntiles * a.ncb;
        k = nt ? synth_gen_kernel<true> : synth_gen_kernel<false>;
    }
    a.fd_ncb = aeth::make_fastdiv(a.ncb);
    aeth::DeviceGuard dg(s->ctx->device);
    hipLaunchKernelGGL(k, dim3((unsigned)grid), dim3(kBlock), 0, aeth::ctx_stream(s->ctx), a);
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

}  // namespace

extern "C" {

int aeth_synth_create(aeth_ctx *ctx, const float *proto_host, size_t ntaps, size_t channels, size_t hop, int phase,
                      size_t max_frames, aeth_synth **out)
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
    const size_t K = (ntaps + hop - 1) / hop;
    AETH_REQUIRE(K <= kMaxK, AETH_E_UNSUPPORTED, "%zu taps at hop %zu: %zu frames overlap in one output sample, at most %u", ntaps, hop, K,
                 kMaxK);
    aeth_fft *fft = nullptr;
    int rc = aeth_fft_create(ctx, channels, max_frames, &fft); if (rc) return rc;      // names the refused length
    aeth_synth *s = new (std::nothrow) aeth_synth();
    float *rev = hop == channels ? new (std::nothrow) float[ntaps] : nullptr;
    if (!s || (hop == channels && !rev)) {
        delete s; delete[] rev;
        (void)aeth_fft_destroy(fft);
        return aeth::set_error(AETH_E_NOMEM, "out of host memory");
    }
    s->ctx = ctx; s->fft = fft;
    s->M = channels; s->L = ntaps; s->P = ntaps / channels; s->D = hop; s->K = K; s->phase = phase;
    const float *up = proto_host;
    if (hop == channels) {
        // out row n = sum over p ascending of g[(P - 1 - p) M + q] * row_{n - P + 1 + p}[q]: the fold of the reversed rows
        s->kind = ROUTE_FOLD;
        for (size_t p = 0; p < s->P; p++)
            for (size_t q = 0; q < channels; q++) rev[p * channels + q] = proto_host[(s->P - 1 - p) * channels + q];
        up = rev;
        s->fold.ctx = ctx;
        s->fold.M = channels; s->fold.L = ntaps; s->fold.P = s->P; s->fold.D = hop; s->fold.phase = AETH_CHAN_PHASE_FRAME;
        aeth::chan_geometry(&s->fold);
        s->tile = s->fold.tile;
    } else if (ntaps % hop == 0 && K <= kRingMaxK) {
        // K - 1 halo frames per tile: a sixteenth of the tile at most (K = 2: 1 of 16, K = 8: 7 of 128)
        s->kind = ROUTE_RING;
        s->tile = 16;
        while (s->tile < 16 * (K - 1)) s->tile *= 2;
    } else {
        s->kind = ROUTE_GEN;
        s->tile = hop <= kGenElems / 2 ? kGenElems / hop : 1;
    }
    aeth::DeviceGuard dg(ctx->device);
    hipError_t e = hipMalloc((void **)&s->g_dev, ntaps * sizeof(float));
    if (e == hipSuccess) e = hipMemcpyAsync(s->g_dev, up, ntaps * sizeof(float), hipMemcpyHostToDevice, aeth::ctx_stream(ctx));
    if (e == hipSuccess) e = hipStreamSynchronize(aeth::ctx_stream(ctx));
    delete[] rev;
    s->fold.w_dev = s->g_dev;
    if (e != hipSuccess) { (void)aeth_synth_destroy(s); return aeth::hip_fail(e, "aeth_synth_create: prototype upload"); }
    if (max_frames > 0 && max_frames <= SIZE_MAX / 16 / channels - K) {
        rc = ensure_scratch(s, (K - 1 + max_frames) * channels);
        if (rc) { (void)aeth_synth_destroy(s); return rc; }
    }
    *out = s;
    return AETH_OK;
}

int aeth_synth_destroy(aeth_synth *s)
{
    if (!s) return AETH_OK;
    (void)aeth_fft_destroy(s->fft);          // waits for the context's stream
    aeth::DeviceGuard dg(s->ctx->device);
    if (s->g_dev) (void)hipFree(s->g_dev);
    if (s->scratch) (void)hipFree(s->scratch);
    delete s;
    return AETH_OK;
}

size_t aeth_synth_channels(const aeth_synth *s) { return s ? s->M : 0; }
size_t aeth_synth_ntaps(const aeth_synth *s) { return s ? s->L : 0; }
size_t aeth_synth_hop(const aeth_synth *s) { return s ? s->D : 0; }
int aeth_synth_phase(const aeth_synth *s) { return s ? s->phase : 0; }
const char *aeth_synth_route(const aeth_synth *s) { return s ? aeth_fft_route(s->fft) : ""; }
size_t aeth_synth_tile(const aeth_synth *s) { return s ? s->tile : 0; }
size_t aeth_synth_history(const aeth_synth *s) { return s ? s->K - 1 : 0; }

int aeth_synth_unfold(aeth_synth *s, const aeth_cf32 *hist, const aeth_cf32 *frames, size_t n_in, uint64_t first_frame,
                      aeth_cf32 *out, size_t n_out)
{
    size_t F = 0;
    if (s && s->K == 1) hist = nullptr;
    int rc = check_call(s, hist, frames, n_in, out, n_out, &F); if (rc) return rc;
    return launch_unfold(s, hist, frames, F, first_frame, (float2 *)out);
}

int aeth_synth_exec(aeth_synth *s, const aeth_cf32 *hist, const aeth_cf32 *spec, size_t n_in, uint64_t first_frame, int sign,
                    int scale_kind, float x, aeth_cf32 *out, size_t n_out)
{
    size_t F = 0;
    if (s && s->K == 1) hist = nullptr;
    int rc = check_call(s, hist, spec, n_in, out, n_out, &F); if (rc) return rc;
    AETH_REQUIRE(sign == AETH_SIGN_REF_FWD || sign == AETH_SIGN_REF_BWD, AETH_E_ARG, "sign must be +1 or -1");
    AETH_REQUIRE(scale_kind >= AETH_SCALE_NONE && scale_kind <= AETH_SCALE_X, AETH_E_ARG, "bad scale kind %d", scale_kind);
    const size_t nh = (s->K - 1) * s->M;
    rc = ensure_scratch(s, nh + n_in); if (rc) return rc;
    aeth_cf32 *th = (aeth_cf32 *)s->scratch, *tf = th + nh;
    if (hist) { rc = aeth_fft_exec(s->fft, hist, nh, th, s->K - 1, sign, scale_kind, x); if (rc) return rc; }
    rc = aeth_fft_exec(s->fft, spec, n_in, tf, F, sign, scale_kind, x); if (rc) return rc;
    return launch_unfold(s, hist ? th : nullptr, tf, F, first_frame, (float2 *)out);
}

int aeth_synth_dual_window(const float *w, size_t ntaps, size_t hop, float *out_host)
{
    AETH_REQUIRE(w && out_host, AETH_E_ARG, "null pointer");
    AETH_REQUIRE(ntaps >= 1 && hop >= 1, AETH_E_ARG, "dual window of %zu taps at hop %zu: both at least 1", ntaps, hop);
    AETH_REQUIRE(hop <= ntaps, AETH_E_ARG, "hop %zu above the %zu taps", hop, ntaps);
    const double floor_ = 9.5367431640625e-07;       // 2^-20
    // the denominators first: nothing is written on a refusal
    for (size_t r = 0; r < hop && r < ntaps; r++) {
        double den = 0.0;
        for (size_t j = r; j < ntaps; j += hop) den += (double)w[j] * (double)w[j];
        AETH_REQUIRE(den >= floor_, AETH_E_ARG, "the squared window sums to %g over the hops at j = %zu: below 2^-20, no dual window", den, r);
    }
    for (size_t r = 0; r < hop; r++) {
        double den = 0.0;
        for (size_t j = r; j < ntaps; j += hop) den += (double)w[j] * (double)w[j];
        for (size_t j = r; j < ntaps; j += hop) out_host[j] = (float)((double)w[j] / den);
    }
    return AETH_OK;
}

}  // extern "C"
