// aeth_synth.hip -- polyphase synthesis filter bank: weighted overlap-add behind the batched inverse FFT, the transpose
// of aeth_chan.hip (the reference has no synthesis: src/util/plot.rs:46-68 only takes a stream apart).
// Frame m (M samples) is extended periodically to L = P * M, weighted by the real prototype g and added into the output
// at m * D: out[i] = sum over m ascending with 0 <= i - m D < L of g[j] * v_m[(j + rot_m) mod M], j = i - m D (every
// product and every sum rounded: EXACT flags).  K = ceil(L / D) frames touch one output.  Three routes:
//   fold     D == M: the sum is aeth_chan_fold of the row-reversed prototype; no kernel here (aeth_bank.h: chan_launch_fold).
//   ring     D < M, D divides L, K <= 8: a lane owns output offset d of every hop (8-byte accesses) or d and d + 1
//            (16-byte accesses), keeps the K - 1 open accumulators in registers and walks a tile of frames oldest
//            first: frame m gives g[k D + d] * v_m[..] to the accumulator of hop m + k, the first contribution assigns,
//            hop m is then complete and stored.  K - 1 halo frames per tile.
//   general  everything else: a lane owns output i and gathers its (at most K) terms in ascending m; absent terms are
//            skipped, never added as zeros; the P-fold re-read of a frame is served by L2.
#include "aeth_internal.h"
#include "aeth_bank.h"
#include "aeth_fft_plan.h"

#include <memory>

namespace {

using namespace aeth::bank;

constexpr unsigned kMaxK = 256;
constexpr unsigned kRingMaxK = 8;            // the register ring: K - 1 accumulators + K taps + K offsets per lane
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

enum { ROUTE_FOLD = 0, ROUTE_RING = 1, ROUTE_GEN = 2 };

}  // namespace

struct aeth_synth : Bank {
    size_t K = 0;                // frames that overlap in one output sample: ceil(L / D)
    int kind = ROUTE_GEN;
};

namespace {

// what unfold and exec check before any device work
int check_call(const aeth_synth *s, const aeth_cf32 *hist, const aeth_cf32 *in, size_t n, const aeth_cf32 *out, size_t n_out,
               size_t *nframes)
{
    AETH_REQUIRE(s, AETH_E_ARG, "synth is null");
    AETH_REQUIRE(n > 0, AETH_E_LEN, "0 input samples: a call takes at least one frame of %zu channels", s->M);
    AETH_REQUIRE(n % s->M == 0, AETH_E_LEN, "%zu input samples are not a multiple of the %zu channels", n, s->M);
    const size_t F = n / s->M;
    AETH_REQUIRE(frames_fit(*s, F, s->K) && n_out == F * s->D, AETH_E_LEN, "output holds %zu elements, %zu frames x hop %zu give %zu",
                 n_out, F, s->D, frames_fit(*s, F, s->K) ? F * s->D : (size_t)0);
    *nframes = F;
    // the fold route runs the analysis bank's kernels over the M columns, the others run along the D offsets of a hop
    const size_t grid = s->kind == ROUTE_FOLD ? grid_bound(chan_ring(*s), s->M, ntiles_of(*s, F))
                                              : grid_bound(s->kind == ROUTE_RING, s->D, ntiles_of(*s, F));
    return aeth::check_buffers(hist, (s->K - 1) * s->M, in, n, out, n_out, sizeof(aeth_cf32), grid, F, "frames");
}

int launch_unfold(aeth_synth *s, const aeth_cf32 *hist, const aeth_cf32 *in, size_t F, uint64_t first_frame, float2 *out)
{
    // D == M: rot is identically 0, the fold frames by AETH_CHAN_PHASE_FRAME whatever the phase of this bank
    if (s->kind == ROUTE_FOLD) return chan_launch_fold(*s, false, hist, in, F, first_frame, out);
    SynthCall a{};
    a.in = (const float2 *)in;
    a.hist = (const float2 *)hist;               // K >= 2 on both routes
    a.out = out;
    a.g = s->taps;
    a.nframes = F;
    a.M = (unsigned)s->M; a.D = (unsigned)s->D; a.K = (unsigned)s->K; a.L = (unsigned)s->L;
    a.tile = (unsigned)s->tile;
    a.fd_M = aeth::make_fastdiv(a.M);
    a.fd_D = aeth::make_fastdiv(a.D);
    a.stream = s->phase == AETH_CHAN_PHASE_STREAM;
    a.g1 = (unsigned)((first_frame % s->M + 1) % s->M);
    const size_t ntiles = ntiles_of(*s, F);
    const bool nt = aeth::streams_past_cache((F * s->M + F * s->D) * sizeof(float2));
    if (s->kind == ROUTE_GEN) {
        a.ncb = (unsigned)gen_ncb(s->D);
        return launch(*s, nt ? synth_gen_kernel<true> : synth_gen_kernel<false>, ntiles * a.ncb, a);
    }
    // pairs need even offsets at even positions of 16-byte aligned rows: D and M even (rot is then even too)
    const bool wide = s->D % 2 == 0 && s->M % 2 == 0 && aeth::aligned16(in) && aeth::aligned16(out) && aeth::aligned16(hist);
    const RingShape r = ring_shape(wide ? s->D / 2 : s->D, ntiles);       // lanes along the offsets
    a.lx_log2 = r.lx_log2; a.ncb = r.ncb;
    return launch(*s, wide ? (nt ? ring_kernel<2, true>(a.K) : ring_kernel<2, false>(a.K)) : (nt ? ring_kernel<1, true>(a.K) : ring_kernel<1, false>(a.K)),
                  r.grid, a);
}

}  // namespace

extern "C" {

int aeth_synth_create(aeth_ctx *ctx, const float *proto_host, size_t ntaps, size_t channels, size_t hop, int phase,
                      size_t max_frames, aeth_synth **out)
{
    int rc = create_checks(out, ctx, proto_host, ntaps, channels, hop, phase); if (rc) return rc;
    const size_t K = (ntaps + hop - 1) / hop;
    AETH_REQUIRE(K <= kMaxK, AETH_E_UNSUPPORTED, "%zu taps at hop %zu: %zu frames overlap in one output sample, at most %u", ntaps, hop, K,
                 kMaxK);
    aeth_synth *s = nullptr;
    rc = create_planned(ctx, ntaps, channels, hop, phase, max_frames, &s); if (rc) return rc;
    s->K = K;
    std::unique_ptr<float[]> rev;                // the fold route's prototype
    if (hop == channels) {
        // out row n = sum over p ascending of g[(P - 1 - p) M + q] * row_{n - P + 1 + p}[q]: the fold of the reversed rows
        s->kind = ROUTE_FOLD;
        s->tile = chan_tile(*s);
        rev.reset(new (std::nothrow) float[ntaps]);
        if (!rev) { (void)destroy(s); return aeth::set_error(AETH_E_NOMEM, "out of host memory"); }
        for (size_t p = 0; p < s->P; p++)
            for (size_t q = 0; q < channels; q++) rev[p * channels + q] = proto_host[(s->P - 1 - p) * channels + q];
    } else if (ntaps % hop == 0 && K <= kRingMaxK) {
        s->kind = ROUTE_RING;
        s->tile = ring_tile(K);
    } else {
        s->kind = ROUTE_GEN;
        s->tile = gen_tile(hop);
    }
    return create_finish(s, rev ? rev.get() : proto_host, max_frames > 0 && frames_fit(*s, max_frames, K) ? (K - 1 + max_frames) * channels : 0,
                         "aeth_synth_create: prototype upload", out);
}

int aeth_synth_destroy(aeth_synth *s) { return destroy(s); }

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
    rc = aeth::check_sign_scale(sign, scale_kind); if (rc) return rc;
    const size_t nh = (s->K - 1) * s->M;
    rc = ensure_elems(*s, nh + n_in); if (rc) return rc;
    aeth_cf32 *th = (aeth_cf32 *)s->scratch.p, *tf = th + nh;
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
