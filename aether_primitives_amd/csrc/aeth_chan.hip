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
#include "aeth_bank.h"
#include "aeth_fft_plan.h"
#include "aeth_levels.h"

#include <cmath>

namespace {

using namespace aeth::bank;

constexpr unsigned kRingMaxP = 8;            // the register ring: P rows + P rows in flight + P taps per column

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

}  // namespace

bool aeth::bank::chan_ring(const Bank &b) { return b.D == b.M && b.P <= kRingMaxP; }
size_t aeth::bank::chan_tile(const Bank &b) { return chan_ring(b) ? ring_tile(b.P) : gen_tile(b.M); }

namespace {

// what every exec call checks before any device work; out_elem_bytes: size of the caller's output range
int check_call(const aeth_chan *c, const aeth_cf32 *hist, const aeth_cf32 *in, size_t n, const void *out, size_t n_out,
               size_t out_elem_bytes, size_t *nframes)
{
    AETH_REQUIRE(c, AETH_E_ARG, "chan is null");
    AETH_REQUIRE(n > 0, AETH_E_LEN, "0 input samples: a call makes at least one frame of hop %zu", c->D);
    AETH_REQUIRE(n % c->D == 0, AETH_E_LEN, "%zu input samples are not a multiple of the hop %zu", n, c->D);
    const size_t F = n / c->D;
    AETH_REQUIRE(frames_fit(*c, F) && n_out == F * c->M, AETH_E_LEN, "output holds %zu elements, %zu frames x %zu channels give %zu",
                 n_out, F, c->M, frames_fit(*c, F) ? F * c->M : (size_t)0);
    *nframes = F;
    return aeth::check_buffers(hist, c->L - c->D, in, n, out, n_out, out_elem_bytes, grid_bound(chan_ring(*c), c->M, ntiles_of(*c, F)), F, "frames");
}

}  // namespace

int aeth::bank::chan_launch_fold(const Bank &b, bool stream, const aeth_cf32 *hist, const aeth_cf32 *in, size_t F, uint64_t first_frame,
                                 float2 *out)
{
    ChanCall a{};
    a.in = (const float2 *)in;
    a.hist = b.L > b.D ? (const float2 *)hist : nullptr;
    a.out = out;
    a.w = b.taps;
    a.nframes = F;
    a.M = (unsigned)b.M; a.D = (unsigned)b.D; a.P = (unsigned)b.P;
    a.tile = (unsigned)b.tile;
    a.fd_M = aeth::make_fastdiv(a.M);
    a.stream = stream;
    a.g1 = (unsigned)((first_frame % b.M + 1) % b.M);
    const size_t ntiles = ntiles_of(b, F);
    const bool nt = aeth::streams_past_cache((F * b.M + F * b.D) * sizeof(float2));
    if (!chan_ring(b)) {
        a.ncb = (unsigned)gen_ncb(b.M);
        return launch(b, nt ? chan_gen_kernel<true> : chan_gen_kernel<false>, ntiles * a.ncb, a);
    }
    const bool wide = b.M % 2 == 0 && aeth::aligned16(in) && aeth::aligned16(out) && aeth::aligned16(a.hist);
    const RingShape r = ring_shape(wide ? b.M / 2 : b.M, ntiles);       // lanes along the columns
    a.lx_log2 = r.lx_log2; a.ncb = r.ncb;
    return launch(b, wide ? (nt ? ring_kernel<2, true>(a.P) : ring_kernel<2, false>(a.P)) : (nt ? ring_kernel<1, true>(a.P) : ring_kernel<1, false>(a.P)),
                  r.grid, a);
}

namespace {

int fold(const aeth_chan *c, const aeth_cf32 *hist, const aeth_cf32 *in, size_t F, uint64_t first_frame, float2 *out)
{
    return chan_launch_fold(*c, c->phase == AETH_CHAN_PHASE_STREAM && c->D < c->M, hist, in, F, first_frame, out);
}

// fold into the scratch, for the plan to read: `elems` folded samples
int fold_to_scratch(aeth_chan *c, const aeth_cf32 *hist, const aeth_cf32 *in, size_t F, uint64_t first_frame, size_t elems)
{
    int rc = ensure_elems(*c, elems); if (rc) return rc;
    return fold(c, hist, in, F, first_frame, (float2 *)c->scratch.p);
}

}  // namespace

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
    int rc = create_checks(out, ctx, proto_host, ntaps, channels, hop, phase); if (rc) return rc;
    aeth_chan *c = nullptr;
    rc = create_planned(ctx, ntaps, channels, hop, phase, max_frames, &c); if (rc) return rc;
    c->tile = chan_tile(*c);
    return create_finish(c, proto_host, frames_fit(*c, max_frames) ? max_frames * channels : 0, "aeth_chan_create: prototype upload", out);
}

int aeth_chan_destroy(aeth_chan *c) { return destroy(c); }

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
    return fold(c, hist, in, F, first_frame, (float2 *)out);
}

int aeth_chan_exec(aeth_chan *c, const aeth_cf32 *hist, const aeth_cf32 *in, size_t n, uint64_t first_frame, int sign,
                   int scale_kind, float x, aeth_cf32 *out, size_t n_out)
{
    size_t F = 0;
    int rc = check_call(c, hist, in, n, out, n_out, sizeof(aeth_cf32), &F); if (rc) return rc;
    rc = aeth::check_sign_scale(sign, scale_kind); if (rc) return rc;
    rc = fold_to_scratch(c, hist, in, F, first_frame, n_out); if (rc) return rc;
    return aeth_fft_exec(c->fft, (const aeth_cf32 *)c->scratch.p, n_out, out, F, sign, scale_kind, x);
}

int aeth_chan_exec_levels(aeth_chan *c, const aeth_cf32 *hist, const aeth_cf32 *in, size_t n, uint64_t first_frame, int sign,
                          int scale_kind, float x, int mirror, int level_kind, float *levels, size_t n_levels)
{
    size_t F = 0;
    int rc = check_call(c, hist, in, n, levels, n_levels, sizeof(float), &F); if (rc) return rc;
    rc = aeth::check_sign_scale(sign, scale_kind); if (rc) return rc;
    AETH_REQUIRE(aeth::level_kind_ok(level_kind), AETH_E_ARG, "bad level kind %d", level_kind);
    rc = fold_to_scratch(c, hist, in, F, first_frame, n_levels); if (rc) return rc;
    return aeth_fft_exec_levels(c->fft, (const aeth_cf32 *)c->scratch.p, n_levels, F, sign, scale_kind, x, mirror, level_kind, levels,
                                n_levels);
}

}  // extern "C"
