// aeth_spec.hip -- averaged spectra: per-bin power sums and max hold over frames (include/aether_hip.h, aeth_vec_frame_sums,
// aeth_chan_exec_sums, aeth_vec_sum_levels; no body in the reference, whose `waterfall`, src/util/plot.rs:46-68, keeps every
// frame).  Welch's averaged periodogram and the max-hold trace of a spectrum analyser: one row of M numbers out of thousands
// of frames.
//
// The order of every f64 addition is part of the contract (the header): frames are cut into rows of `block`, rows into
// chunks of `chunk` frames; a chunk's frames are added in ascending order, then a row's chunk sums in ascending order.  So
//   frame_sums_kernel       a lane owns one column (8-byte loads) or two adjacent ones (16-byte loads: even len and a
//                           16-byte base) of ONE chunk and walks its frames with kLoads loads in flight, sum and max in
//                           registers.  A workgroup is min(256, columns) lanes along the columns, the rest along the chunks:
//                           one short-lived workgroup per (chunk group, column block).  The chunk partials go to a slab of
//                           the context -- or, when a row is one chunk, straight to the caller's planes.
//   frame_sums_fold_kernel  one lane per (row, column) adds the row's chunk partials in ascending order, out of batches that the
//                           workgroup's other lanes fetch ahead of it.
//   spec_fused_kernel       aeth_chan_exec_sums where a workgroup is one frame (power-of-two M = 512 .. 4096, P = 1, rot = 0):
//                           a workgroup takes one chunk; per frame it loads the window (the call's first frames from a small
//                           head buffer that holds the history, or zeros, in front of the first samples),
//                           multiplies by w, runs the register transform of aeth_fft_core.h (same Cfg, same per-lane twiddle
//                           table, same image-parity bookkeeping as fft_pow2_kernel / ofdm_fused_kernel), scales, takes
//                           level_q and accumulates per point in f64 registers; the next frame's window is in flight
//                           meanwhile.  It never grid-strides: the order must not see the grid.  8 bytes per input sample
//                           read (overlapping frames come from L1 / L2), the chunk partials written.
// No atomics anywhere, so the bytes depend on the frames, `block` and `chunk` only.
//
// Built with -ffp-contract=off: the window product is one rounded f32 product per component as in aeth_chan_fold, the
// transform's arithmetic is inline assembly and level_q carries its own pragma, so the fused route sees the bins of
// aeth_fft_exec bit for bit.
#include "aeth_internal.h"
#include "aeth_bank.h"
#include "aeth_fft_core.h"
#include "aeth_fft_plan.h"
#include "aeth_levels.h"

#include <cmath>

using namespace aeth::fftk;
using namespace aeth::bank;

namespace {

constexpr int kLoads = 8;                    // frames a lane of frame_sums_kernel has in flight
constexpr int PL_SUM = 1, PL_MAX = 2;        // planes a kernel keeps (bit mask)

// How the F frames of a call are cut.  Chunk g = r * K + c is chunk c of row r; the last row may have fewer chunks.
struct Cut {
    size_t F = 0, B = 0, C = 0;              // frames, frames per row (1 .. F), frames per chunk
    size_t R = 0, K = 0, G = 0;              // rows, chunks of a full row, chunks in all
};
Cut cut_of(size_t F, size_t block, size_t chunk)
{
    Cut c;
    c.F = F; c.B = block == 0 || block > F ? F : block; c.C = chunk;
    c.R = (F + c.B - 1) / c.B;
    c.K = (c.B - 1) / chunk + 1;
    const size_t last = F - (c.R - 1) * c.B;
    c.G = (c.R - 1) * c.K + (last - 1) / chunk + 1;
    return c;
}
__host__ __device__ inline size_t chunk_first(const Cut &c, size_t g) { const size_t r = g / c.K; return r * c.B + (g - r * c.K) * c.C; }
// one past the chunk's last frame
__host__ __device__ inline size_t chunk_end(const Cut &c, size_t g)
{
    const size_t r = g / c.K, m0 = r * c.B + (g - r * c.K) * c.C;
    size_t e = (r + 1) * c.B < c.F ? (r + 1) * c.B : c.F;
    if (m0 + c.C < e) e = m0 + c.C;
    return e;
}

__device__ __forceinline__ double max_rule(double best, double q) { return q > best ? q : best; }       // a NaN q never enters

struct SumsCall {
    const float2 *in;            // frame m_base of the call
    size_t m_base;
    Cut cut;
    size_t g0, g1;               // the chunks of this launch
    unsigned len;
    double *sum, *max;           // partials: [g * len + column]
    unsigned lx_log2, ncb;
    aeth::FastDiv fd_ncb;
};

template <int CW, int PL, bool NT> __global__ __launch_bounds__(kBlock) void frame_sums_kernel(SumsCall a)
{
    typedef typename Row<CW>::T V;
    const unsigned tg = aeth::fdiv(blockIdx.x, a.fd_ncb), cb = blockIdx.x - tg * a.ncb;
    const unsigned lx = threadIdx.x & ((1u << a.lx_log2) - 1u), ly = threadIdx.x >> a.lx_log2;
    const size_t col = (((size_t)cb << a.lx_log2) + lx) * CW;
    const size_t g = a.g0 + (size_t)tg * (kBlock >> a.lx_log2) + ly;
    if (col >= a.len || g >= a.g1) return;
    const size_t m0 = chunk_first(a.cut, g), m1 = chunk_end(a.cut, g);
    const float2 *p = a.in + col;
    const size_t len = a.len;

    double s[CW] = {}, b[CW] = {};
    auto take = [&](const V &v, bool first) {
        const float *f = reinterpret_cast<const float *>(&v);
#pragma unroll
        for (int c = 0; c < CW; c++) {
            const double q = aeth::level_q(f[2 * c], f[2 * c + 1]);
            if constexpr (PL & PL_SUM) s[c] = first ? q : s[c] + q;
            if constexpr (PL & PL_MAX) b[c] = max_rule(first ? -__builtin_inf() : b[c], q);
        }
    };
    take(aeth::nt_load<NT>(reinterpret_cast<const V *>(p + (m0 - a.m_base) * len)), true);
    for (size_t m = m0 + 1; m < m1; m += kLoads) {
        V v[kLoads];
#pragma unroll
        for (int j = 0; j < kLoads; j++) {
            const size_t mm = m + j < m1 ? m + j : m1 - 1;                  // past the chunk: a frame that exists, never taken
            v[j] = aeth::nt_load<NT>(reinterpret_cast<const V *>(p + (mm - a.m_base) * len));
        }
#pragma unroll
        for (int j = 0; j < kLoads; j++)
            if (m + j < m1) take(v[j], false);
    }
#pragma unroll
    for (int c = 0; c < CW; c++) {
        if constexpr (PL & PL_SUM) a.sum[g * len + col + c] = s[c];
        if constexpr (PL & PL_MAX) a.max[g * len + col + c] = b[c];
    }
}

// The row fold.  The additions of a column are a chain by definition, so what a launch can do in parallel is fetch: a
// workgroup owns kFoldCols columns of one row; lane (slot, column) has kFoldLoads partials of its column in flight, a batch
// of kFoldBatch consecutive chunks goes through LDS, and the column's lane of slot 0 (sum) or slot 1 (max) adds the batch in
// ascending order while the next batch is on its way.
constexpr int kFoldCols = 16, kFoldSlots = kBlock / kFoldCols, kFoldLoads = 8, kFoldBatch = kFoldSlots * kFoldLoads;

__global__ __launch_bounds__(kBlock) void frame_sums_fold_kernel(const double *__restrict__ psum, const double *__restrict__ pmax, Cut cut,
                                                                 unsigned len, unsigned ncb, double *__restrict__ sum, double *__restrict__ max)
{
    __shared__ double ls[kFoldBatch][kFoldCols], lm[kFoldBatch][kFoldCols];
    const size_t r = blockIdx.x / ncb;
    const unsigned cb = blockIdx.x - (unsigned)r * ncb;
    const unsigned cx = threadIdx.x % kFoldCols, sy = threadIdx.x / kFoldCols;
    const size_t col = (size_t)cb * kFoldCols + cx;
    const bool live = col < len;
    const size_t g0 = r * cut.K, g1 = g0 + cut.K < cut.G ? g0 + cut.K : cut.G;

    double vs[kFoldLoads], vm[kFoldLoads];
    auto fetch = [&](size_t gb) {
#pragma unroll
        for (int u = 0; u < kFoldLoads; u++) {
            const size_t g = gb + (size_t)u * kFoldSlots + sy;
            const bool ok = live && g < g1;
            vs[u] = ok && psum ? psum[g * len + col] : 0.0;
            vm[u] = ok && pmax ? pmax[g * len + col] : -__builtin_inf();
        }
    };
    fetch(g0);
    double s = 0.0, b = -__builtin_inf();
    for (size_t gb = g0; gb < g1; gb += kFoldBatch) {
        __syncthreads();                                     // the adders are done with the batch before
#pragma unroll
        for (int u = 0; u < kFoldLoads; u++) {
            ls[u * kFoldSlots + sy][cx] = vs[u];
            lm[u * kFoldSlots + sy][cx] = vm[u];
        }
        __syncthreads();
        fetch(gb + kFoldBatch);                              // past the row: nothing is loaded
        const int nb = g1 - gb < (size_t)kFoldBatch ? (int)(g1 - gb) : kFoldBatch;
        if (sy == 0 && psum) {
            int j = 0;
            if (gb == g0) { s = ls[0][cx]; j = 1; }          // the row's sum starts from chunk 0's sum
#pragma unroll 8
            for (; j < nb; j++) s = s + ls[j][cx];
        } else if (sy == 1 && pmax) {
#pragma unroll 8
            for (int j = 0; j < nb; j++) b = max_rule(b, lm[j][cx]);
        }
    }
    if (live && sy == 0 && psum) sum[r * len + col] = s;
    if (live && sy == 1 && pmax) max[r * len + col] = b;
}

// ---- the fused route ---------------------------------------------------------------------------------------------------
struct FusedCall {
    const cf *in;
    const cf *head;              // D < M: [M - D samples of history or zeros][in[0 .. min(n, M))], see spec_head_kernel
    const float *w;              // M taps
    const cf *twL;               // the inner plan's per-lane twiddle table
    Cut cut;
    unsigned D;
    float scale;
    int mirror;
    double *sum, *max;           // partials: [g * M + bin]
};

// Two waves per SIMD are what hides the exchanges of the transform, so 256 registers are the budget.  At 16 points per lane
// the transform (points, twiddles, butterfly temporaries) and both planes' accumulators (64 registers) leave no room for
// the next window: that variant loads each window when it needs it, every other one keeps the next window in flight.
// head[j] = s[j - H], H = M - D: the stream around the call's first sample in one piece, so that the frames that reach into
// the history are contiguous like every other frame
__global__ __launch_bounds__(kBlock) void spec_head_kernel(const cf *__restrict__ hist, const cf *__restrict__ in, unsigned H, unsigned cnt,
                                                           cf *__restrict__ head)
{
    const unsigned j = blockIdx.x * kBlock + threadIdx.x;
    if (j >= H + cnt) return;
    head[j] = j >= H ? in[j - H] : hist ? hist[j] : mk(0.f, 0.f);
}

template <class C, int PL> constexpr bool fused_prefetch() { return C::P < 16 || PL != (PL_SUM | PL_MAX); }

template <class C, int S, int PL, bool NT> __global__ __launch_bounds__(C::WG) void spec_fused_kernel(FusedCall a)
{
    constexpr bool PF = fused_prefetch<C, PL>();
    static_assert(C::F == 1 && C::IDLE == 0, "the workgroup is exactly one frame");
    constexpr int N = C::N, T = C::T, P = C::P;
    __shared__ cf lds[C::LDS_TOTAL];
    const int tid = threadIdx.x;
    const size_t g = blockIdx.x;
    const size_t m0 = chunk_first(a.cut, g), m1 = chunk_end(a.cut, g);
    const size_t D = a.D;

    // frame m covers s[(m + 1) * D - N + j]; slot k of a lane is j = tid + k * T.  The call's first frames, which reach in
    // front of in[0], read the head buffer instead: a choice of base pointer, the same in every lane
    auto fetch = [&](cf (&x)[P], size_t m) {
        const size_t e = (m + 1) * D;
        const cf *src = (e >= (size_t)N ? a.in + (e - N) : a.head + m * D) + tid;
#pragma unroll
        for (int k = 0; k < P; k++) x[k] = aeth::nt_load<NT>(src + k * T);
    };
    cf nx[P];
    if constexpr (PF) fetch(nx, m0);
    cf tw[C::TW];
    load_twiddles_lane<C>(tw, a.twL, tid);
    float wt[P];
#pragma unroll
    for (int k = 0; k < P; k++) wt[k] = a.w[tid + k * T];

    const cf ss = mk(a.scale, a.scale);
    double s[P] = {}, b[P] = {};
    bool par = false;
#pragma unroll 1
    for (size_t m = m0; m < m1; m++) {
        if constexpr (!PF) fetch(nx, m);
        cf x[P];
#pragma unroll
        for (int k = 0; k < P; k++) x[k] = mk(wt[k] * nx[k].x, wt[k] * nx[k].y);       // aeth_chan_fold at P = 1: one rounded product each
        if constexpr (PF) fetch(nx, m + 1 < m1 ? m + 1 : m);                           // the next window, in flight behind the transform
        // an odd number of exchanges per transform flips the image parity every frame
        if (fft_next_par<C>(0) == 0 || !par) fft_in_regs<C, S, 0>(x, tw, lds, tid);
        else fft_in_regs<C, S, 1>(x, tw, lds, tid);
        par = (fft_next_par<C>(0) != 0) && !par;
        const bool first = m == m0;
#pragma unroll
        for (int k = 0; k < P; k++) {
            const cf v = cscale_k(x[k], ss);
            const double q = aeth::level_q(v.x, v.y);
            if constexpr (PL & PL_SUM) s[k] = first ? q : s[k] + q;
            if constexpr (PL & PL_MAX) b[k] = max_rule(first ? -__builtin_inf() : b[k], q);
        }
    }
    // mirror: element e goes to e ^ N/2 (fft_pow2_kernel)
    const int msh = a.mirror ? (P / 2) * T : 0;
#pragma unroll
    for (int k = 0; k < P; k++) {
        const size_t o = g * N + tid + k * T + (k < P / 2 ? msh : -msh);
        if constexpr (PL & PL_SUM) a.sum[o] = s[k];
        if constexpr (PL & PL_MAX) a.max[o] = b[k];
    }
}

// ---- plane -> levels -----------------------------------------------------------------------------------------------------
template <int KIND> __global__ __launch_bounds__(kBlock) void sum_levels_kernel(const double *__restrict__ q, size_t n, double count, float *__restrict__ lv)
{
#pragma clang fp contract(off)
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const double qbar = q[i] / count;
    if constexpr (KIND == AETH_LEVEL_NORM) lv[i] = aeth::level_norm_of_q(qbar);
    else if constexpr (KIND == AETH_LEVEL_DB) lv[i] = (float)(10.0 * log10((double)aeth::level_norm_of_q(qbar)));
    else lv[i] = (float)(10.0 * log10(qbar));
}

// ---- host side -----------------------------------------------------------------------------------------------------------
typedef void (*SumsKernel)(SumsCall);
template <int CW, bool NT> SumsKernel sums_kernel(int planes)
{
    switch (planes) {
    case PL_SUM: return frame_sums_kernel<CW, PL_SUM, NT>;
    case PL_MAX: return frame_sums_kernel<CW, PL_MAX, NT>;
    default: return frame_sums_kernel<CW, PL_SUM | PL_MAX, NT>;
    }
}

// Where the chunk partials of a call go: the caller's planes when every row is one chunk, else the context's slab.
struct Partials {
    double *sum = nullptr, *max = nullptr;
    bool direct = false;
};
int partials_of(aeth_ctx *ctx, const Cut &c, size_t len, double *sum_dev, double *max_dev, Partials &p)
{
    p.direct = c.K == 1;
    if (p.direct) { p.sum = sum_dev; p.max = max_dev; return AETH_OK; }
    const size_t plane = c.G * len;
    int rc = aeth::scratch_ensure(ctx, ctx->spec_slab, 2 * plane * sizeof(double)); if (rc) return rc;
    double *slab = static_cast<double *>(ctx->spec_slab.p);
    p.sum = sum_dev ? slab : nullptr;
    p.max = max_dev ? slab + plane : nullptr;
    return AETH_OK;
}

// the chunk sums of chunks [g0, g1) out of frames that start at frame m_base of the call
int launch_chunks(aeth_ctx *ctx, const float2 *frames, size_t m_base, const Cut &c, size_t g0, size_t g1, size_t len, const Partials &p, bool nt)
{
    SumsCall a{};
    a.in = frames; a.m_base = m_base; a.cut = c; a.g0 = g0; a.g1 = g1; a.len = (unsigned)len;
    a.sum = p.sum; a.max = p.max;
    const bool wide = len % 2 == 0 && aeth::aligned16(frames);
    const RingShape r = ring_shape(wide ? len / 2 : len, g1 - g0);
    a.lx_log2 = r.lx_log2; a.ncb = r.ncb; a.fd_ncb = aeth::make_fastdiv(r.ncb);
    const int planes = (p.sum ? PL_SUM : 0) | (p.max ? PL_MAX : 0);
    const SumsKernel k = wide ? (nt ? sums_kernel<2, true>(planes) : sums_kernel<2, false>(planes))
                              : (nt ? sums_kernel<1, true>(planes) : sums_kernel<1, false>(planes));
    hipLaunchKernelGGL(k, dim3((unsigned)r.grid), dim3(kBlock), 0, aeth::ctx_stream(ctx), a);
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

int launch_row_fold(aeth_ctx *ctx, const Cut &c, size_t len, const Partials &p, double *sum_dev, double *max_dev)
{
    if (p.direct) return AETH_OK;
    const size_t ncb = (len + kFoldCols - 1) / kFoldCols;
    hipLaunchKernelGGL(frame_sums_fold_kernel, dim3((unsigned)(c.R * ncb)), dim3(kBlock), 0, aeth::ctx_stream(ctx), (const double *)p.sum,
                       (const double *)p.max, c, (unsigned)len, (unsigned)ncb, sum_dev, max_dev);
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

// what both reductions ask of their planes, behind the lengths; `in` / `hist`: what they must stay clear of
int check_planes(const void *in, size_t in_bytes, const void *hist, size_t hist_bytes, const double *sum_dev, const double *max_dev, size_t n_out)
{
    AETH_REQUIRE(aeth::aligned8(sum_dev) && aeth::aligned8(max_dev), AETH_E_ALIGN, "sum_dev %p or max_dev %p not 8-byte aligned",
                 (const void *)sum_dev, (const void *)max_dev);
    const size_t bytes = n_out * sizeof(double);
    AETH_REQUIRE(!aeth::ranges_touch(sum_dev, bytes, in, in_bytes) && !aeth::ranges_touch(max_dev, bytes, in, in_bytes) &&
                 !aeth::ranges_touch(sum_dev, bytes, hist, hist_bytes) && !aeth::ranges_touch(max_dev, bytes, hist, hist_bytes), AETH_E_ARG,
                 "sum_dev %p or max_dev %p overlaps the input (or its history)", (const void *)sum_dev, (const void *)max_dev);
    AETH_REQUIRE(!aeth::ranges_touch(sum_dev, bytes, max_dev, bytes), AETH_E_ARG, "sum_dev %p overlaps max_dev %p", (const void *)sum_dev,
                 (const void *)max_dev);
    return AETH_OK;
}

// workgroups of the chunk launch (one element per lane, at most) and of the row fold
int check_grids(const Cut &c, size_t len, size_t frames)
{
    AETH_REQUIRE(c.G <= SIZE_MAX / 32 / len, AETH_E_UNSUPPORTED, "%zu chunks of %zu columns overflow", c.G, len);
    AETH_REQUIRE(ring_shape(len, c.G).grid < ((size_t)1 << 31) && c.R * ((len + kFoldCols - 1) / kFoldCols) < ((size_t)1 << 31), AETH_E_UNSUPPORTED,
                 "%zu frames in one call: more than 2^31 workgroups", frames);
    return AETH_OK;
}

// ---- the filter bank's routes ----
bool fused_length(size_t M) { return M == 512 || M == 1024 || M == 2048 || M == 4096; }
bool fused_shape(const aeth_chan *c)
{
    return fused_length(c->M) && c->P == 1 && (c->phase == AETH_CHAN_PHASE_FRAME || c->D == c->M) && c->fft->algo == aeth::FFT_ALGO_POW2 &&
           c->fft->tw_lane_dev;
}
// frames per chunk: 16 Ki bins, 8 .. 32 frames -- a function of M alone.  A fused workgroup (one frame wide) walks one
// chunk, so the chunk is what sets the workgroups of a call: 2^25 samples make 2048 .. 4096 waves, two per SIMD and more.
// Smaller chunks cost slab traffic (16 bytes per bin and chunk), larger ones leave SIMDs with one wave (measured:
// profiles/spec_bw.txt).
size_t chunk_of(const aeth_chan *c)
{
    const size_t k = ((size_t)16 << 10) / c->M;
    return k < 8 ? 8 : k > 32 ? 32 : k;
}

// the general route's slice: the spectrum scratch holds at most this many bytes (whole chunks, one at least).  Measured at
// 2^25 samples (profiles/spec_bw.txt): 64 MiB is as fast as the whole call in one piece (which needs 2 x 8 F M bytes of
// scratch) and 1.6 .. 1.8 x faster than 16 MiB, whose launches are too short.  AETH_SPEC_SLICE_KIB (AETH_TUNING=1) moves it.
constexpr int kSliceKiB = 64 << 10;

template <class C, int S, bool NT> void launch_fused_planes(hipStream_t st, unsigned grid, const FusedCall &a)
{
    if (a.sum && a.max) hipLaunchKernelGGL((spec_fused_kernel<C, S, PL_SUM | PL_MAX, NT>), dim3(grid), dim3(C::WG), 0, st, a);
    else if (a.sum) hipLaunchKernelGGL((spec_fused_kernel<C, S, PL_SUM, NT>), dim3(grid), dim3(C::WG), 0, st, a);
    else hipLaunchKernelGGL((spec_fused_kernel<C, S, PL_MAX, NT>), dim3(grid), dim3(C::WG), 0, st, a);
}
template <class C> int launch_fused(aeth_ctx *ctx, const FusedCall &a, int sign, bool nt)
{
    hipStream_t st = aeth::ctx_stream(ctx);
    const unsigned grid = (unsigned)a.cut.G;
    if (sign > 0) { if (nt) launch_fused_planes<C, +1, true>(st, grid, a); else launch_fused_planes<C, +1, false>(st, grid, a); }
    else          { if (nt) launch_fused_planes<C, -1, true>(st, grid, a); else launch_fused_planes<C, -1, false>(st, grid, a); }
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

int run_fused(aeth_chan *c, const aeth_cf32 *hist, const aeth_cf32 *in, const Cut &cut, int sign, float scale, int mirror, const Partials &p)
{
    FusedCall a{};
    a.in = (const cf *)in;
    if (c->D < c->M) {
        const size_t H = c->M - c->D, n = cut.F * c->D, cnt = n < c->M ? n : c->M;
        int rc = ensure_elems(*c, H + cnt); if (rc) return rc;
        a.head = (const cf *)c->scratch.p;
        hipLaunchKernelGGL(spec_head_kernel, dim3((unsigned)((H + cnt + kBlock - 1) / kBlock)), dim3(kBlock), 0, aeth::ctx_stream(c->ctx),
                           (const cf *)hist, a.in, (unsigned)H, (unsigned)cnt, (cf *)c->scratch.p);
    }
    a.w = c->taps; a.twL = (const cf *)c->fft->tw_lane_dev;
    a.cut = cut; a.D = (unsigned)c->D; a.scale = scale; a.mirror = mirror;
    a.sum = p.sum; a.max = p.max;
    // overlapping frames are read again from the cache: only disjoint ones stream past it
    const bool nt = c->D == c->M && aeth::streams_past_cache(cut.F * c->M * sizeof(float2));
    switch (c->M) {
    case 512: return launch_fused<CfgFor<512>::type>(c->ctx, a, sign, nt);
    case 1024: return launch_fused<CfgFor<1024>::type>(c->ctx, a, sign, nt);
    case 2048: return launch_fused<CfgFor<2048>::type>(c->ctx, a, sign, nt);
    default: return launch_fused<CfgFor<4096>::type>(c->ctx, a, sign, nt);
    }
}

// fold -> transform -> (mirror) -> chunk sums, a slice of whole chunks at a time
int run_general(aeth_chan *c, const aeth_cf32 *hist, const aeth_cf32 *in, const Cut &cut, uint64_t first_frame, int sign, float scale,
                int mirror, const Partials &p)
{
    aeth_ctx *ctx = c->ctx;
    const size_t M = c->M, D = c->D, H = c->L - c->D;
    const size_t slice_bytes = (size_t)aeth::tuning_int("AETH_SPEC_SLICE_KIB", kSliceKiB) << 10;
    size_t per = slice_bytes / sizeof(float2) / M / cut.C;              // chunks of a slice
    if (per < 1) per = 1;
    if (per > cut.G) per = cut.G;
    const size_t fs = per * cut.C;                                      // frames of a slice, at most
    // [folded frames][spectrum][the history of a slice that starts inside the call's first L - D samples]
    const bool several = per < cut.G;
    int rc = ensure_elems(*c, 2 * fs * M + (several ? H : 0)); if (rc) return rc;
    float2 *folded = (float2 *)c->scratch.p, *spec = folded + fs * M, *hbuf = spec + fs * M;
    const bool stream = c->phase == AETH_CHAN_PHASE_STREAM && D < M;
    hipStream_t st = aeth::ctx_stream(ctx);
    for (size_t g0 = 0; g0 < cut.G; g0 += per) {
        const size_t g1 = g0 + per < cut.G ? g0 + per : cut.G;
        const size_t m0 = chunk_first(cut, g0), m1 = chunk_end(cut, g1 - 1), nf = m1 - m0;
        // the L - D samples in front of frame m0's hop: the caller's history, the input, or (rarely) some of both
        const aeth_cf32 *h = hist;
        if (m0 > 0 && H > 0) {
            if (m0 * D >= H) h = in + (m0 * D - H);
            else {
                const size_t have = m0 * D, want = H - have;            // `want` samples of history, then `have` of the input
                if (hist) AETH_HIP(hipMemcpyAsync(hbuf, hist + have, want * sizeof(float2), hipMemcpyDeviceToDevice, st));
                else AETH_HIP(hipMemsetAsync(hbuf, 0, want * sizeof(float2), st));
                AETH_HIP(hipMemcpyAsync(hbuf + want, in, have * sizeof(float2), hipMemcpyDeviceToDevice, st));
                h = (const aeth_cf32 *)hbuf;
            }
        }
        rc = chan_launch_fold(*c, stream, h, in + m0 * D, nf, first_frame % M + m0, folded); if (rc) return rc;
        rc = aeth::fft_run(c->fft, folded, spec, nf, sign, scale); if (rc) return rc;
        if (mirror) { rc = aeth_vec_mirror_frames(ctx, (aeth_cf32 *)spec, M, nf); if (rc) return rc; }
        rc = launch_chunks(ctx, spec, m0, cut, g0, g1, M, p, false); if (rc) return rc;
    }
    return AETH_OK;
}

}  // namespace

extern "C" {

int aeth_vec_frame_sums(aeth_ctx *ctx, const aeth_cf32 *frames_dev, size_t n, size_t len, size_t block, size_t chunk, double *sum_dev,
                        double *max_dev, size_t n_out)
{
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    AETH_REQUIRE(frames_dev, AETH_E_ARG, "frames is null");
    AETH_REQUIRE(sum_dev || max_dev, AETH_E_ARG, "both output planes are null");
    AETH_REQUIRE(n > 0 && len > 0, AETH_E_LEN, "%zu samples in frames of %zu: both at least 1", n, len);
    AETH_REQUIRE(n % len == 0, AETH_E_LEN, "%zu samples are not a multiple of the frame length %zu", n, len);
    AETH_REQUIRE(chunk > 0, AETH_E_LEN, "chunk of %zu frames: at least 1", chunk);
    AETH_REQUIRE(len < ((size_t)1 << 32) && n <= SIZE_MAX / 32, AETH_E_UNSUPPORTED, "%zu samples in frames of %zu", n, len);
    const Cut c = cut_of(n / len, block, chunk);
    AETH_REQUIRE(n_out == c.R * len, AETH_E_LEN, "output planes hold %zu values, %zu rows x %zu columns give %zu", n_out, c.R, len, c.R * len);
    AETH_REQUIRE(aeth::aligned8(frames_dev), AETH_E_ALIGN, "frames %p not 8-byte aligned", (const void *)frames_dev);
    int rc = check_planes(frames_dev, n * sizeof(aeth_cf32), nullptr, 0, sum_dev, max_dev, n_out); if (rc) return rc;
    rc = check_grids(c, len, c.F); if (rc) return rc;

    aeth::DeviceGuard dev_guard(ctx->device);
    Partials p;
    rc = partials_of(ctx, c, len, sum_dev, max_dev, p); if (rc) return rc;
    rc = launch_chunks(ctx, (const float2 *)frames_dev, 0, c, 0, c.G, len, p, aeth::streams_past_cache(n * sizeof(aeth_cf32))); if (rc) return rc;
    return launch_row_fold(ctx, c, len, p, sum_dev, max_dev);
}

size_t aeth_chan_sums_chunk(const aeth_chan *c) { return c ? chunk_of(c) : 0; }
int aeth_chan_sums_fused(const aeth_chan *c) { return c && fused_shape(c) ? 1 : 0; }

int aeth_chan_exec_sums(aeth_chan *c, const aeth_cf32 *hist, const aeth_cf32 *in, size_t n, uint64_t first_frame, int sign, int scale_kind,
                        float x, int mirror, size_t block, int flags, double *sum_dev, double *max_dev, size_t n_out)
{
    AETH_REQUIRE(c, AETH_E_ARG, "chan is null");
    AETH_REQUIRE((flags & ~AETH_SUMS_GENERAL) == 0, AETH_E_ARG, "unknown flags 0x%x", (unsigned)flags);
    AETH_REQUIRE(sum_dev || max_dev, AETH_E_ARG, "both output planes are null");
    AETH_REQUIRE(n > 0, AETH_E_LEN, "0 input samples: a call makes at least one frame of hop %zu", c->D);
    AETH_REQUIRE(n % c->D == 0, AETH_E_LEN, "%zu input samples are not a multiple of the hop %zu", n, c->D);
    const size_t F = n / c->D, M = c->M;
    AETH_REQUIRE(frames_fit(*c, F), AETH_E_LEN, "%zu frames x %zu channels overflow", F, M);
    const Cut cut = cut_of(F, block, chunk_of(c));
    AETH_REQUIRE(n_out == cut.R * M, AETH_E_LEN, "output planes hold %zu values, %zu rows x %zu channels give %zu", n_out, cut.R, M, cut.R * M);
    int rc = aeth::check_sign_scale(sign, scale_kind); if (rc) return rc;
    // (the planes stand in for check_buffers' output; their own checks follow)
    const void *out = sum_dev ? sum_dev : max_dev;
    rc = aeth::check_buffers(hist, c->L - c->D, in, n, out, n_out, sizeof(double), grid_bound(chan_ring(*c), M, ntiles_of(*c, F)), F, "frames");
    if (rc) return rc;
    rc = check_planes(in, n * sizeof(aeth_cf32), hist, (c->L - c->D) * sizeof(aeth_cf32), sum_dev, max_dev, n_out); if (rc) return rc;
    rc = check_grids(cut, M, F); if (rc) return rc;
    AETH_REQUIRE(cut.G < ((size_t)1 << 31), AETH_E_UNSUPPORTED, "%zu frames in one call: more than 2^31 workgroups", F);

    aeth::DeviceGuard dev_guard(c->ctx->device);
    const float s = aeth_scale_factor(scale_kind, M, x);
    Partials p;
    rc = partials_of(c->ctx, cut, M, sum_dev, max_dev, p); if (rc) return rc;
    if (!(flags & AETH_SUMS_GENERAL) && fused_shape(c)) rc = run_fused(c, hist, in, cut, sign, s, mirror ? 1 : 0, p);
    else rc = run_general(c, hist, in, cut, first_frame, sign, s, mirror ? 1 : 0, p);
    if (rc) return rc;
    return launch_row_fold(c->ctx, cut, M, p, sum_dev, max_dev);
}

int aeth_vec_sum_levels(aeth_ctx *ctx, const double *q_dev, size_t n, double count, int level_kind, float *levels_dev)
{
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    AETH_REQUIRE(aeth::level_kind_ok(level_kind), AETH_E_ARG, "bad level kind %d", level_kind);
    AETH_REQUIRE(count > 0.0 && count <= 1.7976931348623157e308, AETH_E_ARG, "count %g is not a finite number above 0", count);
    if (n == 0) return AETH_OK;
    AETH_REQUIRE(q_dev && levels_dev, AETH_E_ARG, "null pointer");
    AETH_REQUIRE(aeth::aligned8(q_dev), AETH_E_ALIGN, "q_dev %p not 8-byte aligned", (const void *)q_dev);
    AETH_REQUIRE(aeth::aligned4(levels_dev), AETH_E_ALIGN, "levels_dev %p not 4-byte aligned", (const void *)levels_dev);
    AETH_REQUIRE(!aeth::ranges_touch(q_dev, n * sizeof(double), levels_dev, n * sizeof(float)), AETH_E_ARG, "levels_dev %p overlaps q_dev %p",
                 (const void *)levels_dev, (const void *)q_dev);
    const size_t blocks = (n + kBlock - 1) / kBlock;
    AETH_REQUIRE(blocks < ((size_t)1 << 31), AETH_E_UNSUPPORTED, "%zu values", n);
    aeth::DeviceGuard dev_guard(ctx->device);
    hipStream_t st = aeth::ctx_stream(ctx);
    switch (level_kind) {
    case AETH_LEVEL_NORM: hipLaunchKernelGGL(sum_levels_kernel<AETH_LEVEL_NORM>, dim3((unsigned)blocks), dim3(kBlock), 0, st, q_dev, n, count, levels_dev); break;
    case AETH_LEVEL_DB: hipLaunchKernelGGL(sum_levels_kernel<AETH_LEVEL_DB>, dim3((unsigned)blocks), dim3(kBlock), 0, st, q_dev, n, count, levels_dev); break;
    default: hipLaunchKernelGGL(sum_levels_kernel<AETH_LEVEL_POWER_DB>, dim3((unsigned)blocks), dim3(kBlock), 0, st, q_dev, n, count, levels_dev); break;
    }
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

}  // extern "C"
