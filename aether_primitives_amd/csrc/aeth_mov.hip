// aeth_mov.hip -- moving-window detectors over a device-resident stream (no body in the reference; definition in
// include/aether_hip.h, aeth_mov_*): for every sample the sum of the last W lag terms x[j] * conj(x[j - L]) and of the
// last W powers |x[j]|^2, the timing metric |P|^2 / (R(i) R(i - L)) of Schmidl and Cox (or the moving mean power), and
// the peak search over it.  An overlapping-window sum, not a reduction onto a grid: van Herk's scheme, every window sum
// adds its own W terms and nothing else, in f64, no floating-point atomics.  Compiled with -ffp-contract=off: the
// metric's products are NOT exact and are defined one rounding per operation.
//
// THE ORDER (a function of W and of the output's index in the call only).  The terms are cut into segments [s W, (s + 1) W)
// counted from the call's index 0 (history: s < 0).  Term j has position k = j - s W in its segment and lies in cell
// c = k / 32; a segment has cps = ceil(W / 32) cells, the last one short when 32 does not divide W.
//   a(k) = the cell's terms from its first through k, added in ascending order from -0.0
//   d(k) = the cell's terms from its last down to k, added in descending order from -0.0
//   T_c  = a(last k of cell c)
//   v    = the log-step scan of T_0 .. T_{cps - 1}: for s = 1, 2, 4, ... < cps:  v[c] = v[c - s] + v[c] for c >= s
//   u    = the same scan of the totals in reverse order, T_{cps - 1} .. T_0
//   h(k) = a(k) for c == 0, else v[c - 1] + a(k)                   (the segment's terms 0 .. k)
//   g(k) = d(k) for c == cps - 1, else u[cps - 2 - c] + d(k)       (the segment's terms k .. W - 1)
//   S(i) = h(W - 1) when i mod W == W - 1 (the window IS a segment), else g(k + 1) of the segment in front + h(k), k = i mod W.
// Sums start from -0.0, so W = 1 hands out each term itself.  A cut at a multiple of W (aeth_mov_grid) keeps the segments
// where they were.
//
// THE KERNEL.  One workgroup of 256 lanes per chunk of 1024 outputs (chunks are counted inside a search block; nothing
// above depends on them).  The chunk needs the terms of indices g - W + 1 .. g + left - 1: at most 5119 of them, in at
// most 163 cells when a segment has more than one.  R(i - L) is summed first, on the grid of the indices i - L (it is R
// at another index, not a fourth quantity of index i), then P and R(i).  For each of the two, a lane owns a cell:
//   1. (cps > 1) the cell totals T into LDS, then the two log-step scans, all cells at once;
//   2. d(k) descending, + u: g of every position a window of the chunk ends its front part on, into LDS (four f64 planes
//      of 1024 slots, one slot of padding per 32: a lane's slots are 32 apart and would share one bank otherwise);
//   3. a(k) ascending, + v: h of every output of the chunk, + the g of step 2: the window sums, the metric, and either
//      the planes (staged in the slots just read, then stored 256 consecutive outputs at a time) or the lane's best
//      candidate, which THE TREE of aeth_reduce.h turns into the chunk's record (the folds behind it: the same file).
// Windows up to 1024 samples first copy the chunk's samples and their lag partners into LDS, 256 consecutive samples per
// load instruction, and the passes read those; longer windows read memory in every pass, 32 consecutive samples per lane (a
// line of the vector cache per lane): slow, and measured as such.  Samples in front of the call come
// from the history (or are zeros) by a select on the address.
#include "aeth_internal.h"
#include "aeth_reduce.h"

#include <cmath>

namespace {

using aeth::FastDiv;
using aeth::red::Cut;

typedef aeth_mov_peak Peak;
static_assert(sizeof(Peak) == 64, "record layout");

constexpr int kBlock = aeth::red::kBlock;
constexpr unsigned kChunk = 1024;                                    // outputs per workgroup
constexpr int kCell = 32;                                            // terms a lane adds in order
constexpr size_t kMaxWindow = 4096;
constexpr size_t kMaxLag = 65536;
constexpr int kCells = 168;                                          // cells of one chunk when a segment has several
constexpr int kSlots = kChunk + kChunk / 32;
constexpr int kStageWindow = 1024;                                   // windows up to this stage their samples in LDS
constexpr int kStage = kChunk + kStageWindow - 1 + (kChunk + kStageWindow - 1) / 32 + 1;

enum { OUT_P = 1, OUT_R = 2, OUT_M = 4, OUT_SEARCH = 8 };

// cells a chunk's terms can lie in, W > 32: the span in whole cells, one more where it starts inside a cell, one more per
// segment it touches (a segment's last cell may be short)
constexpr bool cells_fit()
{
    for (unsigned w = kCell + 1; w <= kMaxWindow; w++) {
        const unsigned span = kChunk + w - 1, segs = (span - 1) / w + 2;
        if (span / kCell + segs + 1 > (unsigned)kCells) return false;
    }
    return true;
}
static_assert(cells_fit(), "kCells");

template <int KIND> constexpr int nq() { return KIND == AETH_MOV_LAG ? 4 : 1; }   // LDS planes: c.re, c.im, q(x_j), R(i - L)  |  q(x_j)

struct Cand;

struct Args {
    const float2 *x, *hist;
    size_t n, block;
    FastDiv cpb;
    int window;
    unsigned lag;
    double r_min, threshold;
    float2 *p;
    float *r, *m;
    Cand *rec;
    int direct;
};

// the terms a pass needs, by their index relative to `g`; outside [rlo, rhi] nobody needs them: zeros, no load.  Q == 3:
// the lag terms c.re, c.im and q(x_j) of index g + r; Q == 1: q(x_j) alone
template <bool NT> struct Terms {
    const float2 *x, *hist;
    long long g, H, L;
    int rlo, rhi;
    const float2 *sa, *sb;                                           // LDS copies of x[g + r] and x[g - L + r], r = rlo .. rhi, or null
    __device__ __forceinline__ float2 sample(long long j, bool in) const
    {
        const bool front = j < 0;
        const float2 *q = front ? (hist ? hist + (H + j) : x) : x + j;
        float2 v = aeth::nt_load<NT>(q);
        if (!in || (front && !hist)) v = make_float2(0.0f, 0.0f);
        return v;
    }
    template <int Q> __device__ __forceinline__ void get(int r, double (&t)[Q]) const
    {
        static_assert(Q == 1 || Q == 3, "terms");
        const bool in = r >= rlo && r <= rhi;
        float2 a, b = make_float2(0.0f, 0.0f);
        if (sa) {                                                    // wave-uniform
            const int at = in ? r - rlo : 0, s = at + (at >> 5);
            a = sa[s];
            if constexpr (Q == 3) b = sb[s];
            if (!in) { a = make_float2(0.0f, 0.0f); b = a; }
        } else {
            const long long j = g + (in ? r : rhi);                  // g + rhi is the last index summed: always there
            a = sample(j, in);
            if constexpr (Q == 3) b = sample(j - L, in);
        }
        const double ar = (double)a.x, ai = (double)a.y;             // products of two f32 values: exact, one rounding each line
        if constexpr (Q == 3) {
            const double br = (double)b.x, bi = (double)b.y;
            t[0] = ar * br + ai * bi;
            t[1] = ai * br - ar * bi;
            t[2] = ar * ar + ai * ai;
        } else {
            t[0] = ar * ar + ai * ai;
        }
    }
};

__device__ __forceinline__ int slot(int r) { return r + (r >> 5); }

// ---- records --------------------------------------------------------------------------------------------------------
// aeth_mov_peak as the kernels hold it: eight 8-byte fields (metric in the low half of `mn`, n_nan in the high half), so
// that a record stays in registers
struct Cand { unsigned long long index, first; double p_re, p_im, r, r_lag; unsigned long long mn, reserved; };
static_assert(sizeof(Cand) == sizeof(Peak), "record layout");
__device__ __forceinline__ float cand_metric(const Cand &c) { return __uint_as_float((unsigned)c.mn); }
__device__ __forceinline__ unsigned long long cand_pack(float metric, unsigned n_nan)
{
    return (unsigned long long)__float_as_uint(metric) | ((unsigned long long)n_nan << 32);
}
__device__ __forceinline__ Cand cand_none(size_t n)
{
    Cand p;
    p.index = n; p.first = n; p.p_re = 0.0; p.p_im = 0.0; p.r = 0.0; p.r_lag = 0.0;
    p.mn = cand_pack(__builtin_nanf(""), 0); p.reserved = 0;
    return p;
}
// the better candidate wins (larger metric, then lower index: a total order, so any tree gives the same record); the
// first crossing is the lower one, the NaN counts add and saturate
__device__ __forceinline__ Cand cand_combine(const Cand &a, const Cand &b, size_t n)
{
    const bool ha = a.index != n, hb = b.index != n;
    const float ma = cand_metric(a), mb = cand_metric(b);
    const bool take_a = ha && (!hb || ma > mb || (ma == mb && a.index < b.index));
    Cand o;
    o.index = take_a ? a.index : b.index;
    o.p_re = take_a ? a.p_re : b.p_re; o.p_im = take_a ? a.p_im : b.p_im;
    o.r = take_a ? a.r : b.r; o.r_lag = take_a ? a.r_lag : b.r_lag;
    o.first = a.first < b.first ? a.first : b.first;
    const unsigned long long nn = (a.mn >> 32) + (b.mn >> 32);
    o.mn = cand_pack(take_a ? ma : mb, nn > 0xffffffffull ? 0xffffffffu : (unsigned)nn);
    o.reserved = 0;
    return o;
}
// ---- the chunk kernel -----------------------------------------------------------------------------------------------
__device__ __forceinline__ long long floor_div(long long a, int w) { return a >= 0 ? a / w : -((-a + w - 1) / w); }

// The window sums S(g + o), o = 0 .. left - 1, of Q quantities whose terms `terms` hands out, on the segment grid of the
// indices g + o (g may be negative: R(i - L) is R at the index i - L, on ITS grid).  G: Q planes of kSlots slots, EP, ES: Q
// planes of kCells; `out(o, S)` is called by the lane that owns output o's cell, o ascending inside a lane.  Wave-uniform
// control flow up to the loops over cells; every lane passes every barrier.
template <int Q, class T, class F>
__device__ __forceinline__ void window_sums(long long g, int left, int W, const T &terms, double (*G)[kSlots], double (*EP)[kCells],
                                            double (*ES)[kCells], F out)
{
    const int tid = (int)threadIdx.x;
    // the segment grid under the terms base .. g + left - 1
    const long long base = g - (W - 1);
    const long long s0 = floor_div(base, W);                         // the segment of the first term
    const int rel0 = (int)(s0 * W - g);                              // its first index relative to g: in (-2 W, 0]
    const int cps = (W + kCell - 1) / kCell;
    const int cell0 = (int)(base - s0 * W) / kCell;                  // cells of that segment in front of the first term's
    const long long imax = g + left - 1, sm = floor_div(imax, W);
    const int ncell = (int)(sm - s0) * cps + (int)(imax - sm * W) / kCell - cell0 + 1;
    // flat cell e -> its cell number in the segment, its first index relative to g, its length
    auto cell_of = [&](int e, int &c, int &rel, int &len) {
        const int ee = e + cell0, seg = ee / cps;
        c = ee - seg * cps;
        rel = rel0 + seg * W + c * kCell;
        len = W - c * kCell < kCell ? W - c * kCell : kCell;
    };

    // 1. cell totals and their two scans (one cell per lane: ncell <= kCells)
    if (cps > 1) {
        int c = 0, rel = 0, len = 0;
        const bool mine = tid < ncell;
        if (mine) {
            cell_of(tid, c, rel, len);
            double T_[Q];
#pragma unroll
            for (int q = 0; q < Q; q++) T_[q] = -0.0;
#pragma unroll 4
            for (int k = 0; k < len; k++) {
                double t[Q];
                terms.template get<Q>(rel + k, t);
#pragma unroll
                for (int q = 0; q < Q; q++) T_[q] += t[q];
            }
#pragma unroll
            for (int q = 0; q < Q; q++) { EP[q][tid] = T_[q]; ES[q][tid] = T_[q]; }
        }
        __syncthreads();
        for (int s = 1; s < cps; s <<= 1) {
            // a partner outside the chunk's cells belongs to a scan nobody reads (a segment that begins in front of the
            // first term has no output here; one that ends behind the last has no window's front part)
            const bool dp = mine && c >= s && tid >= s, ds = mine && c + s < cps && tid + s < ncell;
            double vp[Q], vs[Q];
#pragma unroll
            for (int q = 0; q < Q; q++) {
                vp[q] = dp ? EP[q][tid - s] + EP[q][tid] : 0.0;
                vs[q] = ds ? ES[q][tid + s] + ES[q][tid] : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < Q; q++) {
                if (dp) EP[q][tid] = vp[q];
                if (ds) ES[q][tid] = vs[q];
            }
            __syncthreads();
        }
    }

    // 2. g(k) of the positions r + (W - 1) in 0 .. left - 1 (slot = the output whose window begins there)
    for (int e = tid; e < ncell; e += kBlock) {
        int c, rel, len;
        cell_of(e, c, rel, len);
        if (rel + len - 1 + (W - 1) < 0 || rel + (W - 1) >= left) continue;
        const bool last = c == cps - 1;
        double u[Q], acc[Q];
#pragma unroll
        for (int q = 0; q < Q; q++) { u[q] = (!last && e + 1 < ncell) ? ES[q][e + 1] : 0.0; acc[q] = -0.0; }
#pragma unroll 4
        for (int k = len - 1; k >= 0; k--) {
            double t[Q];
            terms.template get<Q>(rel + k, t);
            const int o = rel + k + (W - 1);
#pragma unroll
            for (int q = 0; q < Q; q++) {
                acc[q] += t[q];
                if (o >= 0 && o < left) G[q][slot(o)] = last ? acc[q] : u[q] + acc[q];
            }
        }
    }
    __syncthreads();

    // 3. h(k) of the outputs and the window sums
    for (int e = tid; e < ncell; e += kBlock) {
        int c, rel, len;
        cell_of(e, c, rel, len);
        if (rel + len - 1 < 0) continue;                             // rel < left by the choice of ncell
        double v[Q], acc[Q];
#pragma unroll
        for (int q = 0; q < Q; q++) { v[q] = (c > 0 && e > 0) ? EP[q][e - 1] : 0.0; acc[q] = -0.0; }
#pragma unroll 2
        for (int k = 0; k < len; k++) {
            double t[Q];
            const int o = rel + k;
            terms.template get<Q>(o, t);
#pragma unroll
            for (int q = 0; q < Q; q++) acc[q] += t[q];
            if (o < 0 || o >= left) continue;
            const bool whole = c * kCell + k == W - 1;
            double S[Q];
#pragma unroll
            for (int q = 0; q < Q; q++) {
                const double h = c > 0 ? v[q] + acc[q] : acc[q];
                S[q] = whole ? h : G[q][slot(o)] + h;
            }
            out(o, S);
        }
    }
    __syncthreads();
}

template <int KIND, bool NT, int OUT>
__global__ __launch_bounds__(kBlock) void mov_kernel(const Args a)
{
    constexpr int Q = nq<KIND>();
    constexpr bool SEARCH = OUT == OUT_SEARCH;
    __shared__ double G[Q][kSlots];
    __shared__ double EP[Q][kCells], ES[Q][kCells];
    static_assert(sizeof(double) * kCells >= 4 * sizeof(Peak), "the search records reuse EP[0]");

    const int tid = (int)threadIdx.x;
    const aeth::red::Geo geo = aeth::red::geo_of<kChunk>(a.n, a.block, a.cpb);
    const int W = a.window, left = (int)geo.left;
    const long long g = (long long)geo.g, L = (long long)a.lag, H = (long long)(W - 1) + L;

    // windows up to kStageWindow: the samples the chunk needs, and their lag partners, once into LDS (consecutive lanes,
    // consecutive samples; slot r + r / 32 as for G), so that the passes below wait for LDS and not for memory
    __shared__ float2 stage[KIND == AETH_MOV_LAG ? 2 : 1][kStage];
    const bool staged = W <= kStageWindow;
    const Terms<NT> direct{a.x, a.hist, g, H, L, -(W - 1), left - 1, nullptr, nullptr};
    if (staged) {
        const Terms<NT> far{a.x, a.hist, g - L, H, L, -(W - 1), left - 1, nullptr, nullptr};
        for (int at = tid; at < left + W - 1; at += kBlock) {
            const int s = at + (at >> 5);
            stage[0][s] = direct.sample(g + (at - (W - 1)), true);
            if constexpr (KIND == AETH_MOV_LAG) stage[1][s] = far.sample(g - L + (at - (W - 1)), true);
        }
        __syncthreads();
    }
    const float2 *sx = staged ? stage[0] : nullptr, *sp = staged ? stage[KIND == AETH_MOV_LAG ? 1 : 0] : nullptr;
    if constexpr (KIND == AETH_MOV_LAG) {
        // R(i - L) first, on the grid of the indices i - L, left in plane 3 for the lanes that will own the outputs below
        const Terms<NT> back{a.x, a.hist, g - L, H, L, -(W - 1), left - 1, sp, sp};
        window_sums<1>(g - L, left, W, back, G + 3, EP, ES, [&](int o, const double (&S)[1]) { G[3][slot(o)] = S[0]; });
    }
    const Terms<NT> terms{a.x, a.hist, g, H, L, -(W - 1), left - 1, sx, sp};
    Cand best = cand_none(a.n);
    float best_m = 0.0f;
    unsigned n_nan = 0;
    window_sums<KIND == AETH_MOV_LAG ? 3 : 1>(g, left, W, terms, G, EP, ES, [&](int o, const auto &S) {
        float M;
        double R, Rl = 0.0;
        bool gate;
        if constexpr (KIND == AETH_MOV_LAG) {
            Rl = G[3][slot(o)];
            const double num = S[0] * S[0] + S[1] * S[1], den = S[2] * Rl;
            M = den == 0.0 ? 0.0f : (float)(num / den);
            R = S[2];
            gate = R >= a.r_min && Rl >= a.r_min;
        } else {
            M = (float)(S[0] / (double)W);
            R = S[0];
            gate = R >= a.r_min;
        }
        if constexpr (SEARCH) {
            const bool nan = M != M;
            n_nan += nan ? 1u : 0u;
            const uint64_t i = (uint64_t)(g + o);
            if (!nan && gate) {
                if (best.index == a.n || M > best_m) {               // ascending inside a lane: the first of equals stays
                    best.index = i; best_m = M; best.r = R;
                    if constexpr (KIND == AETH_MOV_LAG) { best.p_re = S[0]; best.p_im = S[1]; best.r_lag = Rl; }
                }
                if ((double)M >= a.threshold && i < best.first) best.first = i;
            }
        } else {
            // staged in the slots this lane has just read: p in plane 0, (r, m) in plane 1 (the power kind: plane 0)
            if constexpr (KIND == AETH_MOV_LAG) {
                G[0][slot(o)] = __builtin_bit_cast(double, make_float2((float)S[0], (float)S[1]));
                G[1][slot(o)] = __builtin_bit_cast(double, make_float2((float)R, M));
            } else {
                G[0][slot(o)] = __builtin_bit_cast(double, make_float2((float)R, M));
            }
        }
    });
    if constexpr (SEARCH) {
        best.mn = cand_pack(best.index == a.n ? __builtin_nanf("") : best_m, n_nan);
        best = aeth::red::block_reduce(best, reinterpret_cast<Cand *>(&EP[0][0]),
                                       [&](const Cand &p, const Cand &q) { return cand_combine(p, q, a.n); });
        if (tid == 0) a.rec[a.direct ? geo.b : blockIdx.x] = best;
    } else {
        for (int o = tid; o < left; o += kBlock) {
            const size_t i = geo.g + (size_t)o;
            if constexpr (KIND == AETH_MOV_LAG) {
                if constexpr ((OUT & OUT_P) != 0) aeth::nt_store<NT>(a.p + i, __builtin_bit_cast(float2, G[0][slot(o)]));
            }
            const float2 rm = __builtin_bit_cast(float2, G[KIND == AETH_MOV_LAG ? 1 : 0][slot(o)]);
            if constexpr ((OUT & OUT_R) != 0) aeth::nt_store<NT>(a.r + i, rm.x);
            if constexpr ((OUT & OUT_M) != 0) aeth::nt_store<NT>(a.m + i, rm.y);
        }
    }
}

// workgroup b folds in[b * per .. min((b + 1) * per, total)) into out[b]
__global__ __launch_bounds__(kBlock) void mov_fold_kernel(const Cand *__restrict__ in, size_t per, size_t total, size_t n, Cand *__restrict__ out)
{
    __shared__ Cand lds[4];
    const Cand a = aeth::red::fold(in, per, total, cand_none(n), lds, [&](const Cand &p, const Cand &q) { return cand_combine(p, q, n); });
    if (threadIdx.x == 0) out[blockIdx.x] = a;
}

// what both device calls check behind their outputs, in this order, before any device work
int check_call(int kind, size_t window, size_t lag, const aeth_cf32 *hist_dev, const aeth_cf32 *x_dev, size_t n)
{
    AETH_REQUIRE(n != 0, AETH_E_LEN, "a moving window over an empty vector");
    AETH_REQUIRE(kind == AETH_MOV_LAG || kind == AETH_MOV_POWER, AETH_E_ARG, "bad window kind %d", kind);
    AETH_REQUIRE(window != 0, AETH_E_ARG, "window 0");
    AETH_REQUIRE(window <= kMaxWindow, AETH_E_UNSUPPORTED, "window %zu is above %zu", window, kMaxWindow);
    if (kind == AETH_MOV_LAG) {
        AETH_REQUIRE(lag != 0, AETH_E_ARG, "lag 0 with the lag kind");
        AETH_REQUIRE(lag <= kMaxLag, AETH_E_UNSUPPORTED, "lag %zu is above %zu", lag, kMaxLag);
    } else {
        AETH_REQUIRE(lag == 0, AETH_E_ARG, "lag %zu with the power kind (it takes 0)", lag);
    }
    AETH_REQUIRE(aeth::aligned8(x_dev) && aeth::aligned8(hist_dev), AETH_E_ALIGN, "input %p or history %p not 8-byte aligned",
                 (const void *)x_dev, (const void *)hist_dev);
    return AETH_OK;
}

struct Range { const void *p; size_t bytes; const char *name; };

// no output may share a byte with an input or with another output
int check_overlap(const Range *in, int n_in, const Range *out, int n_out)
{
    for (int o = 0; o < n_out; o++) {
        for (int i = 0; i < n_in; i++)
            AETH_REQUIRE(!aeth::ranges_touch(out[o].p, out[o].bytes, in[i].p, in[i].bytes), AETH_E_ARG, "%s at %p overlaps %s at %p",
                         out[o].name, out[o].p, in[i].name, in[i].p);
        for (int i = 0; i < o; i++)
            AETH_REQUIRE(!aeth::ranges_touch(out[o].p, out[o].bytes, out[i].p, out[i].bytes), AETH_E_ARG, "%s at %p overlaps %s at %p",
                         out[o].name, out[o].p, out[i].name, out[i].p);
    }
    return AETH_OK;
}

template <int KIND, int OUT> void launch(hipStream_t s, bool nt, unsigned nwg, const Args &a)
{
    if (nt) hipLaunchKernelGGL((mov_kernel<KIND, true, OUT>), dim3(nwg), dim3(kBlock), 0, s, a);
    else hipLaunchKernelGGL((mov_kernel<KIND, false, OUT>), dim3(nwg), dim3(kBlock), 0, s, a);
}

template <int KIND> void launch_planes(hipStream_t s, bool nt, unsigned nwg, const Args &a, int out)
{
    switch (out) {
    case 1: if constexpr (KIND == AETH_MOV_LAG) launch<KIND, 1>(s, nt, nwg, a); break;
    case 2: launch<KIND, 2>(s, nt, nwg, a); break;
    case 3: if constexpr (KIND == AETH_MOV_LAG) launch<KIND, 3>(s, nt, nwg, a); break;
    case 4: launch<KIND, 4>(s, nt, nwg, a); break;
    case 5: if constexpr (KIND == AETH_MOV_LAG) launch<KIND, 5>(s, nt, nwg, a); break;
    case 6: launch<KIND, 6>(s, nt, nwg, a); break;
    default: if constexpr (KIND == AETH_MOV_LAG) launch<KIND, 7>(s, nt, nwg, a); break;
    }
}

size_t history_of(int kind, size_t window, size_t lag) { return window - 1 + (kind == AETH_MOV_LAG ? lag : 0); }

}  // namespace

extern "C" {

size_t aeth_mov_history(int kind, size_t window, size_t lag)
{
    if ((kind != AETH_MOV_LAG && kind != AETH_MOV_POWER) || window == 0) return 0;
    return history_of(kind, window, lag);
}

size_t aeth_mov_grid(int kind, size_t window)
{
    if ((kind != AETH_MOV_LAG && kind != AETH_MOV_POWER) || window == 0 || window > kMaxWindow) return 0;
    return window;
}

uint64_t aeth_mov_freq_step(const aeth_mov_peak *p, size_t lag)
{
    if (!p || lag == 0 || (p->p_re == 0.0 && p->p_im == 0.0)) return 0;
    return aeth_nco_word(-std::atan2(p->p_im, p->p_re) / (6.283185307179586476925286766559 * (double)lag));
}

int aeth_mov_exec(aeth_ctx *ctx, int kind, size_t window, size_t lag, const aeth_cf32 *hist_dev, const aeth_cf32 *x_dev, size_t n,
                  aeth_cf32 *p_dev, float *r_dev, float *m_dev)
{
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    AETH_REQUIRE(x_dev, AETH_E_ARG, "x is null");
    AETH_REQUIRE(p_dev || r_dev || m_dev, AETH_E_ARG, "every output plane is null");
    int rc = check_call(kind, window, lag, hist_dev, x_dev, n); if (rc) return rc;
    AETH_REQUIRE(kind == AETH_MOV_LAG || !p_dev, AETH_E_ARG, "the power kind has no p plane (p_dev %p)", (void *)p_dev);
    AETH_REQUIRE(aeth::aligned8(p_dev), AETH_E_ALIGN, "p_dev %p not 8-byte aligned", (void *)p_dev);
    AETH_REQUIRE(aeth::aligned4(r_dev) && aeth::aligned4(m_dev), AETH_E_ALIGN, "r_dev %p or m_dev %p not 4-byte aligned", (void *)r_dev,
                 (void *)m_dev);
    const Range in[2] = {{x_dev, n * sizeof(aeth_cf32), "x_dev"}, {hist_dev, history_of(kind, window, lag) * sizeof(aeth_cf32), "hist_dev"}};
    const Range out[3] = {{p_dev, n * sizeof(aeth_cf32), "p_dev"}, {r_dev, n * sizeof(float), "r_dev"}, {m_dev, n * sizeof(float), "m_dev"}};
    rc = check_overlap(in, 2, out, 3); if (rc) return rc;
    Cut c;
    AETH_REQUIRE(aeth::red::cut_of(n, 0, kChunk, c), AETH_E_UNSUPPORTED, "%zu samples need 2^31 workgroups or more", n);

    aeth::DeviceGuard dev_guard(ctx->device);
    const bool nt = aeth::streams_past_cache(n * sizeof(float2));
    Args a{reinterpret_cast<const float2 *>(x_dev), reinterpret_cast<const float2 *>(hist_dev), n, c.block, aeth::make_fastdiv((uint32_t)c.cpb),
           (int)window, (unsigned)lag, 0.0, 0.0, reinterpret_cast<float2 *>(p_dev), r_dev, m_dev, nullptr, 0};
    const int outs = (p_dev ? OUT_P : 0) | (r_dev ? OUT_R : 0) | (m_dev ? OUT_M : 0);
    hipStream_t s = aeth::ctx_stream(ctx);
    if (kind == AETH_MOV_LAG) launch_planes<AETH_MOV_LAG>(s, nt, (unsigned)c.nwg, a, outs);
    else launch_planes<AETH_MOV_POWER>(s, nt, (unsigned)c.nwg, a, outs);
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

int aeth_mov_search(aeth_ctx *ctx, int kind, size_t window, size_t lag, double r_min, double threshold, const aeth_cf32 *hist_dev,
                    const aeth_cf32 *x_dev, size_t n, size_t block, aeth_mov_peak *peaks_dev, aeth_mov_peak *best_host)
{
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    AETH_REQUIRE(x_dev, AETH_E_ARG, "x is null");
    AETH_REQUIRE(peaks_dev || best_host, AETH_E_ARG, "both outputs are null");
    int rc = check_call(kind, window, lag, hist_dev, x_dev, n); if (rc) return rc;
    AETH_REQUIRE(r_min >= 0.0, AETH_E_ARG, "r_min %g is negative or NaN", r_min);
    AETH_REQUIRE(threshold == threshold, AETH_E_ARG, "threshold %g is NaN", threshold);
    AETH_REQUIRE(aeth::aligned8(peaks_dev) && aeth::aligned8(best_host), AETH_E_ALIGN, "peaks_dev %p or best_host %p not 8-byte aligned",
                 (void *)peaks_dev, (void *)best_host);
    Cut c;
    AETH_REQUIRE(aeth::red::cut_of(n, block, kChunk, c), AETH_E_UNSUPPORTED, "%zu samples in blocks of %zu need 2^31 workgroups or more", n, block);
    const Range in[2] = {{x_dev, n * sizeof(aeth_cf32), "x_dev"}, {hist_dev, history_of(kind, window, lag) * sizeof(aeth_cf32), "hist_dev"}};
    const Range out[1] = {{peaks_dev, c.nb * sizeof(Peak), "peaks_dev"}};
    rc = check_overlap(in, 2, out, 1); if (rc) return rc;

    const bool nt = aeth::streams_past_cache(n * sizeof(float2));
    Args a{reinterpret_cast<const float2 *>(x_dev), reinterpret_cast<const float2 *>(hist_dev), n, c.block, aeth::make_fastdiv((uint32_t)c.cpb),
           (int)window, (unsigned)lag, r_min, threshold, nullptr, nullptr, nullptr, nullptr, 0};
    return aeth::red::run_blocks(ctx, ctx->mov_slab, c, reinterpret_cast<Cand *>(peaks_dev), best_host,
        [&](hipStream_t s, unsigned nwg, const Cand *in, size_t per, size_t total, Cand *out) {
            hipLaunchKernelGGL(mov_fold_kernel, dim3(nwg), dim3(kBlock), 0, s, in, per, total, n, out);
        },
        [&](hipStream_t s, Cand *out, int direct) {
            a.rec = out; a.direct = direct;
            if (kind == AETH_MOV_LAG) launch<AETH_MOV_LAG, OUT_SEARCH>(s, nt, (unsigned)c.nwg, a);
            else launch<AETH_MOV_POWER, OUT_SEARCH>(s, nt, (unsigned)c.nwg, a);
        });
}

}  // extern "C"
