// aeth_ofdm.hip -- OFDM symbols on the device (include/aether_hip.h, aeth_ofdm_*; no body in the reference, which has
// `Fft`, `VecOps::vec_mul` and `chunks_mut(fft_len)` framing only).
//
//   demod      symbol s is the window in[s*L + e], e < N, L = N + G: transform, pick the K carriers, one-tap equaliser
//   mod        carriers onto an otherwise zero grid, inverse transform, cyclic prefix in front
//   estimate   per carrier: sum of Y conj(X) over the training symbols in f64, H, the equaliser's coefficient, |H|^2
//
// Two routes, the same bytes:
//   fused      N = 64 .. 4096, power of two: ONE kernel per call, the register transform of aeth_fft_core.h between a
//              load and a store that do the framing -- 8 (N + K) bytes per symbol.  Same Cfg, same per-lane twiddle table
//              (the inner plan's), same butterflies and the same image-parity bookkeeping as fft_pow2_kernel
//              (aeth_fft.hip); every arithmetic instruction of the transform is inline assembly there, so the bins come out
//              bit for bit as from aeth_fft_exec.
//   general    every other length the planner accepts, and every length under AETH_OFDM_GENERAL: strip (or place) into the
//              object's scratch, aeth::fft_run on contiguous frames, pick (or prefix).
//
// This file is built with -ffp-contract=fast like the other transform kernels.  The equaliser's product is kept from fusing
// by eq_mul below; the estimator's f64 products are exact, so fusing cannot change its sums.
#include "aeth_internal.h"
#include "aeth_fft_core.h"
#include "aeth_fft_plan.h"

#include <new>
#include <string>
#include <type_traits>
#include <vector>

using namespace aeth::fftk;

namespace {

constexpr int kBlock = 256;
constexpr int DIR_DEMOD = 0, DIR_MOD = 1;

#ifndef AETH_OFDM_STAGE_T
#define AETH_OFDM_STAGE_T 24            /* as AETH_STAGE_T of aeth_fft.hip */
#endif
template <class C> constexpr bool ofdm_staged_io() { return C::T < AETH_OFDM_STAGE_T && C::F > 1; }
template <class C> struct OneImage : C {
    static constexpr bool DB = false;
    static constexpr int LDS_TOTAL = C::LDS_ELEMS;
};

// v * w exactly as aeth_vec_mul_frames makes it: four products, a difference and a sum, each rounded on its own.
// This file is built with -ffp-contract=fast, under which the backend fuses a product into the sum that uses it whatever
// the source says: neither `#pragma clang fp contract(off)` nor __fmul_rn (a plain operator in HIP) stops it (both were
// tried: v_pk_fma_f32 in the code object, last-bit differences on the device).  So every product passes through an integer
// xor with `zero`, a kernel argument that is always 0: the compiler cannot see through it, and a rounded product is what
// reaches the sum.  Four v_xor_b32 per carrier.
__device__ __forceinline__ float rounded(float p, unsigned zero) { return __uint_as_float(__float_as_uint(p) ^ zero); }
__device__ __forceinline__ cf eq_mul(cf v, cf w, unsigned zero)
{
    const float rr = rounded(v.x * w.x, zero), ii = rounded(v.y * w.y, zero), ri = rounded(v.x * w.y, zero), ir = rounded(v.y * w.x, zero);
    return mk(rr - ii, ri + ir);
}

// What a call hands its kernel.  demod: src = the first window sample, dst = n_sym * K carriers; mod: the other way round.
struct OfdmArgs {
    const cf *src;
    cf *dst;
    const cf *eq;               // demod with EQ: K coefficients
    const int *slot;            // N entries: the carrier of a bin, -1 for none
    const unsigned *bins;       // K entries: the bin of a carrier
    const cf *twL;              // the inner plan's per-lane twiddle table
    size_t n_sym;
    unsigned K, G;
    aeth::FastDiv kdiv, ldiv;   // o / K and o / L for the coalesced copies of the short frames
    float scale;
    unsigned zero;              // 0 (see eq_mul)
};

// DIR: DIR_DEMOD / DIR_MOD.  EQ: demod multiplies by eq[k].  NT: the samples stream past the cache (aeth_internal.h).
template <class C0, int DIR, bool EQ, bool NT>
__global__ __launch_bounds__(C0::WG) void ofdm_fused_kernel(OfdmArgs a)
{
    constexpr int S = DIR == DIR_DEMOD ? +1 : -1;           // Fft::fwd / Fft::bwd (aeth_fft_core.h)
    constexpr bool STAGED = ofdm_staged_io<C0>();
    static_assert(C0::IDLE == 0, "power-of-two shapes have no idle lanes");
    // short frames: ONE exchange image, and the I/O staging area shares its LDS, as in fft_pow2_kernel
    using C = typename std::conditional<STAGED, OneImage<C0>, C0>::type;
    constexpr int N = C::N, T = C::T, P = C::P, F = C::F, WG = C::WG;
    constexpr int IO_ELEMS = STAGED ? F * (N + 1) : 0;
    constexpr int LDS_N = C::LDS_TOTAL > IO_ELEMS ? C::LDS_TOTAL : IO_ELEMS;
    __shared__ cf lds_all[LDS_N];
    cf *lds_io = lds_all;
    constexpr bool WHOLE = F == 1;
    const int tid = WHOLE ? (int)threadIdx.x : (int)(threadIdx.x % T);
    const int fl = WHOLE ? 0 : (int)(threadIdx.x / T);
    cf *lds = lds_all + fl * C::LDS_FRAME;
    const size_t K = a.K, G = a.G, L = (size_t)N + G;

    cf tw[C::TW];
    load_twiddles_lane<C>(tw, a.twL, tid);
    // the carrier of this lane's bins, the same for every symbol (short frames store demod's carriers in output order
    // and never ask)
    constexpr bool SLOTS = DIR == DIR_MOD || !STAGED;
    int slot[SLOTS ? P : 1];
    if constexpr (SLOTS) {
#pragma unroll
        for (int m = 0; m < P; m++) slot[m] = a.slot[tid + m * T];
    }
    // short frames, mod: where the carrier of each bin sits in the staged copy of the group's carriers; a bin without a
    // carrier reads the zero kept behind them (an index, not a branch per bin: sixteen hoisted lane masks spill SGPRs)
    constexpr int ZERO_AT = F * N;
    if constexpr (STAGED && DIR == DIR_MOD) {
#pragma unroll
        for (int m = 0; m < P; m++) slot[m] = slot[m] >= 0 ? fl * (int)K + slot[m] : ZERO_AT;
    }

    const size_t ngroups = (a.n_sym + F - 1) / F;
    const cf ss = mk(a.scale, a.scale);
    bool par = false;
    for (size_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const size_t sym0 = g * F, frame = sym0 + fl;
        const bool active = frame < a.n_sym;
        const int nact = a.n_sym - sym0 < (size_t)F ? (int)(a.n_sym - sym0) : F;     // symbols of this group
        cf w[P];
        if constexpr (STAGED && DIR == DIR_DEMOD) {
            // the group's windows without their prefixes: element e of the staging area is sample e % N of window e / N
            constexpr int ITER = F * N / WG;
            cf stage[ITER];
#pragma unroll
            for (int q = 0; q < ITER; q++) {
                const int e = threadIdx.x + q * WG, f = e / N, j = e % N;
                stage[q] = f < nact ? aeth::nt_load<NT>(a.src + (sym0 + f) * L + j) : mk(0.f, 0.f);
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < ITER; q++) {
                const int e = threadIdx.x + q * WG;
                lds_io[e + e / N] = stage[q];
            }
            __syncthreads();
#pragma unroll
            for (int m = 0; m < P; m++) w[m] = lds_io[fl * (N + 1) + tid + m * T];
        } else if constexpr (STAGED && DIR == DIR_MOD) {
            // the group's nact * K carriers are contiguous: coalesced into LDS, then every lane picks its bins' carriers
            constexpr int ITER = F * N / WG;                // K <= N
            const unsigned have = (unsigned)nact * (unsigned)K;
            cf stage[ITER];
#pragma unroll
            for (int q = 0; q < ITER; q++) {
                const unsigned o = threadIdx.x + q * WG;
                stage[q] = o < have ? aeth::nt_load<NT>(a.src + sym0 * K + o) : mk(0.f, 0.f);
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < ITER; q++) {
                const unsigned o = threadIdx.x + q * WG;
                if (o < have) lds_io[o] = stage[q];
            }
            if (threadIdx.x == 0) lds_io[ZERO_AT] = mk(0.f, 0.f);
            __syncthreads();
            // (a symbol past the end reads what the area held before: it is transformed and never stored)
#pragma unroll
            for (int m = 0; m < P; m++) w[m] = lds_io[slot[m]];
        } else if constexpr (DIR == DIR_DEMOD) {
            const cf *src = a.src + frame * L + tid;
#pragma unroll
            for (int m = 0; m < P; m++) w[m] = active ? aeth::nt_load<NT>(src + m * T) : mk(0.f, 0.f);
        } else {
            const cf *src = a.src + frame * K;
#pragma unroll
            for (int m = 0; m < P; m++) w[m] = (active && slot[m] >= 0) ? aeth::nt_load<NT>(src + slot[m]) : mk(0.f, 0.f);
        }
        // an odd number of exchanges per transform flips the image parity every symbol
        if (fft_next_par<C>(0) == 0 || !par) fft_in_regs<C, S, 0>(w, tw, lds, tid);
        else fft_in_regs<C, S, 1>(w, tw, lds, tid);
        par = (fft_next_par<C>(0) != 0) && !par;
        if constexpr (STAGED) {
            __syncthreads();
#pragma unroll
            for (int m = 0; m < P; m++) lds_io[fl * (N + 1) + tid + m * T] = cscale_k(w[m], ss);
            __syncthreads();
            if constexpr (DIR == DIR_DEMOD) {
                // output o of the group is carrier o % K of symbol o / K: coalesced stores, the bins gathered from LDS
                // (a rolled loop: unrolled, the compiler keeps every lane's bins and coefficients in registers across
                // symbols and the kernel loses a wave per SIMD)
                const unsigned have = (unsigned)nact * (unsigned)K;
                cf *dst = a.dst + sym0 * K;
#pragma unroll 2
                for (unsigned o = threadIdx.x; o < have; o += WG) {
                    const unsigned f = aeth::fdiv(o, a.kdiv), k = o - f * (unsigned)K;
                    cf v = lds_io[f * (N + 1) + a.bins[k]];
                    if constexpr (EQ) v = eq_mul(v, a.eq[k], a.zero);
                    aeth::nt_store<NT>(dst + o, v);
                }
            } else {
                // sample o of the group is position o % L of symbol o / L: the prefix repeats the last G time samples
                const unsigned have = (unsigned)nact * (unsigned)L;
                cf *dst = a.dst + sym0 * L;
                for (unsigned o = threadIdx.x; o < have; o += WG) {
                    const unsigned f = aeth::fdiv(o, a.ldiv), j = o - f * (unsigned)L;
                    const unsigned e = j < (unsigned)G ? j + (N - (unsigned)G) : j - (unsigned)G;
                    aeth::nt_store<NT>(dst + o, lds_io[f * (N + 1) + e]);
                }
            }
        } else if (active) {
            if constexpr (DIR == DIR_DEMOD) {
                cf *dst = a.dst + frame * K;
#pragma unroll
                for (int m = 0; m < P; m++) {
                    if (slot[m] >= 0) {
                        cf v = cscale_k(w[m], ss);
                        if constexpr (EQ) v = eq_mul(v, a.eq[slot[m]], a.zero);
                        aeth::nt_store<NT>(dst + slot[m], v);
                    }
                }
            } else {
                cf *dst = a.dst + frame * L;
                const int tail = N - (int)G;                // time samples from here on are the prefix as well
#pragma unroll
                for (int m = 0; m < P; m++) {
                    const int e = tid + m * T;
                    const cf v = cscale_k(w[m], ss);
                    aeth::nt_store<NT>(dst + G + e, v);
                    if (e >= tail) aeth::nt_store<NT>(dst + (e - tail), v);
                }
            }
        }
    }
}

// ---- the general route's copies: one lane per element, grid-stride ----
// frames[s * N + e] = in[s * L + e]
__global__ __launch_bounds__(kBlock) void ofdm_strip_kernel(const cf *__restrict__ in, cf *__restrict__ frames, size_t n_sym, unsigned N, size_t L)
{
    const size_t total = n_sym * N;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
        const size_t s = i / N, e = i - s * N;
        frames[i] = in[s * L + e];
    }
}
// out[s * K + k] = frames[s * N + bins[k]] (* eq[k])
template <bool EQ>
__global__ __launch_bounds__(kBlock) void ofdm_pick_kernel(const cf *__restrict__ frames, const unsigned *__restrict__ bins,
                                                           const cf *__restrict__ eq, cf *__restrict__ out, size_t n_sym, unsigned N, unsigned K, unsigned zero)
{
    const size_t total = n_sym * K;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
        const size_t s = i / K, k = i - s * K;
        cf v = frames[s * N + bins[k]];
        if constexpr (EQ) v = eq_mul(v, eq[k], zero);
        out[i] = v;
    }
}
// frames[s * N + e] = the carrier of bin e, or zero
__global__ __launch_bounds__(kBlock) void ofdm_place_kernel(const cf *__restrict__ car, const int *__restrict__ slot, cf *__restrict__ frames,
                                                            size_t n_sym, unsigned N, unsigned K)
{
    const size_t total = n_sym * N;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
        const size_t s = i / N, e = i - s * N;
        const int k = slot[e];
        frames[i] = k >= 0 ? car[s * K + k] : mk(0.f, 0.f);
    }
}
// out[s * L + j] = frames[s * N + (j < G ? j + N - G : j - G)]
__global__ __launch_bounds__(kBlock) void ofdm_prefix_kernel(const cf *__restrict__ frames, cf *__restrict__ out, size_t n_sym, unsigned N, unsigned G)
{
    const size_t L = (size_t)N + G, total = n_sym * L;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (size_t)gridDim.x * kBlock) {
        const size_t s = i / L, j = i - s * L;
        out[i] = frames[s * N + (j < G ? j + (N - G) : j - G)];
    }
}

// ---- the estimator: one lane per carrier, the definition of include/aether_hip.h line by line ----
// (every f64 product below has two widened f32 operands and is exact, so a line is one rounding with or without fma;
// contraction is switched off all the same)
__global__ __launch_bounds__(kBlock) void ofdm_estimate_kernel(const cf *__restrict__ y, const cf *__restrict__ x, size_t n_sym, int x_every,
                                                               unsigned K, float nv, int eq_kind, cf *__restrict__ h_out,
                                                               cf *__restrict__ eq_out, float *__restrict__ csi_out)
{
#pragma clang fp contract(off)
    const unsigned k = blockIdx.x * kBlock + threadIdx.x;
    if (k >= K) return;
    double nr = 0.0, ni = 0.0, den = 0.0;
    for (size_t s = 0; s < n_sym; s++) {
        const cf yv = y[s * K + k], xv = x[(x_every ? s : 0) * K + k];
        const double yr = yv.x, yi = yv.y, xr = xv.x, xi = xv.y;
        nr += yr * xr + yi * xi;
        ni += yi * xr - yr * xi;
        den += xr * xr + xi * xi;
    }
    float hr = 0.f, hi = 0.f;
    if (den != 0.0) { hr = (float)(nr / den); hi = (float)(ni / den); }
    const double hrd = hr, hid = hi;
    const double p = hrd * hrd + hid * hid;
    if (h_out) h_out[k] = mk(hr, hi);
    if (csi_out) csi_out[k] = (float)p;
    if (eq_out) {
        cf wv;
        if (eq_kind == AETH_OFDM_EQ_MATCHED) wv = mk(hr, -hi);
        else {
            const double d = p + (eq_kind == AETH_OFDM_EQ_MMSE ? (double)nv : 0.0);
            wv = d != 0.0 ? mk((float)(hrd / d), (float)(-hid / d)) : mk(0.f, 0.f);
        }
        eq_out[k] = wv;
    }
}

// ---- host side ----
bool fused_length(size_t n) { return n == 64 || n == 128 || n == 256 || n == 512 || n == 1024 || n == 2048 || n == 4096; }

unsigned copy_grid(const aeth_ctx *ctx, size_t total)
{
    const size_t blocks = (total + kBlock - 1) / kBlock, cap = (size_t)ctx->num_cus * 32;
    return (unsigned)(blocks < 1 ? 1 : blocks < cap ? blocks : cap);
}

template <class C, int DIR>
int launch_fused(const aeth_ofdm *p, const OfdmArgs &a, bool eq, bool nt)
{
    const aeth_ctx *ctx = p->ctx;
    const size_t ngroups = (a.n_sym + C::F - 1) / C::F, cap = (size_t)ctx->num_cus * 8;
    const unsigned grid = (unsigned)(ngroups < cap ? ngroups : cap);
#define AETH_OFDM_GO(EE, NN) hipLaunchKernelGGL((ofdm_fused_kernel<C, DIR, EE, NN>), dim3(grid), dim3(C::WG), 0, aeth::ctx_stream(ctx), a)
    if constexpr (DIR == DIR_DEMOD) {
        if (eq) { if (nt) AETH_OFDM_GO(true, true); else AETH_OFDM_GO(true, false); }
        else    { if (nt) AETH_OFDM_GO(false, true); else AETH_OFDM_GO(false, false); }
    } else {
        if (nt) AETH_OFDM_GO(false, true); else AETH_OFDM_GO(false, false);
    }
#undef AETH_OFDM_GO
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

template <int DIR>
int dispatch_fused(const aeth_ofdm *p, const OfdmArgs &a, bool eq, bool nt)
{
    switch (p->n_fft) {
#define AETH_BODY(NN) case NN: return launch_fused<typename CfgFor<NN>::type, DIR>(p, a, eq, nt)
    AETH_BODY(64); AETH_BODY(128); AETH_BODY(256); AETH_BODY(512); AETH_BODY(1024); AETH_BODY(2048); AETH_BODY(4096);
#undef AETH_BODY
    default: return aeth::set_error(AETH_E_UNSUPPORTED, "ofdm fused route: length %zu", p->n_fft);
    }
}

OfdmArgs fused_args(const aeth_ofdm *p, const aeth_cf32 *src, aeth_cf32 *dst, const aeth_cf32 *eq, size_t n_sym, float scale)
{
    OfdmArgs a;
    a.src = (const cf *)src; a.dst = (cf *)dst; a.eq = (const cf *)eq;
    a.slot = p->slot_dev; a.bins = p->bins_dev; a.twL = (const cf *)p->fft->tw_lane_dev;
    a.n_sym = n_sym; a.K = (unsigned)p->n_bins; a.G = (unsigned)p->cp;
    a.kdiv = aeth::make_fastdiv((uint32_t)p->n_bins);
    a.ldiv = aeth::make_fastdiv((uint32_t)(p->n_fft + p->cp));
    a.scale = scale;
    a.zero = 0;
    return a;
}

// the general route's frames: n_sym * N samples of the object's scratch (exact size: it is sized by max_symbols)
int frames_of(aeth_ofdm *p, size_t n_sym, cf **frames)
{
    int rc = aeth::scratch_ensure(p->ctx, p->scratch, n_sym * p->n_fft * sizeof(float2), false); if (rc) return rc;
    *frames = static_cast<cf *>(p->scratch.p);
    return AETH_OK;
}

// what demod and mod check after their lengths
int check_io(const aeth_ofdm *p, const aeth_cf32 *in, size_t n_in, const aeth_cf32 *eq, const aeth_cf32 *out, size_t n_out)
{
    AETH_REQUIRE(in && out, AETH_E_ARG, "null pointer");
    AETH_REQUIRE(aeth::aligned8(in) && aeth::aligned8(out) && aeth::aligned8(eq), AETH_E_ALIGN, "pointer not 8-byte aligned");
    AETH_REQUIRE(!aeth::ranges_touch(out, n_out * sizeof(aeth_cf32), in, n_in * sizeof(aeth_cf32)), AETH_E_ARG,
                 "the output range overlaps the input (in place is not supported)");
    AETH_REQUIRE(!aeth::ranges_touch(out, n_out * sizeof(aeth_cf32), eq, p->n_bins * sizeof(aeth_cf32)), AETH_E_ARG,
                 "the output range overlaps the equaliser's coefficients");
    return AETH_OK;
}

int check_symbols(const aeth_ofdm *p, size_t n_sym)
{
    AETH_REQUIRE(p->max_symbols == 0 || n_sym <= p->max_symbols, AETH_E_ARG, "%zu symbols in one call, the object was created for %zu",
                 n_sym, p->max_symbols);
    AETH_REQUIRE(n_sym <= ((size_t)1 << 31), AETH_E_UNSUPPORTED, "%zu symbols in one call: more than 2^31", n_sym);
    return AETH_OK;
}

}  // namespace

extern "C" {

int aeth_ofdm_create(aeth_ctx *ctx, size_t n_fft, size_t cp, const uint32_t *bins_host, size_t n_bins, size_t max_symbols, int flags,
                     aeth_ofdm **out)
{
    AETH_REQUIRE(out, AETH_E_ARG, "null argument: out");
    *out = nullptr;
    AETH_REQUIRE(ctx, AETH_E_ARG, "null argument: ctx");
    AETH_REQUIRE(bins_host, AETH_E_ARG, "bins is null");
    AETH_REQUIRE((flags & ~AETH_OFDM_GENERAL) == 0, AETH_E_ARG, "unknown flags 0x%x", (unsigned)flags);
    AETH_REQUIRE(n_fft >= 2, AETH_E_ARG, "OFDM transform length %zu < 2", n_fft);
    AETH_REQUIRE(n_fft <= ((size_t)1 << 24), AETH_E_UNSUPPORTED, "FFT length %zu > 2^24", n_fft);     /* as aeth_fft_create */
    AETH_REQUIRE(cp <= n_fft, AETH_E_ARG, "cyclic prefix %zu longer than the transform (%zu)", cp, n_fft);
    AETH_REQUIRE(n_bins >= 1 && n_bins <= n_fft, AETH_E_ARG, "%zu carriers on %zu bins", n_bins, n_fft);
    AETH_REQUIRE(max_symbols <= ((size_t)1 << 31), AETH_E_UNSUPPORTED, "max_symbols %zu: more than 2^31", max_symbols);
    std::vector<int> slot(n_fft, -1);
    for (size_t k = 0; k < n_bins; k++) {
        AETH_REQUIRE(bins_host[k] < n_fft, AETH_E_ARG, "carrier %zu: bin %u is not below %zu", k, bins_host[k], n_fft);
        AETH_REQUIRE(slot[bins_host[k]] < 0, AETH_E_ARG, "carrier %zu: bin %u is carrier %d already", k, bins_host[k], slot[bins_host[k]]);
        slot[bins_host[k]] = (int)k;
    }
    // ---- device work from here on ----
    aeth::DeviceGuard g(ctx->device);
    aeth_ofdm *p = new (std::nothrow) aeth_ofdm();
    AETH_REQUIRE(p, AETH_E_NOMEM, "out of host memory");
    p->ctx = ctx; p->n_fft = n_fft; p->cp = cp; p->n_bins = n_bins; p->max_symbols = max_symbols; p->flags = flags;
    int rc = aeth_fft_create(ctx, n_fft, 1, &p->fft);                          /* its refusals pass through */
    p->fused = rc == AETH_OK && !(flags & AETH_OFDM_GENERAL) && fused_length(n_fft) && p->fft->algo == aeth::FFT_ALGO_POW2 && p->fft->tw_lane_dev;
    if (rc == AETH_OK) rc = aeth::upload_table(ctx, bins_host, n_bins * sizeof(uint32_t), &p->bins_dev, "OFDM carrier list");
    if (rc == AETH_OK) rc = aeth::upload_table(ctx, slot.data(), n_fft * sizeof(int), &p->slot_dev, "OFDM bin table");
    if (rc == AETH_OK && !p->fused && max_symbols) rc = aeth::scratch_ensure(ctx, p->scratch, max_symbols * n_fft * sizeof(float2), false);
    if (rc != AETH_OK) { aeth_ofdm_destroy(p); return rc; }
    p->route = p->fused ? std::string("fused") : std::string("general: ") + p->fft->route;
    *out = p;
    return AETH_OK;
}

int aeth_ofdm_destroy(aeth_ofdm *p)
{
    if (!p) return AETH_OK;
    aeth::DeviceGuard g(p->ctx->device);
    (void)hipStreamSynchronize(aeth::ctx_stream(p->ctx));
    if (p->fft) (void)aeth_fft_destroy(p->fft);
    if (p->bins_dev) (void)hipFree(p->bins_dev);
    if (p->slot_dev) (void)hipFree(p->slot_dev);
    (void)aeth::scratch_release(p->scratch);
    delete p;
    return AETH_OK;
}

size_t aeth_ofdm_len(const aeth_ofdm *p) { return p ? p->n_fft : 0; }
size_t aeth_ofdm_cp(const aeth_ofdm *p) { return p ? p->cp : 0; }
size_t aeth_ofdm_symbol(const aeth_ofdm *p) { return p ? p->n_fft + p->cp : 0; }
size_t aeth_ofdm_carriers(const aeth_ofdm *p) { return p ? p->n_bins : 0; }
const char *aeth_ofdm_route(const aeth_ofdm *p) { return p ? p->route.c_str() : ""; }
size_t aeth_ofdm_span(const aeth_ofdm *p, size_t n_sym) { return (p && n_sym) ? (n_sym - 1) * (p->n_fft + p->cp) + p->n_fft : 0; }

int aeth_ofdm_demod(aeth_ofdm *p, const aeth_cf32 *in_dev, size_t n_in, size_t n_sym, const aeth_cf32 *eq_dev, int scale_kind, float x,
                    aeth_cf32 *out_dev, size_t n_out)
{
    AETH_REQUIRE(p, AETH_E_ARG, "ofdm is null");
    int rc = aeth::check_sign_scale(AETH_SIGN_REF_FWD, scale_kind); if (rc) return rc;
    rc = check_symbols(p, n_sym); if (rc) return rc;
    AETH_REQUIRE(n_in >= aeth_ofdm_span(p, n_sym), AETH_E_LEN, "%zu input samples, %zu symbols read %zu", n_in, n_sym, aeth_ofdm_span(p, n_sym));
    AETH_REQUIRE(n_out == n_sym * p->n_bins, AETH_E_LEN, "%zu output carriers, %zu symbols of %zu make %zu", n_out, n_sym, p->n_bins,
                 n_sym * p->n_bins);
    if (n_sym == 0) return AETH_OK;
    const size_t span = aeth_ofdm_span(p, n_sym);
    rc = check_io(p, in_dev, span, eq_dev, out_dev, n_out); if (rc) return rc;
    const float s = aeth_scale_factor(scale_kind, p->n_fft, x);
    aeth::DeviceGuard dev_guard(p->ctx->device);
    if (p->fused) {
        const bool nt = aeth::streams_past_cache(n_sym * (p->n_fft + p->n_bins) * sizeof(float2));
        return dispatch_fused<DIR_DEMOD>(p, fused_args(p, in_dev, out_dev, eq_dev, n_sym, s), eq_dev != nullptr, nt);
    }
    cf *frames = nullptr;
    rc = frames_of(p, n_sym, &frames); if (rc) return rc;
    const unsigned N = (unsigned)p->n_fft, K = (unsigned)p->n_bins;
    hipLaunchKernelGGL(ofdm_strip_kernel, dim3(copy_grid(p->ctx, n_sym * N)), dim3(kBlock), 0, aeth::ctx_stream(p->ctx), (const cf *)in_dev,
                       frames, n_sym, N, p->n_fft + p->cp);
    AETH_HIP(hipGetLastError());
    rc = aeth::fft_run(p->fft, (const float2 *)frames, (float2 *)frames, n_sym, AETH_SIGN_REF_FWD, s); if (rc) return rc;
    if (eq_dev)
        hipLaunchKernelGGL(ofdm_pick_kernel<true>, dim3(copy_grid(p->ctx, n_sym * K)), dim3(kBlock), 0, aeth::ctx_stream(p->ctx),
                           (const cf *)frames, (const unsigned *)p->bins_dev, (const cf *)eq_dev, (cf *)out_dev, n_sym, N, K, 0u);
    else
        hipLaunchKernelGGL(ofdm_pick_kernel<false>, dim3(copy_grid(p->ctx, n_sym * K)), dim3(kBlock), 0, aeth::ctx_stream(p->ctx),
                           (const cf *)frames, (const unsigned *)p->bins_dev, (const cf *)nullptr, (cf *)out_dev, n_sym, N, K, 0u);
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

int aeth_ofdm_mod(aeth_ofdm *p, const aeth_cf32 *car_dev, size_t n_car, size_t n_sym, int scale_kind, float x, aeth_cf32 *out_dev,
                  size_t n_out)
{
    AETH_REQUIRE(p, AETH_E_ARG, "ofdm is null");
    int rc = aeth::check_sign_scale(AETH_SIGN_REF_BWD, scale_kind); if (rc) return rc;
    rc = check_symbols(p, n_sym); if (rc) return rc;
    const size_t L = p->n_fft + p->cp;
    AETH_REQUIRE(n_car == n_sym * p->n_bins, AETH_E_LEN, "%zu input carriers, %zu symbols of %zu make %zu", n_car, n_sym, p->n_bins,
                 n_sym * p->n_bins);
    AETH_REQUIRE(n_out == n_sym * L, AETH_E_LEN, "%zu output samples, %zu symbols of %zu make %zu", n_out, n_sym, L, n_sym * L);
    if (n_sym == 0) return AETH_OK;
    rc = check_io(p, car_dev, n_car, nullptr, out_dev, n_out); if (rc) return rc;
    const float s = aeth_scale_factor(scale_kind, p->n_fft, x);
    aeth::DeviceGuard dev_guard(p->ctx->device);
    if (p->fused) {
        const bool nt = aeth::streams_past_cache(n_sym * (L + p->n_bins) * sizeof(float2));
        return dispatch_fused<DIR_MOD>(p, fused_args(p, car_dev, out_dev, nullptr, n_sym, s), false, nt);
    }
    cf *frames = nullptr;
    rc = frames_of(p, n_sym, &frames); if (rc) return rc;
    const unsigned N = (unsigned)p->n_fft, K = (unsigned)p->n_bins;
    hipLaunchKernelGGL(ofdm_place_kernel, dim3(copy_grid(p->ctx, n_sym * N)), dim3(kBlock), 0, aeth::ctx_stream(p->ctx), (const cf *)car_dev,
                       (const int *)p->slot_dev, frames, n_sym, N, K);
    AETH_HIP(hipGetLastError());
    rc = aeth::fft_run(p->fft, (const float2 *)frames, (float2 *)frames, n_sym, AETH_SIGN_REF_BWD, s); if (rc) return rc;
    hipLaunchKernelGGL(ofdm_prefix_kernel, dim3(copy_grid(p->ctx, n_sym * L)), dim3(kBlock), 0, aeth::ctx_stream(p->ctx), (const cf *)frames,
                       (cf *)out_dev, n_sym, N, (unsigned)p->cp);
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

int aeth_ofdm_estimate(aeth_ofdm *p, const aeth_cf32 *y_dev, const aeth_cf32 *x_dev, size_t n_sym, size_t x_sym, float nv, int eq_kind,
                       aeth_cf32 *h_dev, aeth_cf32 *eq_dev, float *csi_dev)
{
    AETH_REQUIRE(p, AETH_E_ARG, "ofdm is null");
    AETH_REQUIRE(h_dev || eq_dev || csi_dev, AETH_E_ARG, "all three outputs are null");
    AETH_REQUIRE(eq_kind == AETH_OFDM_EQ_ZF || eq_kind == AETH_OFDM_EQ_MMSE || eq_kind == AETH_OFDM_EQ_MATCHED, AETH_E_ARG,
                 "bad equaliser kind %d", eq_kind);
    AETH_REQUIRE(n_sym >= 1, AETH_E_LEN, "an estimate from 0 training symbols");
    int rc = check_symbols(p, n_sym); if (rc) return rc;
    AETH_REQUIRE(x_sym == 1 || x_sym == n_sym, AETH_E_ARG, "x_sym %zu is neither 1 nor n_sym = %zu", x_sym, n_sym);
    AETH_REQUIRE(y_dev && x_dev, AETH_E_ARG, "null pointer");
    AETH_REQUIRE(aeth::aligned8(y_dev) && aeth::aligned8(x_dev) && aeth::aligned8(h_dev) && aeth::aligned8(eq_dev) &&
                 ((uintptr_t)csi_dev & 3u) == 0, AETH_E_ALIGN, "pointer not aligned (8 bytes; csi 4 bytes)");
    const size_t K = p->n_bins, ny = n_sym * K * sizeof(aeth_cf32), nx = x_sym * K * sizeof(aeth_cf32);
    const void *outs[3] = {h_dev, eq_dev, csi_dev};
    const size_t nout[3] = {K * sizeof(aeth_cf32), K * sizeof(aeth_cf32), K * sizeof(float)};
    for (int i = 0; i < 3; i++) {
        AETH_REQUIRE(!aeth::ranges_touch(outs[i], nout[i], y_dev, ny) && !aeth::ranges_touch(outs[i], nout[i], x_dev, nx), AETH_E_ARG,
                     "an output range overlaps the training symbols");
        for (int j = i + 1; j < 3; j++)
            AETH_REQUIRE(!aeth::ranges_touch(outs[i], nout[i], outs[j], nout[j]), AETH_E_ARG, "two output ranges overlap");
    }
    aeth::DeviceGuard dev_guard(p->ctx->device);
    hipLaunchKernelGGL(ofdm_estimate_kernel, dim3((unsigned)((K + kBlock - 1) / kBlock)), dim3(kBlock), 0, aeth::ctx_stream(p->ctx),
                       (const cf *)y_dev, (const cf *)x_dev, n_sym, x_sym == 1 ? 0 : 1, (unsigned)K, nv, eq_kind, (cf *)h_dev, (cf *)eq_dev,
                       csi_dev);
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

}  // extern "C"
