// aeth_fir.hip -- fused  FFT -> (* H) -> IFFT  kernel.
//
// The reference has no FIR (src/fir.rs:3-22 holds taps and an empty scratch, no
// filter method; README.md:95-96 lists it as TODO).  What it does have is the
// frequency-domain multiply chain
//     input.vec_rfft(&mut fft, s).vec_mul(&sig).vec_rifft(&mut fft, s)
// (benches/benches.rs:410-416).  Run over overlapping blocks that chain IS
// overlap-save convolution, so the FIR here is defined as exactly that:
//     block  = x[b*hop - ov .. b*hop - ov + N)            ov = N - hop >= ntaps-1
//     Y      = bwd( fwd(block) * fwd(taps || 0), Scale::N )
//     y[b*hop .. (b+1)*hop) = Y[ov .. N)
// with fwd/bwd the reference's transforms (+j / -j exponent, src/fft.rs:148,150).
//
// One kernel does the whole chain per block: HBM is touched once for the input
// window (8*N/hop B per output) and once for the output (8 B); the forward
// transform's last pass leaves the spectrum in exactly the register slots the
// inverse transform's first pass reads, so the multiply by H happens in registers
// with no exchange.  H and the twiddles live in registers across a persistent
// loop over blocks.  For windows of 512 samples and more hop is rounded down to a multiple of
// 64 samples so that every block's window and output start on a 512-byte boundary.
#include "aeth_internal.h"
#include "aeth_fft_core.h"
#include "aeth_fft_plan.h"
#include "aeth_fir_kernel.h"
#include "aeth_host.h"

#include <cstdlib>
#include <memory>
#include <new>
#include <type_traits>
#include <vector>

using namespace aeth::fftk;


using namespace aeth::firk;

namespace {

// the fused kernel has store variants (demodulating, decimating, level, peak) for these lengths, one block per workgroup
constexpr bool fused_store_len(size_t n) { return 1024 <= n && n <= 4096; }

// The one place a build of fmi_kernel is launched: the streaming (non-temporal) or the cached build by `nt`, then the
// launch's status.  ONLY_NT: the variant ships as a streaming build alone and the caller has decided for it.
template <class C, bool SCALED, int MINW, bool CHIRP, int VAR, bool ONLY_NT = false>
int fmi_go(bool nt, int grid, hipStream_t stream, const FmiArgs &b)
{
    if (ONLY_NT || nt) hipLaunchKernelGGL((fmi_kernel<C, SCALED, MINW, true, CHIRP, VAR>), dim3(grid), dim3(C::WG), 0, stream, b);
    else if constexpr (!ONLY_NT) hipLaunchKernelGGL((fmi_kernel<C, SCALED, MINW, false, CHIRP, VAR>), dim3(grid), dim3(C::WG), 0, stream, b);
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

template <class C, bool SCALED>
int launch_fmi(aeth_ctx *ctx, const FmiArgs &a, hipStream_t stream)
{
    long long ngroups = (a.nblocks + C::F - 1) / C::F;
    // persistent grid = what is resident at once: the kernel's ~230 VGPRs allow 2 waves per SIMD, 8 per CU
    constexpr int kWavesPerCu = 8;
    long long cap = (long long)ctx->num_cus * kWavesPerCu / (C::WG / 64);
    // A launch that runs BESIDE its predecessor on the overlap lane takes three of the four 128-lane workgroups a CU
    // holds: a full grid keeps every wave slot until its last round, so its successor could only overlap that tail;
    // with a slot per CU free the two run side by side from the start.  tools/fir_lab, two queues, grids 704 ... 800
    // of 1024: 46.6 us per launch against 47.5; through the library, alternating in one process
    // (tools/overlap_grid_ab.py, 25 rounds): regions of 20 launches -1.8 %, of 200 launches -1.4 %.  A launch on its own
    // (one queue, or the first of a chain) keeps the full grid: 53.5 us against 54.4.
    // Tuning (sixteenths of the resident grid): AETH_FIR_GRID_CHAINED for a launch beside its predecessor,
    // AETH_FIR_GRID_FIRST for the first launch of a chain / a lone launch on a context with the lane on.
    if (ctx->overlap && !ctx->stream_shared && C::WG == 128) {
        const int num = ctx->last_chained ? aeth::tuning_int("AETH_FIR_GRID_CHAINED", 12) : aeth::tuning_int("AETH_FIR_GRID_FIRST", 16);
        if (num > 0 && num != 16) cap = cap * num / 16;      // above 16: more workgroups than fit at once (they queue for slots)
    }
    int grid = (int)(ngroups < cap ? ngroups : cap);
    if (grid < 1) grid = 1;
    FmiArgs b = a;
    if (b.frame_n == 0) b.frame_n = C::N;
    const bool nt = aeth::streams_past_cache(2 * (size_t)a.n * sizeof(float2));
    if constexpr (SCALED) {
        if (b.chirp) return fmi_go<C, true, 1, true, 0>(nt, grid, stream, b);   // chirp-z frames always carry a scale factor
    }
    // one-frame workgroups run their LDS exchanges at raised wave priority (V_PRIO: -0.3 ... -0.5 us per 16 Mi-sample
    // launch in tools/fir_lab, A/B in one process); the other variants tried measured null or negative and are
    // gone from the code: profiles/r02_fir_lab_variants.txt, r03_fir_lab_variants.txt, r04_fir_lab_dma.txt, DESIGN 4.1
    // ... and N = 2048 (the configuration it was measured on) keeps its exchange image XOR-swizzled instead of padded:
    // no two-way conflict on the contiguous reads, transform-only time 39.8 -> 34.8 us, launch 54.8 -> 53.4 us
    constexpr int VAR = (C::F == 1) ? (V_PRIO | ((C::N == 2048 && C::P == 16) ? V_XOR : 0)) : 0;
    // the demodulating and decimating stores are built for the lengths the host routes to them, 1024 ... 4096
    // (aeth_fft_mul_ifft_demod, aeth_fir_exec_decim); no other length carries a build of either
    constexpr bool kStoreVariants = C::F == 1 && fused_store_len(C::N);
    if constexpr (!kStoreVariants) {
        if (b.bits || b.dec.d > 1)
            return aeth::set_error(AETH_E_UNSUPPORTED, "fused FFT*H*IFFT: no demodulating / decimating build of length %d", C::N);
    }
    if constexpr (kStoreVariants) {
        if (b.bits) {                                       // hard demodulation instead of the sample store
            // the decision's mode is a template parameter (aeth_fir_kernel.h: demod_block): BPSK, QPSK with a
            // separable table, QPSK with any other table -- nothing about it is tested per sample
            auto demod = [&](auto dmv) {
                constexpr int DV = VAR | V_DEMOD | decltype(dmv)::value;
                return fmi_go<C, SCALED, 1, false, DV>(nt, grid, stream, b);
            };
            if (b.bps == 1) return demod(std::integral_constant<int, V_DM_BPSK>());
            if (b.demod_sep) return demod(std::integral_constant<int, 0>());
            return demod(std::integral_constant<int, V_DM_QGEN>());
        }
    }
    if constexpr (kStoreVariants && !SCALED) {
        if (b.dec.d > 1) {                                  // decimating store (aeth_fir_exec_decim)
            // without the swizzle: with it the N = 2048 build needs 260 VGPRs and drops to one wave per SIMD (62 us
            // per 16 Mi-sample launch against 50)
            constexpr int DV = (VAR & ~V_XOR) | V_DECIM;
            return fmi_go<C, false, 2, false, DV>(nt, grid, stream, b);
        }
    }
    if constexpr (!(kStoreVariants && !SCALED)) {
        if (b.levels || b.parts)
            return aeth::set_error(AETH_E_UNSUPPORTED, "fused FFT*H*IFFT: no level-storing / peak-finding build of length %d", C::N);
    }
    if constexpr (kStoreVariants && !SCALED) {
        if (b.levels || b.parts) {                          // correlator products (aeth_corr_exec_levels, aeth_corr_search)
            // what the launch moves: the stream once, and 4 bytes per sample or 16 per wave and block
            const bool cnt = aeth::streams_past_cache((size_t)a.n * (b.levels ? 12 : 8));
            // the transform of the plain build, swizzle included: the epilogues' own registers (f64 q, the logarithm of
            // the dB kinds) still fit -- N = 2048: 250 VGPRs for the peak and the norm, 255 for the dB kinds -- and
            // MINW = 2 holds every build to 256 (tests/test_corr_resources.py checks that none of them spills for it)
            if (b.parts) return fmi_go<C, false, 2, false, VAR | V_PEAK>(cnt, grid, stream, b);
            if (b.level_kind == AETH_LEVEL_NORM) return fmi_go<C, false, 2, false, VAR | V_LEVEL>(cnt, grid, stream, b);
            if (b.level_kind == AETH_LEVEL_DB) return fmi_go<C, false, 2, false, VAR | V_LEVEL | V_LV_DB>(cnt, grid, stream, b);
            return fmi_go<C, false, 2, false, VAR | V_LEVEL | V_LV_POWER_DB>(cnt, grid, stream, b);
        }
    }
    // A launch that runs on its own (one queue, or the head of a chain) issues the next window's loads in four
    // instalments between the passes of the forward transform instead of one burst (V_SPREAD): 54.25 -> 53.34 us per
    // 16 Mi-sample launch on one queue, bit-identical output; beside another launch the burst form wins (47.5 against
    // 47.8 us), so chained launches keep it (profiles/r03_fir_lab_variants.txt).  AETH_FIR_SPREAD=0/1 forces either.
    if constexpr (C::F == 1 && !SCALED && C::NPASS == 3) {
        const int sp = aeth::tuning_int("AETH_FIR_SPREAD", -1);
        const bool chained = ctx->overlap && !ctx->stream_shared && ctx->last_chained;
        if (nt && (sp < 0 ? !chained : sp != 0)) return fmi_go<C, false, 1, false, VAR | V_SPREAD, true>(nt, grid, stream, b);
    }
    return fmi_go<C, SCALED, 1, false, VAR>(nt, grid, stream, b);
}

int dispatch_fmi(aeth_ctx *ctx, size_t fft_len, const FmiArgs &a, hipStream_t stream = nullptr)
{
    if (!stream) stream = aeth::ctx_stream(ctx);
    aeth::DeviceGuard dev_guard(ctx->device);
    const bool scaled = a.chirp != nullptr || !(a.s_fwd == 1.0f && a.s_bwd == 1.0f);
#define AETH_BODY(NN)                                                            \
    return scaled ? launch_fmi<typename CfgFor<NN>::type, true>(ctx, a, stream)  \
                  : launch_fmi<typename CfgFor<NN>::type, false>(ctx, a, stream)
    AETH_POW2_SWITCH(fft_len, AETH_BODY, return aeth::set_error(AETH_E_UNSUPPORTED, "fused FFT*H*IFFT: length %zu", fft_len))
#undef AETH_BODY
}

bool is_pow2(size_t n) { return n && (n & (n - 1)) == 0; }

// [a, a + na) and [b, b + nb) share a sample?
bool touch(const aeth_cf32 *a, size_t na, const aeth_cf32 *b, size_t nb)
{
    return aeth::ranges_touch(a, na * sizeof(aeth_cf32), b, nb * sizeof(aeth_cf32));
}

// ---- aeth_corr_search: from the waves' records to the per-block records and the best of the stream -------------------
// one candidate with a GLOBAL output index; also the record a workgroup of corr_fold_kernel leaves (24 bytes)
struct PeakBest {
    double q;                         // -1: no candidate (q >= 0 for every candidate)
    unsigned long long idx, nnan;
};
constexpr unsigned long long kNoIdx = ~0ull;
constexpr int kFoldBlock = 256;

// a (+) b in place -- larger q, or equal q and lower index: associative and commutative, so no order of combination
// changes the result
__device__ __forceinline__ void best_take(double &q, unsigned long long &idx, unsigned long long &nnan, double oq,
                                          unsigned long long oidx, unsigned long long onnan)
{
    const bool take = oq > q || (oq == q && oidx < idx);
    q = take ? oq : q; idx = take ? oidx : idx; nnan += onnan;
}

// the workgroup's 256 candidates -> one, valid in thread 0
// (not aeth_reduce.h's block_reduce: held as a record, the candidate costs both corr kernels private memory)
__device__ __forceinline__ void best_block_reduce(double &q, unsigned long long &idx, unsigned long long &nnan, double *lq,
                                                  unsigned long long *li, unsigned long long *ln)
{
#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) {
        const double oq = __shfl_xor(q, mask);
        const unsigned long long oi = __shfl_xor(idx, mask), on = __shfl_xor(nnan, mask);
        best_take(q, idx, nnan, oq, oi, on);
    }
    const unsigned wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0) { lq[wv] = q; li[wv] = idx; ln[wv] = nnan; }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kFoldBlock / 64; w++) best_take(q, idx, nnan, lq[w], li[w], ln[w]);
    }
}

// the public record: no candidate -> index n, norm NaN; n_nan saturates at UINT32_MAX
__device__ __forceinline__ void peak_record(aeth_corr_peak *out, double q, unsigned long long idx, unsigned long long nnan, size_t n)
{
    out->index = idx == kNoIdx ? n : (size_t)idx;
    out->norm = idx == kNoIdx ? __builtin_nanf("") : aeth::level_norm_of_q(q);
    out->n_nan = nnan > 0xffffffffull ? 0xffffffffu : (unsigned)nnan;
}

// thread = one overlap-save block: its waves' records -> its public record (when asked for), then the workgroup's best
__global__ __launch_bounds__(kFoldBlock) void corr_fold_kernel(const PeakPart *__restrict__ parts, long long nblocks, int waves,
                                                               int hop, int ov, size_t n, aeth_corr_peak *__restrict__ peaks,
                                                               PeakBest *__restrict__ wg_out)
{
    __shared__ double lq[kFoldBlock / 64];
    __shared__ unsigned long long li[kFoldBlock / 64], ln[kFoldBlock / 64];
    const long long b = (long long)blockIdx.x * kFoldBlock + threadIdx.x;
    double q = -1.0;
    unsigned long long idx = kNoIdx, nnan = 0;
    if (b < nblocks) {
        for (int w = 0; w < waves; w++) {
            const PeakPart *p = parts + b * waves + w;
            const unsigned e = p->e;
            best_take(q, idx, nnan, p->q, e == kPeakNone ? kNoIdx : (unsigned long long)(b * hop - ov + (long long)e), p->nnan);
        }
        if (peaks) peak_record(peaks + b, q, idx, nnan, n);
    }
    best_block_reduce(q, idx, nnan, lq, li, ln);
    if (threadIdx.x == 0) { wg_out[blockIdx.x].q = q; wg_out[blockIdx.x].idx = idx; wg_out[blockIdx.x].nnan = nnan; }
}

// ONE workgroup: the workgroups' records -> the record of the whole stream
__global__ __launch_bounds__(kFoldBlock) void corr_best_kernel(const PeakBest *__restrict__ in, size_t nrec, size_t n,
                                                               aeth_corr_peak *__restrict__ out)
{
    __shared__ double lq[kFoldBlock / 64];
    __shared__ unsigned long long li[kFoldBlock / 64], ln[kFoldBlock / 64];
    double q = -1.0;
    unsigned long long idx = kNoIdx, nnan = 0;
    for (size_t r = threadIdx.x; r < nrec; r += kFoldBlock) best_take(q, idx, nnan, in[r].q, in[r].idx, in[r].nnan);
    best_block_reduce(q, idx, nnan, lq, li, ln);
    if (threadIdx.x == 0) peak_record(out, q, idx, nnan, n);
}

const char kMsgFirInPlace[] = "FIR cannot run in place: the output range overlaps the input (or its history)";
const char kMsgFirAlign[] = "pointer not 8-byte aligned";

// what aeth_fir_exec, aeth_fir_exec_decim and aeth_corr_exec ask of their buffers (`out` holds n_out samples)
int fir_check(const aeth_fir *f, const aeth_cf32 *hist, const aeth_cf32 *in, size_t n, const aeth_cf32 *out, size_t n_out)
{
    AETH_REQUIRE(in && out, AETH_E_ARG, "null pointer");
    // blocks run concurrently and their windows reach into the neighbours' outputs: ANY overlap of the output range
    // with the input or the history reads samples that were already overwritten (out = in + 100 as much as out = in)
    AETH_REQUIRE(!touch(out, n_out, in, n) && !touch(out, n_out, hist, f->ntaps - 1), AETH_E_ARG, "%s", kMsgFirInPlace);
    AETH_REQUIRE(aeth::aligned8(in) && aeth::aligned8(out) && aeth::aligned8(hist), AETH_E_ALIGN, "%s", kMsgFirAlign);
    return AETH_OK;
}

// overlap-save over a stream of n samples; the products add their own fields (dec / n_out, levels, parts)
FmiArgs fir_args(const aeth_fir *f, const aeth_cf32 *hist, const aeth_cf32 *in, size_t n, aeth_cf32 *out)
{
    FmiArgs a;
    a.in = (const cf *)in; a.out = (cf *)out; a.hist = (const cf *)hist; a.Hf = (const cf *)f->Hf;
    a.twN = (const cf *)f->fft->tw_dev; a.twL = (const cf *)f->fft->tw_lane_dev;
    a.n = (long long)n; a.hop = (int)f->hop; a.ov = (int)(f->fft_len - f->hop); a.nhist = (int)(f->ntaps - 1);
    a.nblocks = (long long)((n + f->hop - 1) / f->hop);
    a.s_fwd = 1.0f; a.s_bwd = 1.0f;
    return a;
}

// `batch` frames of the plan's length, each a block of its own (no overlap, no history)
FmiArgs frame_args(const aeth_fft *plan, const void *in, void *out, const void *Hf, size_t n_total, size_t batch, float s_fwd,
                   float s_bwd)
{
    FmiArgs a;
    a.in = (const cf *)in; a.out = (cf *)out; a.hist = nullptr; a.Hf = (const cf *)Hf;
    a.twN = (const cf *)plan->tw_dev; a.twL = (const cf *)plan->tw_lane_dev;
    a.n = (long long)n_total; a.nblocks = (long long)batch;
    a.hop = (int)plan->len; a.ov = 0; a.nhist = 0;
    a.s_fwd = s_fwd; a.s_bwd = s_bwd;
    return a;
}

}  // namespace

namespace aeth {

// Chirp-z transform of `batch` frames of n samples in ONE launch: x*chirp -> fwd_M -> *filt -> bwd_M -> *chirp,
// zero-padded to M = sub->len in registers (aeth_fft_big.hip: fft_run_bluestein, M <= 4096).
int fmi_bluestein(aeth_fft *sub, const float2 *in, float2 *out, size_t n, size_t batch, const float2 *chirp,
                  const float2 *filt, int conj, float scale)
{
    FmiArgs a = frame_args(sub, in, out, filt, n * batch, batch, 1.0f, scale);
    a.hop = (int)n;                                          // frames of n samples, zero-padded to the plan's length
    a.chirp = (const cf *)chirp; a.frame_n = (int)n; a.conj = conj;
    return dispatch_fmi(sub->ctx, sub->len, a);
}

int fir_exec_on(aeth_fir *f, hipStream_t stream, const aeth_cf32 *hist, const aeth_cf32 *in, size_t n, aeth_cf32 *out)
{
    return dispatch_fmi(f->ctx, f->fft_len, fir_args(f, hist, in, n, out), stream);
}

}  // namespace aeth

extern "C" {

/* benches/benches.rs:410-416, per frame, in place */
int aeth_fft_mul_ifft(aeth_fft *plan, aeth_cf32 *frames, size_t n_total, size_t batch, const aeth_cf32 *sig,
                      size_t n_sig, int kind_fwd, float x_fwd, int kind_bwd, float x_bwd)
{
    AETH_REQUIRE(plan, AETH_E_ARG, "plan is null");
    AETH_REQUIRE(n_total == batch * plan->len, AETH_E_LEN, AETH_MSG_FFT_LEN);      /* fft.rs:185-189 */
    AETH_REQUIRE(n_sig == plan->len, AETH_E_LEN, AETH_MSG_VEC_LEN);                 /* vecops.rs:100-104 */
    AETH_REQUIRE(kind_fwd >= 0 && kind_fwd <= 3 && kind_bwd >= 0 && kind_bwd <= 3, AETH_E_ARG, "bad scale kind");
    if (batch == 0) return AETH_OK;
    AETH_REQUIRE(frames && sig, AETH_E_ARG, "null pointer");
    AETH_REQUIRE(aeth::aligned8(frames) && aeth::aligned8(sig), AETH_E_ALIGN, "%s", kMsgFirAlign);
    if (plan->algo != aeth::FFT_ALGO_POW2 || plan->len > 4096) {
        // generic lengths (and the 8192-point frame, too wide for the fused kernel's registers): the three trait calls, unfused
        int rc = aeth_fft_exec(plan, frames, n_total, frames, batch, AETH_SIGN_REF_FWD, kind_fwd, x_fwd);
        if (rc) return rc;
        rc = aeth_vec_mul_frames(plan->ctx, frames, plan->len, batch, sig, n_sig);    // one launch, sig shared by every frame
        if (rc) return rc;
        return aeth_fft_exec(plan, frames, n_total, frames, batch, AETH_SIGN_REF_BWD, kind_bwd, x_bwd);
    }
    return dispatch_fmi(plan->ctx, plan->len,
                        frame_args(plan, frames, frames, sig, n_total, batch, aeth_scale_factor(kind_fwd, plan->len, x_fwd),
                                   aeth_scale_factor(kind_bwd, plan->len, x_bwd)));
}

/* frames.vec_rfft(fft, s).vec_mul(&sig).vec_rifft(fft, s) per frame (benches/benches.rs:410-416), then
 * Modulation::demod_naive on the result (examples/modem.rs:28-31) -- BASELINE config 4's receive side.  For the
 * one-frame-per-workgroup lengths the correlator output is demodulated in registers and only the bit bytes are
 * written (8 B read + bits per sample instead of 8 R + 8 W + 8 R + bits); `frames` is not modified. */
int aeth_fft_mul_ifft_demod(aeth_fft *plan, const aeth_cf32 *frames, size_t n_total, size_t batch, const aeth_cf32 *sig,
                            size_t n_sig, int kind_fwd, float x_fwd, int kind_bwd, float x_bwd, int bps,
                            const aeth_cf32 *table, uint8_t *bits_out, size_t nbits_out, int compat)
{
    AETH_REQUIRE(plan, AETH_E_ARG, "plan is null");
    AETH_REQUIRE(n_total == batch * plan->len, AETH_E_LEN, AETH_MSG_FFT_LEN);
    AETH_REQUIRE(n_sig == plan->len, AETH_E_LEN, AETH_MSG_VEC_LEN);
    AETH_REQUIRE(kind_fwd >= 0 && kind_fwd <= 3 && kind_bwd >= 0 && kind_bwd <= 3, AETH_E_ARG, "bad scale kind");
    AETH_REQUIRE(bps == 1 || bps == 2, AETH_E_UNSUPPORTED, "bits_per_symbol %d: BPSK (1) or QPSK (2)", bps);
    AETH_REQUIRE(nbits_out == n_total * (size_t)bps, AETH_E_LEN, "output holds %zu bits, input gives %zu", nbits_out, n_total * (size_t)bps);
    if (batch == 0) return AETH_OK;
    AETH_REQUIRE(frames && sig && bits_out, AETH_E_ARG, "null pointer");
    AETH_REQUIRE(aeth::aligned8(frames) && aeth::aligned8(sig) && ((uintptr_t)bits_out % (size_t)bps) == 0, AETH_E_ALIGN, "pointer alignment");
    static const aeth_cf32 kB[2] = {{1.f, 1.f}, {-1.f, -1.f}};                              /* modulation.rs:77 */
    static const aeth_cf32 kQ[4] = {{1.f, 1.f}, {-1.f, 1.f}, {1.f, -1.f}, {-1.f, -1.f}};    /* modulation.rs:87-92 */
    const aeth_cf32 *tb = table ? table : (bps == 1 ? kB : kQ);
    if (plan->algo != aeth::FFT_ALGO_POW2 || !fused_store_len(plan->len)) {
        // other lengths: the chain on a copy in the plan's temp, then the stand-alone demodulator
        int rc = aeth::fft_ensure_tmp(plan, n_total); if (rc) return rc;
        rc = aeth_copy_dev(plan->ctx, plan->tmp_dev, frames, n_total * sizeof(float2)); if (rc) return rc;
        rc = aeth_fft_mul_ifft(plan, (aeth_cf32 *)plan->tmp_dev, n_total, batch, sig, n_sig, kind_fwd, x_fwd, kind_bwd, x_bwd);
        if (rc) return rc;
        return aeth_demod_naive(plan->ctx, (const aeth_cf32 *)plan->tmp_dev, n_total, bps, table, bits_out, nbits_out, compat);
    }
    FmiArgs a = frame_args(plan, frames, nullptr, sig, n_total, batch, aeth_scale_factor(kind_fwd, plan->len, x_fwd),
                           aeth_scale_factor(kind_bwd, plan->len, x_bwd));
    a.bits = bits_out; a.bps = bps; a.demod_compat = compat;
    for (int i = 0; i < (bps == 1 ? 2 : 4); i++) { cf t = {tb[i].re, tb[i].im}; a.tab[i] = t; }
    // demod_naive scans 2 * bps candidates (modulation.rs:135): all four for QPSK
    a.demod_sep = bps == 2 && tb[0].re == tb[2].re && tb[1].re == tb[3].re && tb[0].im == tb[1].im && tb[2].im == tb[3].im;
    // out of place (frames are only read), so consecutive calls on disjoint buffers can run on the context's two
    // queues like consecutive aeth_fir_exec calls do (aeth_ctx_set_overlap): the drain of one beside the fill of the next.
    // The reference signal is read by every workgroup until the launch ends, so it is an input like the frames.
    aeth::lanes::Access acc;
    acc.in[0] = aeth::lanes::range_of(frames, n_total * sizeof(aeth_cf32));
    acc.in[1] = aeth::lanes::range_of(sig, n_sig * sizeof(aeth_cf32));
    acc.out = aeth::lanes::range_of(bits_out, nbits_out);
    hipStream_t lane = aeth::ctx_fir_lane(plan->ctx, acc);
    return dispatch_fmi(plan->ctx, plan->len, a, lane);
}

int aeth_fir_create(aeth_ctx *ctx, const aeth_cf32 *taps, size_t ntaps, size_t fft_len, aeth_fir **out)
{
    AETH_REQUIRE(ctx && out, AETH_E_ARG, "null argument");
    *out = nullptr;
    AETH_REQUIRE(taps && ntaps >= 1, AETH_E_ARG, "need at least one tap");
    AETH_REQUIRE(is_pow2(fft_len) && fft_len >= 2 && fft_len <= 4096, AETH_E_UNSUPPORTED,
                 "fft_len %zu: need a power of two in [2, 4096]", fft_len);
    AETH_REQUIRE(2 * ntaps <= fft_len, AETH_E_ARG, "fft_len %zu < 2*ntaps (%zu)", fft_len, 2 * ntaps);
    aeth::DeviceGuard g(ctx->device);
    aeth_fir *f = new (std::nothrow) aeth_fir();
    AETH_REQUIRE(f, AETH_E_NOMEM, "out of host memory");
    f->ctx = ctx; f->ntaps = ntaps; f->fft_len = fft_len;
    // outputs per block: the one-frame-per-workgroup lengths round it down to 64 samples so that every
    // window and output block starts on a 512-byte boundary (descriptor loads, full lines); the short
    // windows, several to a workgroup, are bound by the block count and keep every output they can
    // (measured: fft_len 64, 8 taps: hop 57 -> 170 GS/s, hop 48 -> 155 GS/s)
    size_t L = fft_len - ntaps + 1;
    f->hop = (fft_len >= 512 && L >= 64) ? (L / 64) * 64 : L;
    int rc = aeth_fft_create(ctx, fft_len, 1, &f->fft);
    if (rc == AETH_OK) {
        hipError_t e = hipMalloc((void **)&f->Hf, fft_len * sizeof(float2));
        if (e != hipSuccess) rc = aeth::hip_fail(e, "hipMalloc");
    }
    if (rc == AETH_OK) {
        std::vector<aeth_cf32> padded(fft_len, aeth_cf32{0.f, 0.f});
        for (size_t k = 0; k < ntaps; k++) padded[k] = taps[k];
        rc = aeth_upload(ctx, f->Hf, padded.data(), fft_len * sizeof(float2));
    }
    // H = fwd(taps || 0), then Scale::N folded in (x 1/N is exact for a power of two)
    if (rc == AETH_OK)
        rc = aeth_fft_exec(f->fft, (aeth_cf32 *)f->Hf, fft_len, (aeth_cf32 *)f->Hf, 1, AETH_SIGN_REF_FWD,
                           AETH_SCALE_N, 0.f);
    if (rc == AETH_OK) rc = aeth_ctx_sync(ctx);
    if (rc != AETH_OK) { aeth_fir_destroy(f); return rc; }
    *out = f;
    return AETH_OK;
}

int aeth_fir_destroy(aeth_fir *f)
{
    if (!f) return AETH_OK;
    aeth::DeviceGuard g(f->ctx->device);
    (void)hipStreamSynchronize(aeth::ctx_stream(f->ctx));
    if (f->Hf) (void)hipFree(f->Hf);
    if (f->fft) aeth_fft_destroy(f->fft);
    delete f;
    return AETH_OK;
}

size_t aeth_fir_ntaps(const aeth_fir *f) { return f ? f->ntaps : 0; }
size_t aeth_fir_fft_len(const aeth_fir *f) { return f ? f->fft_len : 0; }
size_t aeth_fir_hop(const aeth_fir *f) { return f ? f->hop : 0; }

int aeth_fir_exec(aeth_fir *f, const aeth_cf32 *hist, const aeth_cf32 *in, size_t n, aeth_cf32 *out)
{
    AETH_REQUIRE(f, AETH_E_ARG, "fir is null");
    if (n == 0) return AETH_OK;
    if (int rc = fir_check(f, hist, in, n, out, n)) return rc;
    // independent consecutive launches alternate between the context's two queues (aeth_ctx_set_overlap); a history
    // buffer is usually the tail of something just written, so such calls stay on the in-order stream
    aeth::lanes::Access acc;
    acc.in[0] = aeth::lanes::range_of(in, n * sizeof(aeth_cf32));
    acc.out = aeth::lanes::range_of(out, n * sizeof(aeth_cf32));
    hipStream_t lane = hist ? aeth::ctx_stream(f->ctx) : aeth::ctx_fir_lane(f->ctx, acc);
    return aeth::fir_exec_on(f, lane, hist, in, n, out);
}

/* fir, then sampling::downsample(&y, &mut dst) (src/sampling.rs:28-42) in one pass: out[i] = y[i * dec],
 * dec = n / n_out; the filter's kernel simply does not store the samples downsample would skip */
int aeth_fir_exec_decim(aeth_fir *f, const aeth_cf32 *hist, const aeth_cf32 *in, size_t n, aeth_cf32 *out, size_t n_out)
{
    AETH_REQUIRE(f, AETH_E_ARG, "fir is null");
    if (n == 0 && n_out == 0) return AETH_OK;
    AETH_REQUIRE(n_out > 0 && n % n_out == 0, AETH_E_ARG, AETH_MSG_DECIM);          /* sampling.rs:32-36 */
    AETH_REQUIRE(n >= n_out, AETH_E_LEN, "downsample from an empty src (the reference panics: index out of bounds)");
    const size_t dec = n / n_out;
    if (dec == 1) return aeth_fir_exec(f, hist, in, n, out);
    if (int rc = fir_check(f, hist, in, n, out, n_out)) return rc;
    AETH_REQUIRE(fused_store_len(f->fft_len), AETH_E_UNSUPPORTED,
                 "decimating store: fft_len %zu (one-block-per-workgroup lengths 1024 .. 4096 only)", f->fft_len);
    AETH_REQUIRE(n < ((size_t)1 << 31), AETH_E_UNSUPPORTED, "decimating store: %zu samples (32-bit index arithmetic)", n);
    FmiArgs a = fir_args(f, hist, in, n, out);
    a.dec = aeth::make_fastdiv((uint32_t)dec); a.n_out = (long long)n_out;
    return dispatch_fmi(f->ctx, f->fft_len, a, aeth::ctx_stream(f->ctx));
}

int aeth_fir_exec_host(aeth_fir *f, const aeth_cf32 *hist, const aeth_cf32 *in, size_t n, aeth_cf32 *out)
{
    AETH_REQUIRE(f, AETH_E_ARG, "fir is null");
    if (n == 0) return AETH_OK;
    AETH_REQUIRE(in && out, AETH_E_ARG, "null pointer");
    aeth_ctx *ctx = f->ctx;
    aeth::DeviceGuard dev_guard(ctx->device);
    const size_t nh = f->ntaps - 1;
    const size_t bytes = n * sizeof(float2);
    int rc = aeth::ctx_stage(ctx, 0, (n + nh) * sizeof(float2)); if (rc) return rc;
    rc = aeth::ctx_stage(ctx, 1, bytes); if (rc) return rc;
    float2 *dh = (float2 *)ctx->stage[0].p;
    float2 *dout = (float2 *)ctx->stage[1].p;
    float2 *din = dh + nh;     // nh*8 bytes in: keeps 8-byte alignment
    if (hist && nh) AETH_HIP(hipMemcpyAsync(dh, hist, nh * sizeof(float2), hipMemcpyHostToDevice, aeth::ctx_stream(ctx)));
    AETH_HIP(hipMemcpyAsync(din, in, bytes, hipMemcpyHostToDevice, aeth::ctx_stream(ctx)));
    rc = aeth_fir_exec(f, hist ? (const aeth_cf32 *)dh : nullptr, (const aeth_cf32 *)din, n, (aeth_cf32 *)dout);
    if (rc) return rc;
    AETH_HIP(hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, aeth::ctx_stream(ctx)));
    AETH_HIP(hipStreamSynchronize(aeth::ctx_stream(ctx)));
    return AETH_OK;
}

}  // extern "C"

/* ---- correlator: "Add Correlation by Freq. Domain Convolution" (README.md:95; the chain of benches/benches.rs:394-416
 * run as overlap-save over a stream).  c[j] = sum_{k<M} conj(s[M-1-k]) * x[j-k] is aeth_fir_exec with the conj-reversed
 * template as taps, so the object is a filter and nothing else; the two fused products take the level / the peak of
 * every block in the kernel's registers (aeth_fir_kernel.h: level_block, peak_block). */
extern "C" {

int aeth_corr_create(aeth_ctx *ctx, const aeth_cf32 *ref, size_t nref, size_t fft_len, aeth_corr **out)
{
    AETH_REQUIRE(ctx && out, AETH_E_ARG, "null argument");
    *out = nullptr;
    AETH_REQUIRE(ref && nref >= 1, AETH_E_ARG, "need at least one template sample");
    AETH_REQUIRE(is_pow2(fft_len) && fft_len >= 2 && fft_len <= 4096, AETH_E_UNSUPPORTED,
                 "fft_len %zu: need a power of two in [2, 4096]", fft_len);
    AETH_REQUIRE(2 * nref <= fft_len, AETH_E_ARG, "fft_len %zu < 2*nref (%zu)", fft_len, 2 * nref);
    // the checks above are aeth_fir_create's, in the words of a template; nref <= 2048 from here on
    std::unique_ptr<aeth_cf32[]> taps(new (std::nothrow) aeth_cf32[nref]);
    aeth_corr *c = new (std::nothrow) aeth_corr();
    if (!taps || !c) delete c;
    AETH_REQUIRE(taps && c, AETH_E_NOMEM, "out of host memory");
    for (size_t k = 0; k < nref; k++) taps[k] = aeth_cf32{ref[nref - 1 - k].re, -ref[nref - 1 - k].im};
    const int rc = aeth_fir_create(ctx, taps.get(), nref, fft_len, &c->fir);
    if (rc != AETH_OK) { delete c; return rc; }
    *out = c;
    return AETH_OK;
}

int aeth_corr_destroy(aeth_corr *c)
{
    if (!c) return AETH_OK;
    const int rc = aeth_fir_destroy(c->fir);
    delete c;
    return rc;
}

size_t aeth_corr_nref(const aeth_corr *c) { return c ? aeth_fir_ntaps(c->fir) : 0; }
size_t aeth_corr_fft_len(const aeth_corr *c) { return c ? aeth_fir_fft_len(c->fir) : 0; }
size_t aeth_corr_hop(const aeth_corr *c) { return c ? aeth_fir_hop(c->fir) : 0; }

int aeth_corr_exec(aeth_corr *c, const aeth_cf32 *hist, const aeth_cf32 *in, size_t n, aeth_cf32 *out)
{
    AETH_REQUIRE(c && c->fir, AETH_E_ARG, "corr is null");
    if (n == 0) return AETH_OK;
    const aeth_fir *f = c->fir;
    if (int rc = fir_check(f, hist, in, n, out, n)) return rc;
    // always the in-order stream: a search usually follows on what was just written
    return aeth::fir_exec_on(c->fir, aeth::ctx_stream(f->ctx), hist, in, n, out);
}

int aeth_corr_exec_levels(aeth_corr *c, const aeth_cf32 *hist, const aeth_cf32 *in, size_t n, int kind, float *levels,
                          size_t n_levels)
{
    AETH_REQUIRE(c && c->fir, AETH_E_ARG, "corr is null");
    AETH_REQUIRE(aeth::level_kind_ok(kind), AETH_E_ARG, "bad level kind %d", kind);
    AETH_REQUIRE(n_levels == n, AETH_E_LEN, "Levels and samples must have same length");
    if (n == 0) return AETH_OK;
    const aeth_fir *f = c->fir;
    AETH_REQUIRE(in && levels, AETH_E_ARG, "null pointer");
    AETH_REQUIRE(aeth::aligned8(in) && aeth::aligned8(hist), AETH_E_ALIGN, "%s", kMsgFirAlign);
    AETH_REQUIRE((reinterpret_cast<uintptr_t>(levels) & 3u) == 0, AETH_E_ALIGN, "levels not 4-byte aligned");
    AETH_REQUIRE(!aeth::ranges_touch(levels, n * sizeof(float), in, n * sizeof(aeth_cf32)) &&
                 !aeth::ranges_touch(levels, n * sizeof(float), hist, (f->ntaps - 1) * sizeof(aeth_cf32)), AETH_E_ARG,
                 "levels overlaps the input (or its history)");
    AETH_REQUIRE(fused_store_len(f->fft_len), AETH_E_UNSUPPORTED,
                 "level store: fft_len %zu (one-block-per-workgroup lengths 1024 .. 4096 only)", f->fft_len);
    FmiArgs a = fir_args(f, hist, in, n, nullptr);
    a.levels = levels; a.level_kind = kind;
    return dispatch_fmi(f->ctx, f->fft_len, a, aeth::ctx_stream(f->ctx));
}

int aeth_corr_search(aeth_corr *c, const aeth_cf32 *hist, const aeth_cf32 *in, size_t n, struct aeth_corr_peak *peaks,
                     size_t n_peaks, struct aeth_corr_peak *best)
{
    AETH_REQUIRE(c && c->fir, AETH_E_ARG, "corr is null");
    AETH_REQUIRE(peaks || best, AETH_E_ARG, "peaks_dev and best_host are both null: nothing to report");
    AETH_REQUIRE(n != 0, AETH_E_LEN, "peak of an empty stream");
    const aeth_fir *f = c->fir;
    const size_t nblocks = (n + f->hop - 1) / f->hop;
    AETH_REQUIRE(!peaks || n_peaks == nblocks, AETH_E_LEN, "peaks holds %zu records, the stream has %zu blocks of %zu", n_peaks,
                 nblocks, f->hop);
    AETH_REQUIRE(in, AETH_E_ARG, "null pointer");
    AETH_REQUIRE(aeth::aligned8(in) && aeth::aligned8(hist) && aeth::aligned8(peaks), AETH_E_ALIGN, "%s", kMsgFirAlign);
    AETH_REQUIRE(!aeth::ranges_touch(peaks, nblocks * sizeof(aeth_corr_peak), in, n * sizeof(aeth_cf32)) &&
                 !aeth::ranges_touch(peaks, nblocks * sizeof(aeth_corr_peak), hist, (f->ntaps - 1) * sizeof(aeth_cf32)), AETH_E_ARG,
                 "peaks overlaps the input (or its history)");
    AETH_REQUIRE(fused_store_len(f->fft_len), AETH_E_UNSUPPORTED,
                 "peak search: fft_len %zu (one-block-per-workgroup lengths 1024 .. 4096 only)", f->fft_len);
    AETH_REQUIRE(nblocks < ((size_t)1 << 28), AETH_E_UNSUPPORTED, "peak search: %zu samples", n);
    aeth_ctx *ctx = f->ctx;
    aeth::DeviceGuard dev_guard(ctx->device);
    // slab: [one PeakPart per wave and block | one PeakBest per workgroup of the fold]
    const int waves = (int)(f->fft_len / 16 / 64);                              // 16 points per lane (aeth_fft_core.h: CfgFor)
    const size_t nwg = (nblocks + kFoldBlock - 1) / kFoldBlock;
    const size_t parts_bytes = nblocks * (size_t)waves * sizeof(PeakPart);
    int rc = aeth::scratch_ensure(ctx, ctx->corr_slab, parts_bytes + nwg * sizeof(PeakBest)); if (rc) return rc;
    PeakPart *parts = static_cast<PeakPart *>(ctx->corr_slab.p);
    PeakBest *wg = reinterpret_cast<PeakBest *>(static_cast<char *>(ctx->corr_slab.p) + parts_bytes);
    aeth::HostIO io;
    if (best) { rc = io.open(ctx, 0, sizeof(aeth_corr_peak)); if (rc) return rc; }   // the pinned bounce buffer
    hipStream_t s = aeth::ctx_stream(ctx);
    FmiArgs a = fir_args(f, hist, in, n, nullptr);
    a.parts = parts;
    rc = dispatch_fmi(ctx, f->fft_len, a, s); if (rc) return rc;
    hipLaunchKernelGGL(corr_fold_kernel, dim3((unsigned)nwg), dim3(kFoldBlock), 0, s, (const PeakPart *)parts, (long long)nblocks,
                       waves, a.hop, a.ov, n, peaks, wg);
    if (best)
        hipLaunchKernelGGL(corr_best_kernel, dim3(1), dim3(kFoldBlock), 0, s, (const PeakBest *)wg, nwg, n,
                           static_cast<aeth_corr_peak *>(io.buf[1]));
    AETH_HIP(hipGetLastError());
    if (best) return io.get(best, 1, sizeof(aeth_corr_peak));
    return AETH_OK;
}

}  // extern "C"
