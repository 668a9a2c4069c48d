// aeth_fir_kernel.h -- device side of the fused  FFT -> (* H) -> IFFT  kernel (aeth_fir.hip holds the host side
// and the reference citations; tools/fir_lab.hip instantiates the same template for A/B measurements).
//
// One 128-lane workgroup per overlap-save block (N = 2048: 16 points per lane), persistent loop over blocks,
// the next block's window prefetched into registers while the current one is transformed.  Every build of
// fmi_kernel that this header allows is one libaether_hip.so launches or tools/fir_lab.hip measures; the block's
// results leave as samples (store_block), bit bytes (demod_block), levels (level_block) or one peak record per wave
// (peak_block).
#pragma once

#include "aeth_internal.h"
#include "aeth_fft_core.h"
#include "aeth_levels.h"

namespace aeth {
namespace firk {

using namespace aeth::fftk;

// V_PEAK: what one wave knows about its share of one block's outputs (16 bytes, one store).  q is -1 and e is
// kPeakNone when the wave saw no candidate.
struct __attribute__((aligned(16))) PeakPart {
    double q;             // largest q(c) (aeth_levels.h) among the wave's samples without a NaN component
    unsigned e;           // window element of the first sample that has it
    unsigned nnan;        // samples with a NaN component
};
static_assert(sizeof(PeakPart) == 16, "one 16-byte store per wave and block");
constexpr unsigned kPeakNone = 0x7fffffffu;

struct FmiArgs {
    const cf *in;
    cf *out;
    const cf *hist;       // ntaps-1 samples preceding in[0], or null
    const cf *Hf;         // N spectrum multipliers, natural order
    const cf *twN;
    const cf *twL;        // per-lane twiddle table of the plan (null: gather from twN)
    long long n;          // samples in `in` / outputs wanted
    long long nblocks;
    int hop, ov, nhist;
    float s_fwd, s_bwd;
    // chirp-z (Bluestein) mode: a block is one frame of frame_n < N samples, multiplied by chirp[e] on the way in
    // and on the way out, zero beyond frame_n; conj = transform with the other exponent sign
    const cf *chirp = nullptr;
    int frame_n = 0;      // valid samples per window (0: the whole window)
    int conj = 0;
    // V_DECIM: only every dec-th output sample is stored, out[i] = y[i * dec] (fir -> sampling::downsample in one pass)
    aeth::FastDiv dec = {1, 0, 0, 0};
    long long n_out = 0;  // samples in `out` = n / dec
    // V_DEMOD: the chain's output goes through Modulation::demod_naive instead of to memory (hard decisions only)
    unsigned char *bits = nullptr;    // n * bps bytes, one per bit
    cf tab[4] = {};                   // BPSK / QPSK symbol table
    int bps = 0, demod_compat = 0;
    int demod_sep = 0;                // host side only: picks the kernel build (DM_QSEP / DM_QGEN, see demod_block)
    // V_LEVEL: levels[o] = level of output sample o instead of the sample (aeth_corr_exec_levels)
    float *levels = nullptr;
    int level_kind = 0;               // host side only: picks the kernel build (V_LV_DB / V_LV_POWER_DB)
    // V_PEAK: nothing of the output is stored, every wave leaves one PeakPart per block at parts[blk * waves + wave]
    // (aeth_corr_search)
    PeakPart *parts = nullptr;
};

// Kernel variants (template parameter VAR, a bit set).  0 is the round-1 kernel.  The first three shape the transform
// and the prefetch, the others replace the sample store; launch_fmi (aeth_fir.hip) decides which launch takes which.
// The values are part of the mangled kernel names, which tests/test_corr_resources.py, tools/variant_coverage.py and
// tools/summarize_profile.py parse, so they stay as they are: the gaps are variants that were measured and removed
// (profiles/).
enum : int {
    V_PRIO   = 4,       // s_setprio 1 around every LDS exchange (its latency chain is what a block's time is made of)
    V_XOR    = 2048,    // XOR-swizzled LDS exchange image instead of the padded one (see aeth_fft_core.h: pidx)
    V_SPREAD = 16384,   // the next window's 16 loads issued in four groups between the passes of this block's forward
                        // transform instead of one burst in front of it (the TA command FIFO is full 40 % of the time)
    V_DECIM  = 512,     // decimating store (aeth_fir_exec_decim)
    V_DEMOD  = 1024,    // hard demodulation instead of the sample store (aeth_fft_mul_ifft_demod)
    V_DM_BPSK = 1 << 16, V_DM_QGEN = 1 << 17,     // with V_DEMOD: the decision's mode (neither: QPSK, separable table)
    V_LEVEL  = 1 << 19, // a 4-byte level of every output sample instead of the sample (aeth_corr_exec_levels)
    V_LV_DB = 1 << 20, V_LV_POWER_DB = 1 << 21,   // with V_LEVEL: the level kind (neither: AETH_LEVEL_NORM)
    V_PEAK   = 1 << 22, // the block's largest |c|^2 instead of any store (aeth_corr_search)
};
constexpr int V_ALL = V_PRIO | V_XOR | V_SPREAD | V_DECIM | V_DEMOD | V_DM_BPSK | V_DM_QGEN | V_LEVEL | V_LV_DB | V_LV_POWER_DB |
                      V_PEAK;

// cache-policy bits of the streamed accesses (aux operand of the buffer instructions: 1 = sc0, 2 = nt, 16 = sc1):
// loads nt, stores nt + sc1.  Chosen by an element-wise copy at first (tools/nt_modes.hip), since measured in the kernel
// itself, 8-byte accesses, persistent workgroups, two launches in flight (tools/fir_lab.hip, profiles/fir_policy_lab.txt;
// per cent of the launch time against these values): loads plain or sc1 +3.3 ... +3.7, nt + sc1 the same as nt; stores
// nt alone +0.1 ... +0.5 (one queue: +0.9 ... +1.3), sc1 alone +3.3 ... +6.2, plain +5.2 ... +8.2.
constexpr int kLoadAux = 2, kStoreAux = 18;
// ... except some slots of a window, which are loaded plain (0) instead of nt.  That began as the window's halo -- the
// last ov samples of a window are the first ov of its right neighbour's, read by a workgroup on another XCD in the same
// round -- in slot 0 and slot P-1: +3.2 % on the headline (profiles/fir_head_bench.txt).  The lab says the sharing is not
// what pays: plain on two slots nobody shares (7 and 8) gains the same, on one of the halo slots half of it, on only the
// shared HALF of each halo slot (a wave-uniform branch around the load) nothing.  What counts is the share of a window's
// loads that go without the hint, wherever they sit: 1 / 2 / 3 / 4 / 5 / 6 / 8 / 16 of 16 slots give +1.8 / 0 / -1.5 /
// -2.0 ... -2.6 / -2.3 ... -2.7 / -1.5 / +3.1 / +3.5 % of the launch time against two (one queue: the same curve, -2.1
// at four).  sc1 (16) and sc0 (1) on these slots: the same as plain to 0.4 %.
constexpr int kHaloAux = 0;
// The slots that take kHaloAux, bit m = slot m: the first and the last, and at N = 2048 with 16 slots (the configuration
// the table was measured on, as V_XOR) the two at either end: a quarter of the window, and exactly the halo of the longest
// filters the plan takes (ov = 256).  Frames (ov = 0) go through the same builds with the same slots.
template <class C> constexpr unsigned plain_slots()
{
    return (C::N == 2048 && C::P == 16) ? 0xC003u : (1u | 1u << (C::P - 1));
}

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// Stream accesses carry the non-temporal hint (aux bit 1) when the launch moves more than the cache holds: a
// window is read once and an output block written once, so neither should displace the tables in L2 or take the
// write-allocate path (A/B in one process on 256 MiB: stores alone -3 %, loads alone +3 %, both -5 % of the launch
// time).  NT is a kernel template parameter: short chains over cache-sized operands (C4) keep plain accesses.

__device__ __forceinline__ cf as_cf(u32x2 v) { return __builtin_bit_cast(cf, v); }
__device__ __forceinline__ u32x2 as_u32x2(cf v) { return __builtin_bit_cast(u32x2, v); }

// What a build of the kernel does with those constants.  Every configuration the library launches takes this primary
// template, the shipped rule; tools/fir_lab.hip specialises it for configurations of its own (a Cfg with a LabPolicy
// member) to time other policies, halo rules and burst orders beside it in one process.  The policy hangs on C and not on
// a template parameter of its own because the mangled names of the library's builds are parsed (see VAR above).
template <class C, class = void>
struct StreamPolicy {
    static constexpr int store = kStoreAux;                 // the 8-byte sample stores of store_block
    static constexpr int slot(int i) { return i; }          // the i-th load of a window's burst fetches this slot
    // Slot m of a window through its descriptor.  The aux operand is an immediate, so which slots go without the hint
    // is a compile-time rule on m (plain_slots): no branch, one load per slot, and the policy is a hint only -- a slot on
    // either side of the rule returns the same bytes.
    template <bool NT, class RS>
    static __device__ __forceinline__ cf load(RS rs, int tid, int m)
    {
        const int off = (tid + m * C::T) * 8;
        if ((plain_slots<C>() >> m) & 1) return as_cf(__builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, NT ? kHaloAux : 0));
        return as_cf(__builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, NT ? kLoadAux : 0));
    }
};

// the i-th load of a window's burst: slot m = StreamPolicy<C>::slot(i) into its register
template <class C, bool NT, class RS>
__device__ __forceinline__ void load_slot(cf (&x)[C::P], RS rs, int tid, int i)
{
    const int m = StreamPolicy<C>::slot(i);
    x[m] = StreamPolicy<C>::template load<NT>(rs, tid, m);
}

// one block's input window -> registers (slot m = window element tid + m*T)
template <class C, bool NT>
__device__ __forceinline__ void load_window(cf (&x)[C::P], const FmiArgs &a, long long blk, int tid)
{
    const long long win0 = blk * a.hop - a.ov;              // first input sample of the window
    if (blk >= a.nblocks) {
#pragma unroll
        for (int m = 0; m < C::P; m++) x[m] = mk(0.f, 0.f);
        return;
    }
    if constexpr (C::F == 1) {
        if (win0 >= 0) {
            // wave-uniform window: buffer loads, the descriptor's range check zero-fills past the end
            long long left = a.n - win0;
            int bytes = (int)(left < a.frame_n ? left : a.frame_n) * 8;
            auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<cf *>(a.in + win0), 0, bytes, 0x00020000);
#pragma unroll
            for (int i = 0; i < C::P; i++)
                load_slot<C, NT>(x, rs, tid, i);
            // (the window's oldest ov-nhist samples are zeroed when the window is consumed: doing it
            // here would put a wait for the load right behind its issue)
            return;
        }
    }
    if constexpr (C::F > 1) {
        // several windows per workgroup: when the whole group lies inside the stream (workgroup-uniform test)
        // the loads need no per-element range logic, only the zeroing of the samples older than the history
        const long long first = (blk - (long long)(threadIdx.x / C::T)) * a.hop - a.ov;
        const long long last_end = first + (long long)(C::F - 1) * a.hop + C::N;
        if (a.frame_n == C::N && first >= 0 && last_end <= a.n && blk - (long long)(threadIdx.x / C::T) + C::F <= a.nblocks) {
#pragma unroll
            for (int m = 0; m < C::P; m++) {
                const cf v = a.in[win0 + tid + m * C::T];
                x[m] = (tid + m * C::T >= a.ov - a.nhist) ? v : mk(0.f, 0.f);
            }
            return;
        }
        if (a.frame_n < C::N && a.ov == 0 && blk - (long long)(threadIdx.x / C::T) + C::F <= a.nblocks) {
            // chirp-z frames (hop = frame_n samples each, zero beyond): every frame of the group exists
#pragma unroll
            for (int m = 0; m < C::P; m++) {
                const int e = tid + m * C::T;
                x[m] = e < a.frame_n ? a.in[win0 + e] : mk(0.f, 0.f);
            }
            return;
        }
    }
#pragma unroll
    for (int m = 0; m < C::P; m++) {
        const long long gi = win0 + tid + m * C::T;
        cf v = mk(0.f, 0.f);
        if (tid + m * C::T >= a.ov - a.nhist && tid + m * C::T < a.frame_n) {
            if (gi >= 0) { if (gi < a.n) v = a.in[gi]; }
            else if (a.hist && gi >= -(long long)a.nhist) v = a.hist[a.nhist + gi];
        }
        x[m] = v;
    }
}

// Branch-free form for the steady state of one-frame workgroups (win0 >= 0 guaranteed by
// the caller): a block past the end gets a zero-length descriptor, so the loads still
// issue -- and return zeros without touching memory.  No divergent path means hipcc can
// COUNT the loads in flight (vmcnt(N)) instead of falling back to vmcnt(0).
template <class C, bool NT>
__device__ __forceinline__ void load_window_srd(cf (&x)[C::P], const FmiArgs &a, long long blk, int tid)
{
    const bool active = blk < a.nblocks;
    const long long win0 = active ? blk * a.hop - a.ov : 0;
    long long left = a.n - win0;
    const int bytes = active ? (int)(left < a.frame_n ? left : a.frame_n) * 8 : 0;
    auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<cf *>(a.in + win0), 0, bytes, 0x00020000);
#pragma unroll
    for (int i = 0; i < C::P; i++)
        load_slot<C, NT>(x, rs, tid, i);
}

// the same, slots [M0, M1) only (V_SPREAD: the window arrives in four instalments)
template <class C, bool NT, int M0, int M1>
__device__ __forceinline__ void load_window_srd_part(cf (&x)[C::P], const FmiArgs &a, long long blk, int tid)
{
    const bool active = blk < a.nblocks;
    const long long win0 = active ? blk * a.hop - a.ov : 0;
    long long left = a.n - win0;
    const int bytes = active ? (int)(left < a.frame_n ? left : a.frame_n) * 8 : 0;
    auto rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<cf *>(a.in + win0), 0, bytes, 0x00020000);
#pragma unroll
    for (int i = M0; i < M1; i++)
        load_slot<C, NT>(x, rs, tid, i);
    __builtin_amdgcn_sched_barrier(0);
}

// Modulation::demod_naive on the block's output samples (modulation.rs:33-56 for [cf32; 4], :133-144 for [cf32; 2]):
// nearest table symbol by squared distance, d = rn(rn(dr*dr) + rn(di*di)) -- the products are rounded before the sum
// (packed multiplies and adds as asm statements: nothing for -ffp-contract=fast to fuse), so the decisions are those
// of aeth_demod_naive on the stored samples -- folded as the reference's min_by does: the running minimum is replaced
// by a strictly smaller distance and by an unordered pair (`v_cmp_nle`: !(best <= d)), equal distances keep the first.
//
// Same skeleton as store_block<CHECK = false>: no branch anywhere.  The mode (DM) is a template parameter, the bit
// bytes leave through a per-block buffer descriptor whose range check drops what must not be written (a block past
// the end: zero-length descriptor; samples in front of the valid part: offset out of range), so hipcc can count the
// memory operations in flight and the loop's only wait stays `vmcnt(16)`.
//   DM_BPSK  two candidates, one byte per sample
//   DM_QSEP  QPSK table of the form {(a,c), (b,c), (a,d), (b,d)} (the generic one is): the four distances are built
//            from four squares instead of eight -- six packed instructions per sample, bit for bit the values of DM_QGEN
//   DM_QGEN  any other four-entry table
enum : int { DM_BPSK = 1, DM_QSEP = 2, DM_QGEN = 3 };

// (a.x - t.x, a.x - t.y) / (a.y - t.x, a.y - t.y): one sample component against two table components (t wave-uniform)
__device__ __forceinline__ cf diff_re(cf a, cf t) { cf d; asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[0,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(a), "s"(t)); return d; }
__device__ __forceinline__ cf diff_im(cf a, cf t) { cf d; asm("v_pk_add_f32 %0, %1, %2 op_sel:[1,0] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(a), "s"(t)); return d; }
__device__ __forceinline__ cf pk_sq(cf a) { cf d; asm("v_pk_mul_f32 %0, %1, %1" : "=v"(d) : "v"(a)); return d; }
__device__ __forceinline__ cf pk_sum(cf a, cf b) { cf d; asm("v_pk_add_f32 %0, %1, %2" : "=v"(d) : "v"(a), "v"(b)); return d; }
// (a.x + b.x, a.y + b.x) and (a.x + b.y, a.y + b.y)
__device__ __forceinline__ cf pk_sum_lo(cf a, cf b) { cf d; asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,0] op_sel_hi:[1,0]" : "=v"(d) : "v"(a), "v"(b)); return d; }
__device__ __forceinline__ cf pk_sum_hi(cf a, cf b) { cf d; asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[1,1]" : "=v"(d) : "v"(a), "v"(b)); return d; }

// wave-uniform operands of the decision, built once per launch from the table in the kernel arguments
struct DemodK {
    cf x01, y01, x23, y23;      // (t0.x, t1.x), (t0.y, t1.y), (t2.x, t3.x), (t2.y, t3.y); DM_QSEP uses x01 and (t0.y, t2.y) in y01
    unsigned hi;                // what bit 1 of the index contributes to the stored pair of bytes: 0x100, or 0x200 for `idx & 2` (modulation.rs:54)
};

template <int DM>
__device__ __forceinline__ DemodK demod_consts(const FmiArgs &a)
{
    DemodK k;
    k.x01 = mk(a.tab[0].x, a.tab[1].x); k.y01 = mk(a.tab[0].y, DM == DM_QSEP ? a.tab[2].y : a.tab[1].y);
    k.x23 = mk(a.tab[2].x, a.tab[3].x); k.y23 = mk(a.tab[2].y, a.tab[3].y);
    k.hi = a.demod_compat ? 0x200u : 0x100u;
    return k;
}

// the bytes demod_naive emits for one sample: bit 0 of the index in byte 0, bit 1 (or idx & 2) in byte 1
template <int DM>
__device__ __forceinline__ unsigned demod_decide(cf v, const DemodK &k)
{
    if constexpr (DM == DM_BPSK) {
        const cf d = pk_sum(pk_sq(diff_re(v, k.x01)), pk_sq(diff_im(v, k.y01)));     // (d0, d1)
        return !(d.x <= d.y) ? 1u : 0u;
    } else {
        cf d01, d23;
        if constexpr (DM == DM_QSEP) {
            const cf px = pk_sq(diff_re(v, k.x01)), py = pk_sq(diff_im(v, k.y01));   // (px0, px1), (py0, py1)
            d01 = pk_sum_lo(px, py); d23 = pk_sum_hi(px, py);
        } else {
            d01 = pk_sum(pk_sq(diff_re(v, k.x01)), pk_sq(diff_im(v, k.y01)));
            d23 = pk_sum(pk_sq(diff_re(v, k.x23)), pk_sq(diff_im(v, k.y23)));
        }
        const bool c1 = !(d01.x <= d01.y);
        const float b1 = c1 ? d01.y : d01.x;
        const bool c2 = !(b1 <= d23.x);
        const float b2 = c2 ? d23.x : b1;
        const bool c3 = !(b2 <= d23.y);
        const bool bit0 = c3 | (c1 & !c2), bit1 = c3 | c2;                           // index = c3 ? 3 : c2 ? 2 : c1 ? 1 : 0
        return (bit0 ? 1u : 0u) | (bit1 ? k.hi : 0u);
    }
}

template <class C, bool SCALED, bool NT, int DM>
__device__ __forceinline__ void demod_block(const cf (&w)[C::P], const FmiArgs &a, const DemodK &k, long long blk, int tid)
{
    static_assert(C::F == 1, "demodulating store: one block per workgroup");
    constexpr int B = DM == DM_BPSK ? 1 : 2;                        // bytes per sample
    const long long base = blk * a.hop - a.ov;
    long long left = a.n - base;
    int bytes = (int)(left < a.frame_n ? left : a.frame_n) * B;
    if (blk >= a.nblocks) bytes = 0;
    auto rs = __builtin_amdgcn_make_buffer_rsrc(a.bits + base * B, 0, bytes, 0x00020000);
    const cf ss = mk(a.s_bwd, a.s_bwd);
#pragma unroll
    for (int m = 0; m < C::P; m++) {
        const int e = tid + m * C::T;
        const int off = (e >= a.ov) ? e * B : 0x7ffffff0;
        const cf v = SCALED ? cscale_k(w[m], ss) : w[m];
        const unsigned o = demod_decide<DM>(v, k);
        if constexpr (B == 1) __builtin_amdgcn_raw_buffer_store_b8((unsigned char)o, rs, off, 0, NT ? kStoreAux : 0);
        else __builtin_amdgcn_raw_buffer_store_b16((unsigned short)o, rs, off, 0, NT ? kStoreAux : 0);
    }
}

// The level of every output sample of the block instead of the sample (aeth_levels.h: the arithmetic of
// aeth_vec_levels, so the values are those of aeth_vec_levels on the stored samples).  Same skeleton as demod_block:
// a descriptor over the block's valid range, offsets past it for the window elements in front of the valid part, no
// branch anywhere.
template <class C, bool SCALED, bool NT, int KIND>
__device__ __forceinline__ void level_block(const cf (&w)[C::P], const FmiArgs &a, long long blk, int tid)
{
    static_assert(C::F == 1, "level store: one block per workgroup");
    const long long base = blk * a.hop - a.ov;
    long long left = a.n - base;
    int bytes = (int)(left < a.frame_n ? left : a.frame_n) * 4;
    if (blk >= a.nblocks) bytes = 0;
    auto rs = __builtin_amdgcn_make_buffer_rsrc(a.levels + base, 0, bytes, 0x00020000);
    const cf ss = mk(a.s_bwd, a.s_bwd);
#pragma unroll
    for (int m = 0; m < C::P; m++) {
        const int e = tid + m * C::T;
        const int off = (e >= a.ov) ? e * 4 : 0x7ffffff0;
        const cf v = SCALED ? cscale_k(w[m], ss) : w[m];
        __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, aeth::level_of<KIND>(v.x, v.y)), rs, off, 0,
                                              NT ? kStoreAux : 0);
    }
}

// The block's peak instead of any sample: the rule of aeth_vec_stats -- order by q (f64), the lowest index wins among
// equals, a sample with a NaN component is counted and is no candidate.  A lane walks its P elements in ascending
// index with a strict `>`, so it keeps the first of equals; lanes combine by "larger q, or equal q and lower index",
// which is associative and commutative: the xor butterfly leaves the same record in every lane of the wave, and the
// order in which corr_fold_kernel (aeth_fir.hip) combines the waves does not matter either.  One 16-byte record per
// wave leaves through a descriptor over the block's records (lanes other than 0: offset out of range; a block past the
// end: zero length) -- no workgroup barrier, no LDS, no atomics.
template <class C, bool SCALED, bool NT>
__device__ __forceinline__ void peak_block(const cf (&w)[C::P], const FmiArgs &a, long long blk, int tid)
{
    static_assert(C::F == 1 && C::WG % 64 == 0, "peak search: one block per workgroup, whole waves");
    constexpr int WAVES = C::WG / 64;
    const long long base = blk * a.hop - a.ov;
    long long left = a.n - base;
    const int lim = (int)(left < a.frame_n ? left : a.frame_n);        // window elements at and past it are no outputs
    const cf ss = mk(a.s_bwd, a.s_bwd);
    double bq = -1.0;                                                   // q >= 0 for every candidate
    unsigned be = kPeakNone, nn = 0;
#pragma unroll
    for (int m = 0; m < C::P; m++) {
        const int e = tid + m * C::T;
        const cf v = SCALED ? cscale_k(w[m], ss) : w[m];
        const double q = aeth::level_q(v.x, v.y);
        const bool valid = e >= a.ov && e < lim;
        nn += (valid && q != q) ? 1u : 0u;                              // q is NaN exactly when a component is
        const bool take = valid && q > bq;                              // false for a NaN q
        bq = take ? q : bq; be = take ? (unsigned)e : be;
    }
#pragma unroll
    for (int mask = 32; mask >= 1; mask >>= 1) {
        const double oq = __shfl_xor(bq, mask);
        const unsigned oe = __shfl_xor(be, mask);
        nn += __shfl_xor(nn, mask);
        const bool take = oq > bq || (oq == bq && oe < be);
        bq = take ? oq : bq; be = take ? oe : be;
    }
    auto rs = __builtin_amdgcn_make_buffer_rsrc(a.parts + blk * WAVES, 0, blk < a.nblocks ? WAVES * 16 : 0, 0x00020000);
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const unsigned long long qb = __builtin_bit_cast(unsigned long long, bq);
    u32x4 r; r.x = (unsigned)qb; r.y = (unsigned)(qb >> 32); r.z = be; r.w = nn;
    const int off = (tid & 63) == 0 ? (tid >> 6) * 16 : 0x7ffffff0;
    __builtin_amdgcn_raw_buffer_store_b128(r, rs, off, 0, NT ? kStoreAux : 0);
}

// CHECK = false: the caller knows that the block exists (no branch around the stores, so that hipcc keeps
// counting the memory operations in flight across them)
template <class C, bool SCALED, bool NT, bool CHECK = true, bool DECIM = false>
__device__ __forceinline__ void store_block(const cf (&w)[C::P], const FmiArgs &a, long long blk, int tid)
{
    if constexpr (CHECK) { if (blk >= a.nblocks) return; }
    const long long base = blk * a.hop - a.ov;              // output index of window element 0
    if constexpr (C::F == 1 && DECIM) {
        // sampling::downsample behind the filter (sampling.rs:28-42: dst[i] = src[i * dec]) folded into the store:
        // output sample o of the stream is kept iff dec divides it, and lands at out[o / dec].  32-bit index
        // arithmetic (the host side checks n < 2^31); q0 = first kept index of this block, descriptor from there.
        const unsigned o0 = (unsigned)(blk * a.hop);                              // first output sample of the block
        const unsigned q0 = aeth::fdiv(o0 + a.dec.d - 1, a.dec);
        const long long left = a.n_out - (long long)q0;
        const int bytes = left > 0 ? (int)(left < (long long)C::N ? left : (long long)C::N) * 8 : 0;
        auto rs = __builtin_amdgcn_make_buffer_rsrc(a.out + q0, 0, bytes, 0x00020000);
        const cf ss = mk(a.s_bwd, a.s_bwd);
#pragma unroll
        for (int m = 0; m < C::P; m++) {
            const int e = tid + m * C::T;
            const unsigned o = o0 + (unsigned)(e - a.ov);                         // meaningful for e >= ov only
            const unsigned q = aeth::fdiv(o, a.dec);
            const bool keep = e >= a.ov && q * a.dec.d == o && (long long)o < a.n;
            const int off = keep ? (int)(q - q0) * 8 : 0x7ffffff0;
            cf v = SCALED ? cscale_k(w[m], ss) : w[m];
            __builtin_amdgcn_raw_buffer_store_b64(as_u32x2(v), rs, off, 0, NT ? StreamPolicy<C>::store : 0);
        }
    } else if constexpr (C::F == 1) {
        long long left = a.n - base;
        int bytes = (int)(left < a.frame_n ? left : a.frame_n) * 8;   // stores past the end (of the stream, of the frame) are dropped by the range check
        if constexpr (!CHECK) { if (blk >= a.nblocks) bytes = 0; }    // a block past the end: every store dropped, no branch
        auto rs = __builtin_amdgcn_make_buffer_rsrc(a.out + base, 0, bytes, 0x00020000);
        const cf ss = mk(a.s_bwd, a.s_bwd);
        // no branch around the stores either: window elements in front of the valid part
        // (e < ov) get an offset past the descriptor's range and are dropped by its check
#pragma unroll
        for (int m = 0; m < C::P; m++) {
            const int e = tid + m * C::T;
            const int off = (e >= a.ov) ? e * 8 : 0x7ffffff0;
            cf v = SCALED ? cscale_k(w[m], ss) : w[m];
            __builtin_amdgcn_raw_buffer_store_b64(as_u32x2(v), rs, off, 0, NT ? StreamPolicy<C>::store : 0);   // streamed stores (kStoreAux)
        }
    } else {
#pragma unroll
        for (int m = 0; m < C::P; m++) {
            const int e = tid + m * C::T;
            const long long o = base + e;
            if (e >= a.ov && o < a.n && e < a.frame_n) a.out[o] = SCALED ? cscale(w[m], a.s_bwd) : w[m];
        }
    }
}

// the chain on one block held in w[]: vec_rfft -> vec_mul -> vec_rifft (benches/benches.rs:410-416)
// V_SPREAD form for three-pass configurations: nx[] = the window of block `gn`, loaded in four instalments
template <class C, bool NT, int VAR>
__device__ __forceinline__ void transform_block_spread(cf (&w)[C::P], cf (&nx)[C::P], const cf (&tw)[C::TW], const cf (&H)[C::P],
                                                       cf *__restrict__ lds, const FmiArgs &a, long long gn, int tid)
{
    static_assert(C::NPASS == 3 && C::P % 4 == 0, "spread loads: three passes");
    constexpr int XP = ((VAR & V_PRIO) ? 1 : 0) | ((VAR & V_XOR) ? 8 : 0);
    constexpr int Q = C::P / 4;
    load_window_srd_part<C, NT, 0, Q>(nx, a, gn, tid);
    run_pass<C, 0, +1, 0, XP>(w, tw, lds, tid);
    load_window_srd_part<C, NT, Q, 2 * Q>(nx, a, gn, tid);
    run_pass<C, 1, +1, 0, XP>(w, tw, lds, tid);
    load_window_srd_part<C, NT, 2 * Q, 3 * Q>(nx, a, gn, tid);
    run_pass<C, 2, +1, 0, XP>(w, tw, lds, tid);
#pragma unroll
    for (int m = 0; m < C::P; m++) w[m] = cmul(w[m], H[m]);
    load_window_srd_part<C, NT, 3 * Q, 4 * Q>(nx, a, gn, tid);
    fft_in_regs<C, -1, fft_next_par<C>(0), XP>(w, tw, lds, tid);
}

template <class C, bool SCALED, bool BLU, int VAR>
__device__ __forceinline__ void transform_block(cf (&w)[C::P], const cf (&tw)[C::TW], const cf (&H)[C::P],
                                                cf *__restrict__ lds, const FmiArgs &a, int tid)
{
    constexpr int XP = ((VAR & V_PRIO) ? 1 : 0) | ((VAR & V_XOR) ? 8 : 0);
    if constexpr (BLU) {
        // x[n] (conjugated for the other exponent sign) * chirp[n]; chirp is 0 beyond the frame (descriptor range)
        auto cr = __builtin_amdgcn_make_buffer_rsrc(const_cast<cf *>(a.chirp), 0, a.frame_n * 8, 0x00020000);
#pragma unroll
        for (int m = 0; m < C::P; m++) {
            const cf ch = as_cf(__builtin_amdgcn_raw_buffer_load_b64(cr, (tid + m * C::T) * 8, 0, 0));
            cf v = w[m];
            if (a.conj) v.y = -v.y;
            w[m] = cmul(v, ch);
        }
    }
    fft_in_regs<C, +1, 0, XP>(w, tw, lds, tid);             // vec_rfft: the reference's fwd (+j exponent)
    if constexpr (SCALED) {
        const cf ss = mk(a.s_fwd, a.s_fwd);
#pragma unroll
        for (int m = 0; m < C::P; m++) w[m] = cscale_k(w[m], ss);           // Scale of vec_rfft
    }
#pragma unroll
    for (int m = 0; m < C::P; m++) w[m] = cmul(w[m], H[m]);                 // vec_mul (vecops.rs:99-112)
    fft_in_regs<C, -1, fft_next_par<C>(0), XP>(w, tw, lds, tid);   // vec_rifft: bwd (-j); two transforms leave the parity even
    if constexpr (BLU) {
        auto cr = __builtin_amdgcn_make_buffer_rsrc(const_cast<cf *>(a.chirp), 0, a.frame_n * 8, 0x00020000);
#pragma unroll
        for (int m = 0; m < C::P; m++) {
            const cf ch = as_cf(__builtin_amdgcn_raw_buffer_load_b64(cr, (tid + m * C::T) * 8, 0, 0));
            cf v = cmul(w[m], ch);
            if (a.conj) v.y = -v.y;
            w[m] = v;
        }
    }
}

// SCALED = false: both Scale factors are 1 (FIR: 1/N is folded into H)
// BLU: chirp-z frames (see FmiArgs): the frame is multiplied by the chirp behind the load and in front of the store
template <class C, bool SCALED, int MINW, bool NT, bool BLU, int VAR = 0>
__global__ __launch_bounds__(C::WG, MINW) void fmi_kernel(FmiArgs a)
{
    static_assert((VAR & ~V_ALL) == 0, "VAR names a kernel variant that does not exist");
    __shared__ cf lds_all[C::LDS_TOTAL];
    // F == 1: the whole workgroup is one frame, so the block index stays provably wave-uniform
    const int tid = (C::F == 1) ? (int)threadIdx.x : (int)(threadIdx.x % C::T);
    const int fl = (C::F == 1) ? 0 : (int)(threadIdx.x / C::T);
    cf *lds = lds_all + fl * C::LDS_FRAME;
    const long long ngroups = (a.nblocks + C::F - 1) / C::F;
    cf nx[C::P], tw[C::TW], H[C::P];
    constexpr int DM = (VAR & V_DM_BPSK) ? DM_BPSK : (VAR & V_DM_QGEN) ? DM_QGEN : DM_QSEP;
    static_assert(!(VAR & (V_DM_BPSK | V_DM_QGEN)) || (VAR & V_DEMOD), "decision mode without V_DEMOD");
    [[maybe_unused]] DemodK dk;
    if constexpr (VAR & V_DEMOD) dk = demod_consts<DM>(a);
    constexpr int LK = (VAR & V_LV_DB) ? AETH_LEVEL_DB : (VAR & V_LV_POWER_DB) ? AETH_LEVEL_POWER_DB : AETH_LEVEL_NORM;
    static_assert(!(VAR & (V_LV_DB | V_LV_POWER_DB)) || (VAR & V_LEVEL), "level kind without V_LEVEL");
    static_assert(!(VAR & (V_LEVEL | V_PEAK)) || (C::F == 1 && !BLU && !(VAR & (V_DEMOD | V_DECIM))),
                  "level store / peak search: the plain loop of one-block workgroups");
    // software pipeline: the next block's window is in flight while this one is transformed.
    // The first window goes out before the (L2-resident) tables so the HBM fetch starts at once.
    load_window<C, NT>(nx, a, (long long)blockIdx.x * C::F + fl, tid);
    if (a.twL) load_twiddles_lane<C>(tw, a.twL, tid);
    else load_twiddles<C>(tw, a.twN, tid);
#pragma unroll
    for (int m = 0; m < C::P; m++) H[m] = a.Hf[tid + m * C::T];
    // Drain the table loads HERE, once.  Otherwise hipcc places their counted waits at the first
    // uses inside the loop body, where they run every iteration and end in vmcnt(0) halfway
    // through each block -- forcing the prefetched window AND the previous block's stores to
    // complete there instead of riding under the whole block.
    __builtin_amdgcn_s_waitcnt(0x0F70);                     // vmcnt(0) only
#pragma unroll 1
    for (long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
        const long long blk = g * C::F + fl;
        cf w[C::P];
#pragma unroll
        for (int m = 0; m < C::P; m++) w[m] = nx[m];
        // window samples older than the ntaps-1 the outputs depend on are forced to zero, so a
        // block is a function of exactly x[out0-(ntaps-1) .. out0+hop): shards of one stream
        // (history = ntaps-1 samples) then reproduce the unsharded run bit for bit
        if constexpr (C::F == 1) { if (tid < a.ov - a.nhist) w[0] = mk(0.f, 0.f); }
        const long long gn = g + gridDim.x;
        if constexpr (C::F == 1 && (VAR & V_SPREAD) && !SCALED && !BLU) {
            // (loads issued inside transform_block_spread)
        } else if constexpr (C::F == 1) {
            // gn >= gridDim.x >= 1, so the window never starts before the stream: descriptor path
            load_window_srd<C, NT>(nx, a, gn, tid);
        } else {
            if (gn < ngroups) load_window<C, NT>(nx, a, gn * C::F + fl, tid);
        }
        if constexpr (C::F == 1 && (VAR & V_SPREAD) && !SCALED && !BLU) transform_block_spread<C, NT, VAR>(w, nx, tw, H, lds, a, gn, tid);
        else transform_block<C, SCALED, BLU, VAR>(w, tw, H, lds, a, tid);
        if constexpr (VAR & V_DEMOD) demod_block<C, SCALED, NT, DM>(w, a, dk, blk, tid);
        else if constexpr (VAR & V_LEVEL) level_block<C, SCALED, NT, LK>(w, a, blk, tid);
        else if constexpr (VAR & V_PEAK) peak_block<C, SCALED, NT>(w, a, blk, tid);
        else store_block<C, SCALED, NT, true, (VAR & V_DECIM) != 0>(w, a, blk, tid);
    }
}

}  // namespace firk
}  // namespace aeth
