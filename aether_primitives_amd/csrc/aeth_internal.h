// aeth_internal.h -- shared host-side plumbing for libaether_hip.so (not installed).
#pragma once

#include <hip/hip_runtime.h>

#include <array>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../../include/aether_hip.h"
#include "aeth_lane_hazards.h"

namespace aeth {
struct PipeState;
// one device buffer a context keeps between calls: grown on demand (scratch_ensure), given back by aeth_ctx_trim
struct DevScratch {
    void *p = nullptr;
    size_t bytes = 0;
};
}  // namespace aeth

struct aeth_ctx {
    int device = 0;
    hipStream_t stream_main = nullptr;   // use aeth::ctx_stream(ctx): it orders the caller behind the overlap lane
    bool owns_stream = false;
    int num_cus = 256;
    // Overlap lane (aeth_ctx_set_overlap): a second HIP queue.  Consecutive fused-FIR launches alternate between the
    // two queues, so that the drain of one launch (its last round only stores) runs beside the fill of the next (its
    // first round only loads).  A chain starts on the main stream behind everything enqueued before it; each later
    // launch goes where no buffer hazard is left open (ctx_fir_lane: `hazards` holds the ranges of both lanes since
    // the last join), with no event packet in front of it.  Any other call on the context joins the lane first, so
    // results are those of one in-order stream.
    hipStream_t stream_aux = nullptr;
    hipEvent_t ev_head = nullptr;  // recorded on the main stream in front of the head of a chain, unless the context was idle
    bool aux_behind_head = false;  // ... and the aux lane has not waited for it yet: its first launch of the chain does
    hipEvent_t ev_aux_done = nullptr;
    bool overlap = false;          // feature switch (off for borrowed streams)
    bool stream_shared = false;    // aeth_ctx_stream() handed the main stream to code this library does not see: the
                                   // lane stays out of use until aeth_ctx_set_overlap(ctx, 1) is called again
    bool aux_pending = false;      // the aux lane holds work the main stream is not yet ordered behind
    int chain_last = -1;           // lane of the latest FIR launch while nothing else has been enqueued since; else -1
    bool last_chained = false;     // the latest ctx_fir_lane call put its launch beside its predecessor
    aeth::lanes::Tracker hazards;  // what the launches of the chain read and write, per lane; reset with chain_last
    uint64_t lane_packets = 0;     // event-wait / event-record packets ctx_fir_lane has put in front of launches
    uint64_t lane_joins = 0;       // chains ctx_fir_lane ended itself: a hazard on both lanes, or a full tracker
    unsigned since_sync = 0;       // stream hand-outs (= launches, roughly) since the last aeth_ctx_sync: a short wait blocks, a long one polls
    // host pipeline (aeth_fir_stream_host): stage streams, device slots, events, pinned staging pool, copy threads --
    // created on its first run and kept (aeth_host.h)
    aeth::PipeState *pipe = nullptr;
    // Device scratch, one buffer per user -- they are held at the same time (aeth_fir_exec_host keeps both staging slots
    // across its launch; aeth_corr_search keeps its slab while HostIO may hold stage[1]):
    //   stage[2]    the host-slice flavours' input / output (ctx_stage)
    //   stats_slab  per-chunk records of aeth_vec_stats (aeth_stats.hip)
    //   corr_slab   per-wave and per-workgroup records of aeth_corr_search (aeth_fir.hip)
    //   sync_slab   [chunk records][block records] of aeth_sync_line / aeth_sync_lag (aeth_sync.hip), and
    //   mov_slab    the same of aeth_mov_search (aeth_mov.hip): the layout is aeth::red::run_blocks' (aeth_reduce.h)
    //   spec_slab   [chunk sums][chunk maxima] of aeth_vec_frame_sums / aeth_chan_exec_sums (aeth_spec.hip)
    aeth::DevScratch stage[2], stats_slab, corr_slab, sync_slab, mov_slab, spec_slab;
    // small host-slice calls: two pinned, device-visible bounce buffers (aeth::HostIO)
    void *bounce[2] = {nullptr, nullptr};
    // plans of the one-shot vec_fft / vec_ifft (aeth_fft.hip: fft_cache_get), most recently used first
    void *fft_cache = nullptr;
};

namespace aeth {

int set_error(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));
int hip_fail(hipError_t e, const char *what);

// The context's stream for anything but a chained FIR launch: joins the overlap lane (the main stream waits for
// what the aux lane still holds) and ends the chain.
hipStream_t ctx_stream(aeth_ctx *ctx);
inline hipStream_t ctx_stream(const aeth_ctx *ctx) { return ctx_stream(const_cast<aeth_ctx *>(ctx)); }
// Stream for a fused-FIR launch that reads a.in[] and writes a.out (EVERY buffer the caller owns and the kernel
// touches).  While the previous call on this context was such a launch: the lane beside it when `a` has no hazard
// with anything on the predecessor's lane, the predecessor's own lane (in order behind it) when the hazards are all
// there, else the main stream behind a join.
hipStream_t ctx_fir_lane(aeth_ctx *ctx, const lanes::Access &a);
// no launch of the lane is the context's latest call any more: the next ctx_fir_lane starts a chain
inline void ctx_chain_end(aeth_ctx *ctx)
{
    ctx->chain_last = -1;
    ctx->last_chained = false;
    ctx->hazards.reset();
}

// Ensure `s` holds >= bytes of device memory: nothing happens when it already does; else it is replaced by a buffer of
// bytes + bytes/4 (`slack`: the context's own buffers) or of exactly bytes (the filter banks' frames, aeth_bank.h).  The
// context's stream is waited for before the old buffer is freed.  (The staging slots used to be
// freed without that wait: hipFree waits for the device itself and the host-slice calls are synchronous, so the
// explicit wait changes nothing observable there.)
int scratch_ensure(aeth_ctx *ctx, DevScratch &s, size_t bytes, bool slack = true);
// frees it; on a failed free the buffer stays recorded and the HIP error is returned (aeth_ctx_trim reports it,
// aeth_ctx_destroy does not)
hipError_t scratch_release(DevScratch &s);
// every scratch buffer of the context
inline std::array<DevScratch *, 7> ctx_scratch(aeth_ctx *ctx)
{
    return {&ctx->stage[0], &ctx->stage[1], &ctx->stats_slab, &ctx->corr_slab, &ctx->sync_slab, &ctx->mov_slab, &ctx->spec_slab};
}
// ensure staging slot `i` holds >= bytes of device memory (an unused slot still gets 16 bytes)
inline int ctx_stage(aeth_ctx *ctx, int i, size_t bytes) { return scratch_ensure(ctx, ctx->stage[i], bytes ? bytes : 16); }
// frees the plans vec_fft / vec_ifft built for this context (aeth_ctx_destroy, aeth_ctx_trim)
void fft_cache_release(aeth_ctx *ctx);

// Buffers of one host-slice call (the literal trait call: host slice in, host slice out, synchronous).
//   small (every buffer <= kZeroCopyMax): the context's two pinned, device-visible bounce buffers -- memcpy in, the kernel
//     reads and writes HOST memory over PCIe, one wait, memcpy out: one launch and one completion round trip per call.
//     Measured (tools/host_latency.hip, 2048 samples): 15.4 us against 31.6 us for pageable H2D -> kernel -> D2H and
//     19.7 us for pinned async copies around a device-resident kernel; the floor (an empty kernel + wait) is 10.4 us.
//   large: device staging and the runtime's copy engines, as before (link-rate-bound, not latency-bound).
constexpr size_t kZeroCopyMax = (size_t)256 << 10;
struct HostIO {
    aeth_ctx *ctx;
    bool pinned;
    void *buf[2] = {nullptr, nullptr};
    // bytes0 / bytes1: sizes of the two buffers the call needs (0: unused)
    int open(aeth_ctx *c, size_t bytes0, size_t bytes1);
    int put(int slot, const void *src, size_t bytes);          // caller memory -> buffer
    int get(void *dst, int slot, size_t bytes);                // after the kernels: wait, buffer -> caller memory
    int wait();                                                // the result stays in the buffer (tfwd / tbwd)
};

// Tuning knobs: environment integers that are consulted ONLY when the process was started with AETH_TUNING=1; a
// normal run never reads them.  libaether_hip.so carries the nine that choose between SHIPPED behaviours, all
// documented in include/aether_hip.h ("Tuning knobs"): AETH_FIR_GRID_FIRST, AETH_FIR_GRID_CHAINED, AETH_FIR_SPREAD,
// AETH_NT, AETH_PIPE_THREADS, AETH_PIPE_MIXED, AETH_SYNC_SPIN_US, AETH_SPEC_SLICE_KIB, AETH_CRC_ROUTE.
int tuning_int(const char *name, int dflt);
// Lab knobs (tools/tune_*.py, prime_route.py, vs_rocfft.py sweeps): routes and shapes that were measured and not
// kept.  They exist only in the lab build (`make LAB=1` -> lib/libaether_hip_lab.so, -DAETH_LAB=1); in the product
// every lab_int() is its default at compile time, so the paths behind the other values are not in the library.
#if defined(AETH_LAB) && AETH_LAB
#define lab_int tuning_int      /* the lab build reads them like any other knob */
#else
constexpr int lab_int(const char *, int dflt) { return dflt; }
#endif

inline bool aligned4(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 3u) == 0; }
inline bool aligned8(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }
inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
// [a, a + na) and [b, b + nb) share a byte?  (never for a null pointer or an empty range)
inline bool ranges_touch(const void *a, size_t na, const void *b, size_t nb)
{
    if (!a || !b || !na || !nb) return false;
    const uintptr_t a0 = (uintptr_t)a, a1 = a0 + na, b0 = (uintptr_t)b, b1 = b0 + nb;
    return a0 < b1 && b0 < a1;
}

// n / d for 32-bit n by multiply-high and shifts (Granlund-Montgomery round-up form):
// index arithmetic of store-bound kernels must not cost more than their stores.
struct FastDiv {
    uint32_t d, m, sh1, sh2;
};
inline FastDiv make_fastdiv(uint32_t d)
{
    FastDiv f;
    f.d = d;
    uint32_t l = 0;
    while ((1ull << l) < d) l++;
    f.m = (uint32_t)((((1ull << l) - d) << 32) / d + 1);
    f.sh1 = l < 1 ? l : 1;
    f.sh2 = l > 0 ? l - 1 : 0;
    return f;
}
__device__ __forceinline__ uint32_t fdiv(uint32_t n, const FastDiv &f)
{
    const uint32_t t = __umulhi(f.m, n);
    return (t + ((n - t) >> f.sh1)) >> f.sh2;
}

// Streamed data (touched exactly once by a kernel) is accessed with the non-temporal hint: no write-allocate,
// no retention in L2 / Infinity Cache.  Measured on MI355X with 256 MiB operands: element-wise kernels 5.9 -> 6.5
// TB/s, batched FFT 5.4 -> 5.8-6.1, interpolate 5.5 -> 6.2, the fused FIR kernel -3 % launch time.  A chain of
// kernels over an operand that FITS the 256 MiB cache wants the opposite (C4's 64 MiB channel: 107 GS/s with
// plain accesses, 96 with the hint), so the hint is a kernel template parameter picked per launch by size.
template <bool NT, typename V> __device__ __forceinline__ V nt_load(const V *p)
{
    static_assert(sizeof(V) == 4 || sizeof(V) == 8 || sizeof(V) == 16, "4-, 8- or 16-byte accesses");
    if constexpr (!NT) return *p;
    else {
        typedef unsigned VT __attribute__((ext_vector_type(sizeof(V) / 4)));
        if constexpr (sizeof(V) == 4) return __builtin_bit_cast(V, __builtin_nontemporal_load(reinterpret_cast<const unsigned *>(p)));
        else return __builtin_bit_cast(V, __builtin_nontemporal_load(reinterpret_cast<const VT *>(p)));
    }
}
template <bool NT, typename V> __device__ __forceinline__ void nt_store(V *p, V v)
{
    static_assert(sizeof(V) == 4 || sizeof(V) == 8 || sizeof(V) == 16, "4-, 8- or 16-byte accesses");
    if constexpr (!NT) *p = v;
    else {
        typedef unsigned VT __attribute__((ext_vector_type(sizeof(V) / 4)));
        if constexpr (sizeof(V) == 4) __builtin_nontemporal_store(__builtin_bit_cast(unsigned, v), reinterpret_cast<unsigned *>(p));
        else __builtin_nontemporal_store(__builtin_bit_cast(VT, v), reinterpret_cast<VT *>(p));
    }
}

// does a launch that moves `bytes` stream past the cache?  (half the 256 MiB Infinity Cache; AETH_NT=0/1 forces it
// under AETH_TUNING=1)
inline bool streams_past_cache(size_t bytes)
{
    const int forced = tuning_int("AETH_NT", -1);
    if (forced >= 0) return forced != 0;
    return bytes > ((size_t)128 << 20);
}

struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) ok = (hipSetDevice(dev) == hipSuccess);
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

}  // namespace aeth

#define AETH_HIP(call)                                              \
    do {                                                            \
        hipError_t e__ = (call);                                    \
        if (e__ != hipSuccess) return aeth::hip_fail(e__, #call);   \
    } while (0)

#define AETH_REQUIRE(cond, code, ...)                               \
    do {                                                            \
        if (!(cond)) return aeth::set_error((code), __VA_ARGS__);   \
    } while (0)

namespace aeth {
// what every transforming call asks of its sign and Scale kind
inline int check_sign_scale(int sign, int kind)
{
    AETH_REQUIRE(sign == AETH_SIGN_REF_FWD || sign == AETH_SIGN_REF_BWD, AETH_E_ARG, "sign must be +1 or -1");
    AETH_REQUIRE(kind >= AETH_SCALE_NONE && kind <= AETH_SCALE_X, AETH_E_ARG, "bad scale kind %d", kind);
    return AETH_OK;
}

// a table built on the host goes to a new device buffer *dev on the context's stream, which is waited for; on a failure
// nothing stays allocated, *dev is null and `what` names the upload in the HIP error's text
int upload_table(aeth_ctx *ctx, const void *host, size_t bytes, void **dev, const char *what);
template <class T> int upload_table(aeth_ctx *ctx, const void *host, size_t bytes, T **dev, const char *what)
{
    return upload_table(ctx, host, bytes, (void **)dev, what);
}

// ---- the call frontier of the code modules: what a call checks between its handle and its first launch, one small step
// each, run in the call's own order; none allocates
inline uint64_t mul_sat(uint64_t a, uint64_t b) { return b && a > UINT64_MAX / b ? UINT64_MAX : a * b; }   // or 2^64 - 1
inline int check_flags(uint32_t flags, uint32_t known)
{
    return flags & ~known ? set_error(AETH_E_ARG, "unknown flag bits 0x%x", flags & ~known) : AETH_OK;
}
// whole codewords on both sides, *F of them: an encoder's K bits in and N coded bits out, a decoder's (`dec`) N soft values
// in and N or K bits out
inline int check_codewords(bool dec, size_t nin, uint32_t per_in, size_t nout, uint32_t per_out, size_t *F)
{
    *F = nin / per_in;
    AETH_REQUIRE(nin == *F * per_in, AETH_E_LEN, dec ? "nsoft %zu is no multiple of N = %u" : "nbits %zu is no multiple of K = %u", nin, per_in);
    if (dec) AETH_REQUIRE(nout == *F * per_out, AETH_E_LEN, "%zu codewords give %zu bits (%u each), not %zu", *F, *F * per_out, per_out, nout);
    else AETH_REQUIRE(nout / per_out == *F && nout % per_out == 0, AETH_E_LEN, "%zu codewords of N = %u are %llu coded bits, not %zu", *F,
                      per_out, (unsigned long long)mul_sat(*F, per_out), nout);
    return AETH_OK;
}
// No output may share a byte with an input or with another output: every output against every input, then every pair of
// outputs.  The text follows the number of slots the call declares, not of those in use, unless the call words it (`io_text`).
struct Span { const void *p; size_t bytes; };
inline int check_disjoint(std::initializer_list<Span> in, std::initializer_list<Span> out, const char *io_text = nullptr)
{
    if (!io_text)
        io_text = out.size() > 1 ? (in.size() > 1 ? "an output overlaps an input" : "an output overlaps the input")
                                 : (in.size() > 1 ? "the output overlaps an input" : "the output overlaps the input");
    for (const Span &o : out)
        for (const Span &i : in) AETH_REQUIRE(!ranges_touch(o.p, o.bytes, i.p, i.bytes), AETH_E_ARG, "%s", io_text);
    const char *oo_text = out.size() == 2 ? "the two outputs overlap" : "two outputs overlap";
    for (const Span *a = out.begin(); a != out.end(); a++)
        for (const Span *b = a + 1; b != out.end(); b++) AETH_REQUIRE(!ranges_touch(a->p, a->bytes, b->p, b->bytes), AETH_E_ARG, "%s", oo_text);
    return AETH_OK;
}
// `count` of the caller's `noun` ("frames", "codewords") ask for `workgroups` of them in one launch
inline int check_grid(uint64_t workgroups, size_t count, const char *noun)
{
    return workgroups >> 31 ? set_error(AETH_E_UNSUPPORTED, "%zu %s in one call: more than 2^31 workgroups", count, noun) : AETH_OK;
}
// a code object's destroy before it deletes the object, and its create when a later upload fails: waits for the context's
// stream and frees each buffer that is there (the slab's first); the first HIP error comes back once all have been freed
inline hipError_t release_tables(aeth_ctx *ctx, std::initializer_list<void *> bufs)
{
    DeviceGuard dg(ctx->device);
    (void)hipStreamSynchronize(ctx_stream(ctx));
    hipError_t first = hipSuccess;
    for (void *b : bufs)
        if (const hipError_t e = b ? hipFree(b) : hipSuccess; first == hipSuccess) first = e;
    return first;
}

// What a call over complex samples checks behind its lengths and before any device work: n input samples, hist_elems
// samples of history (hist may be null), n_out output elements of out_elem_bytes each, `count` of the caller's `noun`
// ("frames", "outputs") on at most `grid` workgroups.
inline int check_buffers(const aeth_cf32 *hist, size_t hist_elems, const aeth_cf32 *in, size_t n, const void *out, size_t n_out,
                         size_t out_elem_bytes, size_t grid, size_t count, const char *noun)
{
    AETH_REQUIRE(in && out, AETH_E_ARG, "null pointer");
    AETH_REQUIRE(aligned8(in) && aligned8(hist), AETH_E_ALIGN, "input or history pointer not 8-byte aligned");
    AETH_REQUIRE(((uintptr_t)out & (out_elem_bytes - 1)) == 0, AETH_E_ALIGN, "output pointer not %zu-byte aligned", out_elem_bytes);
    const int rc = check_disjoint({{in, n * sizeof(aeth_cf32)}, {hist, hist_elems * sizeof(aeth_cf32)}}, {{out, n_out * out_elem_bytes}},
                                  "the output range overlaps the input (or its history)");
    return rc ? rc : check_grid(grid, count, noun);
}
}  // namespace aeth

// message texts of the reference's panics (kept verbatim for the binding)
#define AETH_MSG_VEC_LEN "Vectors must have same length"            /* src/vecops.rs:100-104 */
#define AETH_MSG_FFT_LEN "Input and FFT must be the same length"    /* src/fft.rs:163-167   */
#define AETH_MSG_DECIM   "Only even decimations are supported"      /* src/sampling.rs:32-36 */
