/*
 * aether_hip.h -- C ABI of the MI355X (gfx950) backend for the cf32 hot path of
 * razorheadfx/aether_primitives: VecOps / Fft / FIR / sampling.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ or torch types.
 * The reference is a Rust crate; a maintainer binds these symbols from an
 * `extern "C"` block and implements the crate's own traits on top (rust/ in
 * this repo holds that binding; INTEGRATION.md walks through it).  Each entry
 * point cites the reference interface (path:line in the upstream tree) it
 * replaces.
 *
 * Conventions
 *  - aeth_cf32 is bit-identical to the crate's cf32 = Complex<f32>, repr(C)
 *    (src/lib.rs:8-12) and to HIP float2.
 *  - Every function returns AETH_OK (0) or a negative AETH_E_* code and never
 *    unwinds.  aeth_last_error() returns a thread-local message.  The
 *    reference's convention is panic-on-misuse (assert_eq!, e.g.
 *    src/vecops.rs:100-104, src/fft.rs:163-167); the binding re-raises
 *    AETH_E_LEN as a panic with the reference's message text, which
 *    aeth_last_error() carries verbatim.
 *  - "dev" functions take DEVICE pointers, are ordered on the context's HIP
 *    stream and return without waiting (aeth_ctx_sync to wait).
 *    "host" functions take HOST slices, stage through the context's pinned
 *    buffers and return when the result is back in the caller's slice --
 *    the literal one-frame-per-call trait semantics (PCIe-bound; use the dev
 *    flavour on the hot path).
 *  - A context/plan is not thread-safe (every reference method takes
 *    `&mut self`), but may move between threads; distinct contexts are
 *    independent (one device + one stream each).
 *  - Buffers: device pointers must be 8-byte aligned (AETH_E_ALIGN otherwise);
 *    16-byte alignment enables the widest loads.
 */
#ifndef AETHER_HIP_H
#define AETHER_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AETH_API __attribute__((visibility("default")))

/* src/lib.rs:8-12 */
typedef struct { float re, im; } aeth_cf32;

typedef struct aeth_ctx aeth_ctx;       /* device + stream + staging buffers      */
typedef struct aeth_fft aeth_fft;       /* replaces Cfft (src/fft.rs:134-159)     */
typedef struct aeth_fir aeth_fir;       /* gives Fir<T> (src/fir.rs:3-22) a body  */
typedef struct aeth_corr aeth_corr;     /* streaming correlator: a matched filter with fused level / peak stores */
typedef struct aeth_seq aeth_seq;       /* LFSR sequences: sequence::generate (src/sequence.rs:47-53) for linear generators */
typedef struct aeth_chan aeth_chan;     /* polyphase analysis filter bank: windowed, overlapped frames in front of aeth_fft */
typedef struct aeth_synth aeth_synth;   /* polyphase synthesis filter bank: weighted overlap-add behind aeth_fft */
typedef struct aeth_resamp aeth_resamp; /* polyphase rational resampler: up U, real FIR, down Q in one pass */
typedef struct aeth_arb aeth_arb;       /* arbitrary-ratio resampler: interpolated polyphase taps behind a Q32.32 time word */
typedef struct aeth_cc aeth_cc;         /* convolutional code: encoder and block-wise soft-decision Viterbi decoder */
typedef struct aeth_remap aeth_remap;   /* rate matching: a periodic byte map (puncture, depuncture, interleave, chains) */
typedef struct aeth_crc aeth_crc;       /* frame checks: a CRC of width 1 .. 64 over bit frames: registers, attach, check */
typedef struct aeth_rs aeth_rs;         /* Reed-Solomon code over GF(2^m): systematic encoder, errors-and-erasures decoder */
typedef struct aeth_ldpc aeth_ldpc;     /* quasi-cyclic LDPC code: systematic encoder and layered integer min-sum decoder */
typedef struct aeth_turbo aeth_turbo;   /* turbo code: two RSC encoders and a windowed max-log-MAP iterative decoder */
typedef struct aeth_polar aeth_polar;   /* polar code: encoder and successive-cancellation decoder with a flip and candidate records */
typedef struct aeth_polar_list aeth_polar_list;   /* polar code: successive-cancellation list decoder with path metrics */
typedef struct aeth_ofdm aeth_ofdm;    /* OFDM symbols: strip + transform + pick + equalise, and the way back, one kernel each */
typedef struct aeth_event aeth_event;   /* hipEvent on the context's stream       */
typedef struct aeth_pool aeth_pool;     /* replaces Pool<T> (src/pool.rs:71-160) for pinned host buffers */

enum {
    AETH_OK = 0,
    AETH_E_LEN = -1,          /* the reference's assert_eq! length panics          */
    AETH_E_ARG = -2,          /* null pointer, bad enum, zero length where illegal */
    AETH_E_ALIGN = -3,        /* device pointer not 8-byte aligned                  */
    AETH_E_HIP = -4,          /* a HIP runtime call failed (message has details)   */
    AETH_E_NOMEM = -5,
    AETH_E_UNSUPPORTED = -6   /* e.g. an FFT length the backend cannot plan        */
};

/* enum Scale, src/fft.rs:6-18 */
enum { AETH_SCALE_NONE = 0, AETH_SCALE_SN = 1, AETH_SCALE_N = 2, AETH_SCALE_X = 3 };

/* Sign of the DFT exponent: out[k] = sum_n in[n] * exp(sign * 2*pi*i*n*k/N).
 * The reference plans Fft::fwd with FFTplanner::new(true) and Fft::bwd with
 * FFTplanner::new(false) (src/fft.rs:148,150); in rustfft 3.x the argument is
 * `inverse`, so fwd carries the +j exponent.  The binding maps
 * fwd/ifwd/tfwd -> AETH_SIGN_REF_FWD and bwd/ibwd/tbwd -> AETH_SIGN_REF_BWD in
 * exactly one place. */
enum { AETH_SIGN_REF_FWD = +1, AETH_SIGN_REF_BWD = -1 };

/* Tuning knobs.  The library reads these environment integers ONLY in a process started with AETH_TUNING=1; each
 * chooses between behaviours that ship (measured routes and shapes that were not kept are not in the library at all:
 * csrc/aeth_internal.h, lab_int):
 *   AETH_FIR_GRID_FIRST    sixteenths of the resident grid for a fused-FIR launch that starts a chain or runs alone
 *                          with the overlap lane on (default 16)
 *   AETH_FIR_GRID_CHAINED  the same for a launch that runs beside its predecessor (default 12); values above 16
 *                          oversubscribe: the workgroups without a slot start as earlier ones finish (measured
 *                          20 / 24 / 32: within noise of 12, profiles/r04_k20_trace.txt)
 *   AETH_FIR_SPREAD        0 / 1: force the burst / spread form of the next-window prefetch (default: spread for a
 *                          lone launch, burst beside another)
 *   AETH_NT                0 / 1: force plain / non-temporal accesses on streamed operands (default: by size)
 *   AETH_PIPE_THREADS      host copy threads of the stream pipeline (default: 3/8 of the cores the process may use -- affinity mask and
 *                          cgroup CPU quota --, 2..12)
 *   AETH_PIPE_MIXED        1: a pageable input next to a pinned output downloads directly into the caller's memory
 *                          (default 0: both sides staged -- the mixed form measured 2.4 x slower downloads)
 *   AETH_SYNC_SPIN_US      how long aeth_ctx_sync polls both queues before it blocks (default 2000)
 *   AETH_SPEC_SLICE_KIB    KiB of spectrum the general route of aeth_chan_exec_sums keeps at a time (default 65536; the
 *                          result does not depend on it)
 *   AETH_CRC_ROUTE         2: aeth_crc_exec / attach / check take the long route for every L >= 1 (default 0: by L,
 *                          aeth_crc_route; the result does not depend on it) */
AETH_API const char *aeth_last_error(void);
AETH_API int aeth_version(void);                     /* 0x00MMmmpp */
AETH_API int aeth_device_count(int *count);

/* ---- context ----------------------------------------------------------- */
AETH_API int aeth_ctx_create(int device, aeth_ctx **out);
/* borrow an existing hipStream_t (e.g. torch's current stream); not destroyed */
AETH_API int aeth_ctx_create_on_stream(int device, void *hip_stream, aeth_ctx **out);
AETH_API int aeth_ctx_destroy(aeth_ctx *ctx);
AETH_API int aeth_ctx_sync(aeth_ctx *ctx);
/* Overlap lane (no reference counterpart: the reference is synchronous; this is the device analogue of keeping
 * two stages of src/pipeline.rs:52-137 busy).  When enabled, consecutive aeth_fir_exec (and aeth_fft_mul_ifft_demod)
 * calls alternate between two HIP queues of the context, so that the end of one launch overlaps the start of the
 * next.  The ordering guarantee: such a launch is ordered behind every earlier launch whose buffers it touches --
 * it reads what that one writes, or writes what that one reads or writes, in any byte -- and behind everything
 * enqueued on the context before the first of these launches; launches that share no buffer may run in either order
 * or side by side.  Every other call (and aeth_ctx_sync / aeth_event_record) is ordered behind both queues, so
 * results are those of one in-order stream.  Off by default; refused for contexts on a borrowed stream. */
AETH_API int aeth_ctx_set_overlap(aeth_ctx *ctx, int enable);
AETH_API int aeth_ctx_overlap(const aeth_ctx *ctx);   /* 1 if enabled AND in use (0 while aeth_ctx_stream has parked it) */
/* What the lane has spent on ordering since the context was created (either pointer may be null): event-wait and
 * event-record packets put in front of its launches, and chains it ended with a join of the two queues because a
 * launch touched buffers of launches on both (or the host's record of them was full).  A chain of independent
 * launches over a rotating buffer set costs at most two packets at its start (none on an idle context) and none after. */
AETH_API int aeth_ctx_lane_counts(const aeth_ctx *ctx, uint64_t *packets, uint64_t *joins);
/* hipStream_t of the context, for interop (torch ExternalStream, the caller's own copies and kernels).  Handing it out
 * parks the overlap lane: every later launch stays on this stream, so work the caller enqueues on it is ordered behind
 * the library's, until the caller re-arms the lane with aeth_ctx_set_overlap(ctx, 1). */
AETH_API void *aeth_ctx_stream(aeth_ctx *ctx);
AETH_API int aeth_ctx_device(const aeth_ctx *ctx);

/* ---- device memory (caller-owned; the library never keeps host pointers) -- */
AETH_API int aeth_dev_alloc(aeth_ctx *ctx, size_t bytes, void **dptr);
AETH_API int aeth_dev_free(aeth_ctx *ctx, void *dptr);
AETH_API int aeth_upload(aeth_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);   /* waits */
AETH_API int aeth_download(aeth_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes); /* waits */
AETH_API int aeth_copy_dev(aeth_ctx *ctx, void *dst_dev, const void *src_dev, size_t bytes);  /* async */

/* ---- timing on the context's stream (bench harness) ---------------------- */
AETH_API int aeth_event_create(aeth_ctx *ctx, aeth_event **out);
AETH_API int aeth_event_destroy(aeth_event *ev);
AETH_API int aeth_event_record(aeth_event *ev);
AETH_API int aeth_event_sync(aeth_event *ev);
AETH_API int aeth_event_elapsed_ms(aeth_event *start, aeth_event *stop, float *ms);

/* ---- VecOps, device flavour: trait VecOps, src/vecops.rs:39-89 ------------ */
/* All in place on `self_`.  Binary ops take both lengths so the reference's
 * "Vectors must have same length" assert (e.g. :100-104) lives on this side. */
AETH_API int aeth_vec_scale (aeth_ctx *ctx, aeth_cf32 *self_, size_t n, float scale);          /* :94-97   */
AETH_API int aeth_vec_mul   (aeth_ctx *ctx, aeth_cf32 *self_, size_t n, const aeth_cf32 *other, size_t n_other); /* :99-112  */
AETH_API int aeth_vec_div   (aeth_ctx *ctx, aeth_cf32 *self_, size_t n, const aeth_cf32 *other, size_t n_other); /* :114-125 */
AETH_API int aeth_vec_conj  (aeth_ctx *ctx, aeth_cf32 *self_, size_t n);                       /* :127-130 */
AETH_API int aeth_vec_add   (aeth_ctx *ctx, aeth_cf32 *self_, size_t n, const aeth_cf32 *other, size_t n_other); /* :132-142 */
AETH_API int aeth_vec_sub   (aeth_ctx *ctx, aeth_cf32 *self_, size_t n, const aeth_cf32 *other, size_t n_other); /* :144-155 */
AETH_API int aeth_vec_mirror(aeth_ctx *ctx, aeth_cf32 *self_, size_t n);                       /* :157-161 */
AETH_API int aeth_vec_clone (aeth_ctx *ctx, aeth_cf32 *self_, size_t n, const aeth_cf32 *other, size_t n_other); /* :163-172 */
AETH_API int aeth_vec_zero  (aeth_ctx *ctx, aeth_cf32 *self_, size_t n);                       /* :174-177 */
/* vec_mirror applied to each of `batch` consecutive frames of `frame_len`
 * (the `chunks_mut(fft_len).for_each(|c| c.vec_rfft(..).vec_mirror())` idiom,
 * src/util/plot.rs:59-61) */
AETH_API int aeth_vec_mirror_frames(aeth_ctx *ctx, aeth_cf32 *self_, size_t frame_len, size_t batch);
/* vec_mul with ONE right-hand side shared by `batch` consecutive frames of `frame_len` (frames[f][j] *= sig[j]):
 * the middle step of `c.vec_rfft(..).vec_mul(&sig).vec_rifft(..)` over chunks_mut(fft_len)
 * (benches/benches.rs:410-416); n_sig != frame_len -> AETH_E_LEN with the reference's text (:100-104) */
AETH_API int aeth_vec_mul_frames(aeth_ctx *ctx, aeth_cf32 *frames, size_t frame_len, size_t batch,
                                 const aeth_cf32 *sig, size_t n_sig);
/* vec_mutate (:179-182) takes a Rust closure and stays on the host side of the binding. */
/* A CHAIN of the element-wise methods above in one pass over memory: `v.vec_add(&a).vec_mul(&b).vec_conj()` (the
 * reference's chaining, src/vecops.rs:12-38; BASELINE config 1) reads `self_` once, every binary link's operand once,
 * and writes `self_` once -- one launch and 32 B per sample for that chain instead of three launches and 64 B.  Each
 * link is its own kernel's arithmetic, rounded link by link: bit-identical to the separate calls.  Per link the checks
 * of its own entry point ("Vectors must have same length"); an operand that overlaps self_ is refused (AETH_E_ARG).
 * vec_mirror (a permutation) and vec_mutate (a closure) are not links.  Any number of steps (8 per pass). */
enum { AETH_VEC_SCALE = 0, AETH_VEC_MUL = 1, AETH_VEC_DIV = 2, AETH_VEC_CONJ = 3, AETH_VEC_ADD = 4, AETH_VEC_SUB = 5,
       AETH_VEC_CLONE = 6, AETH_VEC_ZERO = 7 };
typedef struct aeth_vec_step { int op; const aeth_cf32 *other_dev; size_t n_other; float scale; } aeth_vec_step;
AETH_API int aeth_vec_chain(aeth_ctx *ctx, aeth_cf32 *self_, size_t n, const aeth_vec_step *steps, size_t n_steps);

/* ---- VecOps, host-slice flavour (synchronous) ----------------------------- */
AETH_API int aeth_host_vec_scale (aeth_ctx *ctx, aeth_cf32 *self_, size_t n, float scale);
AETH_API int aeth_host_vec_mul   (aeth_ctx *ctx, aeth_cf32 *self_, size_t n, const aeth_cf32 *other, size_t n_other);
AETH_API int aeth_host_vec_div   (aeth_ctx *ctx, aeth_cf32 *self_, size_t n, const aeth_cf32 *other, size_t n_other);
AETH_API int aeth_host_vec_conj  (aeth_ctx *ctx, aeth_cf32 *self_, size_t n);
AETH_API int aeth_host_vec_add   (aeth_ctx *ctx, aeth_cf32 *self_, size_t n, const aeth_cf32 *other, size_t n_other);
AETH_API int aeth_host_vec_sub   (aeth_ctx *ctx, aeth_cf32 *self_, size_t n, const aeth_cf32 *other, size_t n_other);
AETH_API int aeth_host_vec_mirror(aeth_ctx *ctx, aeth_cf32 *self_, size_t n);
AETH_API int aeth_host_vec_clone (aeth_ctx *ctx, aeth_cf32 *self_, size_t n, const aeth_cf32 *other, size_t n_other);
AETH_API int aeth_host_vec_zero  (aeth_ctx *ctx, aeth_cf32 *self_, size_t n);

/* ---- VecStats and levels (no body in the reference yet) -------------------- */
/* The reference lists "Add VecStats (f32, cf32): Min(index), Max(index), Mean(index), Power" as an open item
 * (README.md:90-91) and maps every bin of a spectrum through c.norm() and, with use_db, DB::from(c).db()
 * (src/util/plot.rs:65,127; src/util/mod.rs:26-34: 10 * log10(ratio) in f64).  Both are defined here so that they can
 * be reproduced exactly with IEEE operations (csrc/aeth_levels.h), for a sample c = (re, im):
 *   q(c)    = (double)re * re + (double)im * im      one rounding of |c|^2, the same bits with or without fma
 *   norm(c) = (float)sqrt(q(c))                      Complex::norm() = hypot without hypot's platform dependence
 * Level kinds:
 *   AETH_LEVEL_NORM      norm(c)
 *   AETH_LEVEL_DB        (float)(10.0 * log10((double)norm(c))), the reference's literal DB::from(c.norm()).db().  This is
 *                        10 * log10 of an AMPLITUDE: the reference's quirk (a power level would be 20 * log10), kept as
 *                        the default like its other quirks
 *   AETH_LEVEL_POWER_DB  (float)(10.0 * log10(q(c))), the corrected form
 * norm = 0 gives -inf and a NaN component gives NaN, as Rust's f64::log10 does. */
enum { AETH_LEVEL_NORM = 0, AETH_LEVEL_DB = 1, AETH_LEVEL_POWER_DB = 2 };
/* One read-only pass over x (8 B per sample).  min / max are ordered by q (f64), ties go to the LOWEST index (numpy's
 * argmin / argmax); samples with a NaN component are counted in n_nan and are not candidates (all NaN: both indices
 * are n, both norms NaN).  The sums include NaN samples, so mean and power are NaN then, as IEEE says, and n_nan tells
 * why.  "Mean(index)" of the reference's list has no meaning that could be pinned down and is left out.
 * Bitwise reproducible: the f64 sums are combined in an order that depends on the element index and n only -- not on
 * the device's CU count, the pointer's alignment, the cache policy (AETH_NT) or host / device flavour.  Element counts
 * and indices are size_t throughout.  The struct shares its name with the function, so C and C++ callers alike
 * spell the type `struct aeth_vec_stats`. */
struct aeth_vec_stats {
    size_t n, n_nan;              /* samples; samples with a NaN component                       */
    size_t min_index, max_index;  /* LOWEST index among equal q; NaN samples are not candidates  */
    float  min_norm, max_norm;    /* norm() of those two samples                                 */
    double mean_re, mean_im;      /* sum(re) / n, sum(im) / n, accumulated in f64                */
    double power;                 /* sum(q) / n, accumulated in f64                              */
};
/* n == 0 -> AETH_E_LEN.  Waits for the result (the record is 64 bytes). */
AETH_API int aeth_vec_stats(aeth_ctx *ctx, const aeth_cf32 *x_dev, size_t n, struct aeth_vec_stats *out_host);
AETH_API int aeth_host_vec_stats(aeth_ctx *ctx, const aeth_cf32 *x_host, size_t n, struct aeth_vec_stats *out_host);
/* levels_dev[i] = level of x_dev[i] (8 B in, 4 B out per sample).  Stream-ordered, x_dev is not modified, the two
 * ranges must not overlap (AETH_E_ARG), levels_dev 4-byte aligned; n_levels != n -> AETH_E_LEN. */
AETH_API int aeth_vec_levels(aeth_ctx *ctx, const aeth_cf32 *x_dev, size_t n, int level_kind,
                             float *levels_dev, size_t n_levels);

/* ---- Scale: src/fft.rs:22-37 ---------------------------------------------- */
/* factor exactly as the reference computes it in f32: SN -> (n as f32).sqrt().recip(),
 * N -> (n as f32).recip(), X -> x, None -> 1 (and no pass at all). */
AETH_API float aeth_scale_factor(int scale_kind, size_t n, float x);
AETH_API int aeth_scale_apply(aeth_ctx *ctx, int scale_kind, float x, aeth_cf32 *data_dev, size_t n);

/* ---- Fft: trait Fft src/fft.rs:48-77, struct Cfft :134-235 ----------------- */
/* Cfft::with_len(len) (:147-158).  max_batch sizes the plan's device scratch
 * (>= 2*len*max_batch, mirroring Cfft.tmp :141,155); exec grows it on demand.
 * Lengths: every len from 1 to 2^23, and of the lengths in (2^23, 2^24] the power of two 2^24 and every product
 * n1 * n2 of two factors of at most 8192 points that one launch each transforms (a power of two, a row of the
 * register-resident table, or a length the LDS mixed-radix kernel does: prime factors all <= 61 in at most 16 radix passes).  Any other length takes the chirp-z
 * transform, whose convolution of M >= 2 len - 1 points (a power of two) is a plan of its own under the same limit;
 * above 2^23 that would be M = 2^25, and the call returns AETH_E_UNSUPPORTED with a message that names len (8388609
 * and 16777213 are such lengths; 9000000 = 3000 * 3000 is served).  len > 2^24 -> AETH_E_UNSUPPORTED.  Nothing stays
 * allocated after a refusal.  aeth_vec_fft, aeth_host_vec_fft and the host flavours plan through this call. */
AETH_API int aeth_fft_create(aeth_ctx *ctx, size_t len, size_t max_batch, aeth_fft **out);
AETH_API int aeth_fft_destroy(aeth_fft *plan);
AETH_API size_t aeth_fft_len(const aeth_fft *plan);                                   /* Fft::len :232-234 */
/* text name of the kernel path chosen for this length ("stockham_pow2", ...) */
AETH_API const char *aeth_fft_algorithm(const aeth_fft *plan);
/* the whole plan, sub-plans included, as text owned by the plan (valid until aeth_fft_destroy); "" for a null plan.
 *   route  := leaf | four | mixed | chirp
 *   leaf   := ("identity" | "stockham_pow2" | "stockham_mixed" | "stockham_mixed_ragged") " " len
 *   four   := "fourstep_pow2 " n1 "x" n2                      two launches: n1-point columns, n2-point rows
 *           | "fourstep_pow2 deep " n1 "x[" route "]"          the rows are a plan of their own (2^23, 2^24)
 *   mixed  := "fourstep_mixed[small " n1 " | " route "]"       n1 in 2..10, 12, 15, 16 in registers over one
 *                                                              register-resident transform of len / n1: no transposes
 *           | "fourstep_mixed[fast " route " x " route "]"     the pair nearest the square root whose factors are both
 *                                                              register-resident (power of two or table row)
 *           | "fourstep_mixed[fallback " route " x " route "]" else the nearest pair of single-launch factors
 *   chirp  := "bluestein " len " (one launch, M=" m ")"        the chirp-z chain in one kernel (m <= 4096; a call of
 *                                                              2^31 samples or more takes the multi-launch form)
 *           | "bluestein " len " (multi launch, M=" m ")[" route "]"   pre, transform, multiply, inverse, post; the
 *                                                              route is that of the m-point convolution transform
 * e.g. "fourstep_mixed[fallback bluestein 82 (one launch, M=256) x stockham_mixed_ragged 100]",
 *      "bluestein 2097153 (multi launch, M=8388608)[fourstep_pow2 deep 128x[fourstep_pow2 256x256]]". */
AETH_API const char *aeth_fft_route(const aeth_fft *plan);
/* `batch` frames of len() each, device pointers, out == in => in-place
 * (fwd/bwd :162-182, ifwd/ibwd :184-204).  n_in is the TOTAL element count of
 * `in` and must equal batch*len ("Input and FFT must be the same length"). */
AETH_API int aeth_fft_exec(aeth_fft *plan, const aeth_cf32 *in, size_t n_in, aeth_cf32 *out,
                           size_t batch, int sign, int scale_kind, float x);
/* The same followed by vec_mirror on every frame (`chunks_mut(fft_len).for_each(|c| c.vec_rfft(&mut fft, s)
 * .vec_mirror())`, src/util/plot.rs:59-61): for the register-resident power-of-two lengths the swap of the halves
 * is folded into the transform's store addresses (no second pass over memory), other lengths run the two steps. */
AETH_API int aeth_fft_exec_mirrored(aeth_fft *plan, const aeth_cf32 *in_dev, size_t n_in, aeth_cf32 *out_dev,
                                    size_t batch, int sign, int scale_kind, float x);
/* The whole `waterfall` / `spectrum` computation (src/util/plot.rs:46-68, :109-130) in one call, per frame: the
 * transform with its Scale, vec_mirror if mirror != 0, then the level of every bin (level kinds: see aeth_vec_levels).
 * in_dev is not modified.  Bit-identical to aeth_fft_exec / aeth_fft_exec_mirrored into a scratch buffer followed by
 * aeth_vec_levels.  For the register-resident power-of-two lengths the level is taken in registers and a 4-byte value
 * is stored where the 8-byte bin would go: the spectrum is never written (12 B per sample).  Other lengths run the
 * transform into the plan's temp (Cfft.tmp), then the levels kernel. */
AETH_API int aeth_fft_exec_levels(aeth_fft *plan, const aeth_cf32 *in_dev, size_t n_in, size_t batch, int sign,
                                  int scale_kind, float x, int mirror, int level_kind,
                                  float *levels_dev, size_t n_levels);
/* Per frame: the transform, then sampling::interpolate(&frame, &mut dst, n_between) (src/sampling.rs:7-24) -- BASELINE
 * config 5's chain in one call.  dst receives batch frames of len + (len-1)*n_between samples; `in` is not modified.
 * The spectrum goes through the plan's temp (Cfft.tmp); bit-identical to aeth_fft_exec + aeth_interpolate_frames. */
AETH_API int aeth_fft_exec_interpolate(aeth_fft *plan, const aeth_cf32 *in_dev, size_t n_in, size_t batch, int sign,
                                       int scale_kind, float x, aeth_cf32 *dst_dev, size_t dst_cap, size_t n_between,
                                       int compat_im, size_t *n_written);
/* VecOps::vec_fft / vec_ifft (src/vecops.rs:184-196): in place on a whole slice with a plan of its length.  The reference
 * builds a fresh Cfft on every call; the context keeps the plans these calls have built (the eight most recently used
 * lengths, 2^24 points in total at most; aeth_ctx_trim frees them), so a repeated length plans once.  sign: AETH_SIGN_REF_FWD for vec_fft, _BWD for vec_ifft. */
AETH_API int aeth_vec_fft(aeth_ctx *ctx, aeth_cf32 *x_dev, size_t n, int sign, int scale_kind, float x);
AETH_API int aeth_host_vec_fft(aeth_ctx *ctx, aeth_cf32 *x_host, size_t n, int sign, int scale_kind, float x);
/* host slices, one frame per call: the literal trait methods. out may equal in. */
AETH_API int aeth_fft_exec_host(aeth_fft *plan, const aeth_cf32 *in, size_t n_in,
                                aeth_cf32 *out, size_t n_out, int sign, int scale_kind, float x);
/* tfwd/tbwd (:206-230): transform into the plan's internal temp and lend it.
 * *view points to host memory valid until the next call on this plan. */
AETH_API int aeth_fft_exec_tmp_host(aeth_fft *plan, const aeth_cf32 *in, size_t n_in,
                                    int sign, int scale_kind, float x, const aeth_cf32 **view);
/* device flavour of the same: *view_dev is the plan's device temp */
AETH_API int aeth_fft_exec_tmp(aeth_fft *plan, const aeth_cf32 *in, size_t n_in, size_t batch,
                               int sign, int scale_kind, float x, const aeth_cf32 **view_dev);

/* ---- frequency-domain multiply chain: benches/benches.rs:410-416 ----------- */
/* frames.vec_rfft(fft, s_fwd).vec_mul(sig).vec_rifft(fft, s_bwd) per frame, fused into
 * one kernel (the "correlator inplace" benchmark; also BASELINE config 4).
 * `sig_dev` has fft_len elements.  In place on `frames_dev`. */
AETH_API int aeth_fft_mul_ifft(aeth_fft *plan, aeth_cf32 *frames_dev, size_t n_total, size_t batch,
                               const aeth_cf32 *sig_dev, size_t n_sig,
                               int scale_kind_fwd, float x_fwd, int scale_kind_bwd, float x_bwd);
/* The same chain followed by Modulation::demod_naive on its output (examples/modem.rs:28-31; BASELINE config 4's
 * receive side): only the bit bytes are written, `frames` is not modified.  BPSK / QPSK (table_host NULL = the generic
 * tables, `compat` as in aeth_demod_naive).  For plan lengths 1024 .. 4096 the decisions are taken in the chain's
 * registers; other lengths run the two steps through the plan's temp.  Same bits as aeth_fft_mul_ifft +
 * aeth_demod_naive. */
AETH_API int aeth_fft_mul_ifft_demod(aeth_fft *plan, const aeth_cf32 *frames_dev, size_t n_total, size_t batch,
                                     const aeth_cf32 *sig_dev, size_t n_sig, int scale_kind_fwd, float x_fwd,
                                     int scale_kind_bwd, float x_bwd, int bits_per_symbol,
                                     const aeth_cf32 *table_host, uint8_t *bits_out_dev, size_t nbits_out, int compat);

/* ---- FIR (src/fir.rs:3-22 holds taps + scratch but no filter method) ------- */
/* y[n] = sum_{k<ntaps} taps[k] * x[n-k] by overlap-save built from the
 * reference's own chain rfft -> vec_mul -> rifft(Scale::N).  taps are host
 * memory, copied.  fft_len must be a supported power of two >= 2*ntaps. */
AETH_API int aeth_fir_create(aeth_ctx *ctx, const aeth_cf32 *taps_host, size_t ntaps,
                             size_t fft_len, aeth_fir **out);
AETH_API int aeth_fir_destroy(aeth_fir *fir);
AETH_API size_t aeth_fir_ntaps(const aeth_fir *fir);
AETH_API size_t aeth_fir_fft_len(const aeth_fir *fir);
AETH_API size_t aeth_fir_hop(const aeth_fir *fir);      /* outputs per block (<= fft_len-ntaps+1) */
/* n outputs for n inputs.  hist_dev: NULL => zero initial state, else the
 * ntaps-1 samples preceding in_dev[0] (x[-(ntaps-1)] .. x[-1]).  The output range must not touch the input range
 * or the history (AETH_E_ARG): blocks run concurrently and read windows that reach into their neighbours', so ANY
 * overlap -- not only out == in -- would read samples already overwritten.  (Rust's &[T] / &mut [T] make that
 * unrepresentable on the reference side; the C ABI has to refuse it.) */
AETH_API int aeth_fir_exec(aeth_fir *fir, const aeth_cf32 *hist_dev, const aeth_cf32 *in_dev,
                           size_t n, aeth_cf32 *out_dev);
/* The filter followed by sampling::downsample (src/sampling.rs:28-42) in one pass: out[i] = y[i * dec] with
 * dec = n / n_out.  n % n_out != 0 -> AETH_E_ARG "Only even decimations are supported" (:32-36).  Bit-identical
 * to aeth_fir_exec + aeth_downsample; the output write traffic drops by dec.  fft_len 1024 .. 4096. */
AETH_API int aeth_fir_exec_decim(aeth_fir *fir, const aeth_cf32 *hist_dev, const aeth_cf32 *in_dev, size_t n,
                                 aeth_cf32 *out_dev, size_t n_out);
AETH_API int aeth_fir_exec_host(aeth_fir *fir, const aeth_cf32 *hist_host, const aeth_cf32 *in_host,
                                size_t n, aeth_cf32 *out_host);

/* ---- streaming correlator (listed as open in the reference) ------------------------------------ */
/* The reference lists "Add Correlation by Freq. Domain Convolution" as an open item (README.md:95); what it has is the
 * chain of its "correlator inplace" benchmark (benches/benches.rs:394-416), a circular correlation inside one frame --
 * aeth_fft_mul_ifft.  Run as overlap-save over a stream, that chain finds a template s of M = nref samples in x:
 *
 *     c[j] = sum_{k<M} conj(s[M-1-k]) * x[j-k]        j = 0 .. n-1
 *
 * the causal matched filter: exactly aeth_fir_exec with taps h[k] = conj(s[M-1-k]).  x[i] for i < 0 is zero, or comes
 * from hist_dev (the M-1 samples in front of in_dev[0]), as for the FIR.  An occurrence of s that starts at stream index
 * p peaks at j = p + M - 1, so lag = j - (M-1); with a history the lag can be as low as -(M-1).  Normalised
 * correlation (division by the local energy) is not computed.
 *
 * The object holds the filter built from the conj-reversed template and nothing else; create takes the length rules
 * and error codes of aeth_fir_create (fft_len a power of two in [2, 4096], fft_len >= 2*nref).  All three exec calls are
 * ordered on the context's in-order stream (never on the overlap lane) and validate everything before any device work. */
AETH_API int aeth_corr_create(aeth_ctx *ctx, const aeth_cf32 *ref_host, size_t nref, size_t fft_len, aeth_corr **out);
AETH_API int aeth_corr_destroy(aeth_corr *corr);
AETH_API size_t aeth_corr_nref(const aeth_corr *corr);
AETH_API size_t aeth_corr_fft_len(const aeth_corr *corr);
AETH_API size_t aeth_corr_hop(const aeth_corr *corr);     /* outputs per overlap-save block = samples per peak record */
/* out_dev[j] = c[j].  Any fft_len the FIR supports; bit-identical to aeth_fir_exec with the taps above, and refuses what
 * it refuses (output overlapping the input or the history: AETH_E_ARG; alignment: AETH_E_ALIGN) with the same texts. */
AETH_API int aeth_corr_exec(aeth_corr *corr, const aeth_cf32 *hist_dev, const aeth_cf32 *in_dev, size_t n,
                            aeth_cf32 *out_dev);
/* levels_dev[j] = level of c[j] (level kinds: see aeth_vec_levels).  Every overlap-save block stores a 4-byte level
 * where the 8-byte sample would go; c is never written: 8 B read + 4 B written per sample.  All three kinds are ONE pass
 * (the f64 logarithm of the two dB kinds runs in the fused kernel's registers).  Bit-identical to aeth_corr_exec into a
 * scratch buffer followed by aeth_vec_levels.  n_levels != n -> AETH_E_LEN; levels_dev 4-byte aligned (AETH_E_ALIGN) and
 * clear of the input and the history (AETH_E_ARG).  fft_len 1024 .. 4096 (AETH_E_UNSUPPORTED otherwise). */
AETH_API int aeth_corr_exec_levels(aeth_corr *corr, const aeth_cf32 *hist_dev, const aeth_cf32 *in_dev, size_t n,
                                   int level_kind, float *levels_dev, size_t n_levels);
/* Peak search in one pass: nothing of c goes to memory (8 B read per sample + 16 B written per block).  One record
 * per overlap-save block b, covering the outputs [b*hop, min((b+1)*hop, n)), under the rule of aeth_vec_stats:
 *   index  GLOBAL output index of the largest q(c[j]) of the block; the LOWEST index wins among equal q; a sample with
 *          a NaN component is no candidate
 *   norm   norm() of that sample
 *   n_nan  samples of the block with a NaN component
 * A block without a candidate reports index = n and norm = NaN.  16 bytes, no padding. */
struct aeth_corr_peak { size_t index; float norm; unsigned n_nan; };
/* peaks_dev (DEVICE memory, 8-byte aligned, clear of the input and the history) may be NULL; if it is not, n_peaks must
 * be ceil(n / hop) (AETH_E_LEN).  best_host may be NULL; if it is not, the call waits and returns the best record of the
 * whole stream under the same ordering with n_nan summed (saturating at UINT32_MAX).  Both NULL -> AETH_E_ARG; n == 0 ->
 * AETH_E_LEN.  The records equal aeth_vec_stats (max_index, max_norm, n_nan) of the matching slice of aeth_corr_exec's
 * output.  No floating-point atomics anywhere: bitwise reproducible from run to run.  fft_len 1024 .. 4096
 * (AETH_E_UNSUPPORTED otherwise).  The call's internal records live in the context (released by aeth_ctx_trim). */
AETH_API int aeth_corr_search(aeth_corr *corr, const aeth_cf32 *hist_dev, const aeth_cf32 *in_dev, size_t n,
                              struct aeth_corr_peak *peaks_dev, size_t n_peaks, struct aeth_corr_peak *best_host);

/* ---- LFSR sequences: src/sequence.rs:18-53 ------------------------------------------------------ */
/* sequence::generate(init, generator, len) (src/sequence.rs:47-53) runs any closure serially; every generator the reference
 * documents is a linear recurrence over GF(2) -- seq[n] = seq[n-d1] ^ seq[n-d2] ^ ... (the simple_sequence test, :61-68;
 * the LTE TS 36.211 7.2 example of the doc comment, :34-46; m-sequences, Gold codes).  For that class position p is
 * reached in O(log p) by powers of a 64 x 64 bit matrix, so the device generates any range [skip, skip + n) with every
 * wave starting on its own, and the consumers -- bits, XOR into a bit stream, chips, sign-flip spreading -- are fused
 * into the same pass: the sequence itself never touches memory.  All integer, all bit-exact.
 *
 * A register is a set of DISTINCT delays d_k in 1 .. 64; its order is max d_k.  `init` is a word whose bit i is seq[i]
 * for i < order, as sequence::expand(seed, order) gives it (:18-21); higher bits are ignored.  For n >= order
 * seq[n] = XOR_k seq[n - d_k]: sequence::generate(expand(init, order), |n, s| (sum s[n - d_k]) % 2, len).  Positions
 * below `order` return the init bits themselves; an all-zero init is legal and gives zeros.  A sequence object holds
 * 1 .. 4 registers and emits the XOR of their sequences at the same position (Gold codes: two).  skip is any uint64_t;
 * skip + n must not overflow (AETH_E_ARG).  Not mirrored here (the bindings do): generate returning `init` unchanged
 * when len <= init.len() (:48), and expand's shift overflow for len > 64 (:20). */
struct aeth_seq_reg { const uint32_t *delays; size_t ndelays; };
/* Host only -- no context, no device: the 64 sequence bits at [skip, skip + 64) of ONE register, bit i = seq[skip + i]. */
AETH_API int aeth_seq_window(const struct aeth_seq_reg *reg, uint64_t init, uint64_t skip, uint64_t *window);
/* Validates (null pointers; nregs outside 1 .. 4; ndelays outside 1 .. 64; a delay of 0 or above 64; repeated delays: all
 * AETH_E_ARG) before any device work, then keeps the matrix powers and uploads the device jump table once. */
AETH_API int aeth_seq_create(aeth_ctx *ctx, const struct aeth_seq_reg *regs, size_t nregs, aeth_seq **out);
AETH_API int aeth_seq_destroy(aeth_seq *seq);
AETH_API size_t aeth_seq_nregs(const aeth_seq *seq);
AETH_API size_t aeth_seq_order(const aeth_seq *seq, size_t reg);
AETH_API size_t aeth_seq_chunk(const aeth_seq *seq);   /* consecutive positions one wave generates from one jump-ahead */
/* Device calls, stream-ordered like every other device call.  `init` points to nregs words on the HOST and is read
 * before the call returns (the registers' windows at `skip` are computed on the host, in microseconds, and travel as
 * kernel arguments).  With c[i] the sequence bit at position skip + i (generate's output, src/sequence.rs:47-53):
 *   bits      out[i] = c[i], one byte per bit, values {0, 1}: the reference's Vec<u8> and aeth_modulate's input.
 *   scramble  out[i] = (in[i] & 1) ^ c[i]; out == in is allowed, any other overlap is AETH_E_ARG.
 *   chips     out[i] = c[i] ? one : zero, the two values copied bit for bit ((1,1) / (-1,-1): the reference's BPSK table,
 *             src/modulation.rs:77).
 *   spread    out[i] = sym[i / sf] with the sign bit of both components flipped where c[i] == 1: a multiplication by
 *             +-1 that is exact for -0.0 and NaN payloads too.  n_out != nsym * sf -> AETH_E_LEN; sf >= 1; sf == 1 with
 *             out == sym scrambles the symbols in place (twice: despreads), any other overlap is AETH_E_ARG.
 * bits and scramble take any byte alignment; cf32 pointers are 8-byte aligned (AETH_E_ALIGN).  n == 0 -> AETH_OK without
 * a launch.  At most 2^46 positions per call (AETH_E_UNSUPPORTED).  Everything is validated before any device work. */
AETH_API int aeth_seq_bits(aeth_seq *seq, const uint64_t *init, uint64_t skip, uint8_t *bits_dev, size_t n);
AETH_API int aeth_seq_scramble(aeth_seq *seq, const uint64_t *init, uint64_t skip, const uint8_t *in_dev, uint8_t *out_dev,
                               size_t n);
AETH_API int aeth_seq_chips(aeth_seq *seq, const uint64_t *init, uint64_t skip, aeth_cf32 zero, aeth_cf32 one,
                            aeth_cf32 *out_dev, size_t n);
AETH_API int aeth_seq_spread(aeth_seq *seq, const uint64_t *init, uint64_t skip, const aeth_cf32 *sym_dev, size_t nsym,
                             size_t sf, aeth_cf32 *out_dev, size_t n_out);
/* generate + download into a host slice; waits (sequence::generate's own shape, src/sequence.rs:47-53) */
AETH_API int aeth_host_seq_bits(aeth_seq *seq, const uint64_t *init, uint64_t skip, uint8_t *bits_host, size_t n);

/* ---- polyphase analysis filter bank (no body in the reference) --------------------------------- */
/* The reference cuts a stream into frames with chunks_mut(fft_len) (`waterfall`, src/util/plot.rs:46-68, :59-61):
 * disjoint, rectangular frames of exactly fft_len samples.  A receiver needs a window (so that a strong carrier does not
 * leak over the whole waterfall), overlap between frames (Welch / STFT) and a prototype filter longer than the
 * transform (the polyphase channelizer that splits a capture into M decimated channels).  All three are one operation:
 * weight L = P * M samples, fold them modulo M, transform M points, advance by the hop D.
 *   P = 1, D = M, w = 1   the reference's framing          P = 1, D < M   a windowed, overlapped spectrogram
 *   P > 1, D = M          the critically sampled channelizer   P > 1, D < M   the oversampled one
 * An aeth_chan is made of a REAL prototype w[0 .. L) (host floats, copied), channels = M, hop = D and a phase mode.
 * L = ntaps is a multiple of M, P = L / M in 1 .. 64, D in 1 .. M.
 *
 * The stream: s[i] = in_dev[i] for 0 <= i < n; for -(L - D) <= i < 0 it is hist_dev[L - D + i], or zero when hist_dev
 * is NULL (the FIR's convention; hist_dev is ignored when L == D).  n must be a multiple of D (AETH_E_LEN); the call
 * makes F = n / D frames.  Frame m ends with the D newest samples: it covers s[(m + 1) * D - L + j], j = 0 .. L - 1, so
 * the chunks of a stream concatenate exactly when the caller passes the previous L - D samples as history.
 *
 * The fold is defined bit for bit (f32, no contraction).  For q = 0 .. M - 1, with r = (q - rot) mod M:
 *     u_m[q] = sum over p = 0 .. P - 1, ascending, of  w[p * M + r] * s[(m + 1) * D - L + p * M + r]
 * every product rounded, the sum started from the p = 0 product (not from +0), products added left to right, re and im
 * independently.
 *   AETH_CHAN_PHASE_FRAME   rot = 0: the phase of every frame refers to its own first sample (STFT).
 *   AETH_CHAN_PHASE_STREAM  rot = ((g + 1) * D) mod M with g = first_frame + m the global frame number (g + 1 is reduced
 *                           modulo M before the multiplication: first_frame is any uint64_t).  Bin k is then the stream
 *                           mixed by exp(sign * 2 pi i k t / M), t counted from the first sample ever fed, filtered by w
 *                           and decimated by D: what an oversampled channelizer needs.  rot is 0 when D == M.
 * The transform: X_m = Scale * DFT_M(u_m), sign and Scale as for aeth_fft_exec, through an aeth_fft plan the object owns.
 *
 * All exec calls are ordered on the context's in-order stream and validate everything before any device work: NULL
 * pointers AETH_E_ARG; n == 0, n not a multiple of D, or an output count other than F * M AETH_E_LEN; cf32 pointers
 * 8-byte and level pointers 4-byte aligned (AETH_E_ALIGN); the output range clear of the input and the history
 * (AETH_E_ARG).  Element counts are size_t. */
enum { AETH_CHAN_PHASE_FRAME = 0, AETH_CHAN_PHASE_STREAM = 1 };
enum { AETH_CHAN_PROTO_RECT = 0, AETH_CHAN_PROTO_HANN = 1, AETH_CHAN_PROTO_HAMMING = 2, AETH_CHAN_PROTO_SINC_HAMMING = 3 };
/* No body in the reference (its framing, src/util/plot.rs:46-68, is the P = 1, D = M, w = 1 case).  The inner plan is
 * made by aeth_fft_create(ctx, channels, ...): a transform length it refuses fails here with its code and its message
 * naming the length, and nothing stays allocated.  P > 64: AETH_E_UNSUPPORTED; any other violation of the rules above:
 * AETH_E_ARG.  max_frames > 0 sizes the scratch of exec / exec_levels at creation; it grows on demand like the plan's. */
AETH_API int aeth_chan_create(aeth_ctx *ctx, const float *proto_host, size_t ntaps, size_t channels, size_t hop, int phase,
                              size_t max_frames, aeth_chan **out);
/* No body in the reference (src/util/plot.rs:46-68 frames without an object).  Waits for the context's stream. */
AETH_API int aeth_chan_destroy(aeth_chan *chan);
/* No body in the reference (src/util/plot.rs:46-68: fft_len is an argument there): M, L, D and the phase mode. */
AETH_API size_t aeth_chan_channels(const aeth_chan *chan);
AETH_API size_t aeth_chan_ntaps(const aeth_chan *chan);
AETH_API size_t aeth_chan_hop(const aeth_chan *chan);
AETH_API int aeth_chan_phase(const aeth_chan *chan);
/* No body in the reference (src/util/plot.rs:46-68 plans inside the call): the inner plan's aeth_fft_route text, owned
 * by the object. */
AETH_API const char *aeth_chan_route(const aeth_chan *chan);
/* No body in the reference (src/util/plot.rs:46-68): consecutive frames one workgroup (hop == M with P <= 8: one lane)
 * folds, like aeth_seq_chunk: the launch geometry, for tests that want to cross its edges. */
AETH_API size_t aeth_chan_tile(const aeth_chan *chan);
/* No body in the reference (src/util/plot.rs:46-68, chunks_mut(fft_len), is its w = 1, P = 1, D = M case): the front end
 * alone, out_dev[m * M + q] = u_m[q], n_out == F * M.  16 B per output sample when every input comes from HBM once. */
AETH_API int aeth_chan_fold(aeth_chan *chan, const aeth_cf32 *hist_dev, const aeth_cf32 *in_dev, size_t n,
                            uint64_t first_frame, aeth_cf32 *out_dev, size_t n_out);
/* No body in the reference (src/util/plot.rs:46-68 runs vec_rfft on disjoint chunks): the fold into the object's
 * scratch, then aeth_fft_exec of the F frames into out_dev; bit-identical to aeth_chan_fold followed by aeth_fft_exec. */
AETH_API int aeth_chan_exec(aeth_chan *chan, const aeth_cf32 *hist_dev, const aeth_cf32 *in_dev, size_t n,
                            uint64_t first_frame, int sign, int scale_kind, float x, aeth_cf32 *out_dev, size_t n_out);
/* No body in the reference (the whole `waterfall`, src/util/plot.rs:46-68, with a window and overlap): the fold into
 * scratch, then aeth_fft_exec_levels; bit-identical to aeth_chan_fold followed by aeth_fft_exec_levels, so the
 * register-resident power-of-two M never write the spectrum.  n_levels == F * M. */
AETH_API int aeth_chan_exec_levels(aeth_chan *chan, const aeth_cf32 *hist_dev, const aeth_cf32 *in_dev, size_t n,
                                   uint64_t first_frame, int sign, int scale_kind, float x, int mirror, int level_kind,
                                   float *levels_dev, size_t n_levels);
/* No body in the reference (src/util/plot.rs:46-68 has no window).  Host only, needs no context: L = channels *
 * taps_per_channel taps, computed in f64 and rounded once to f32, n = 0 .. L - 1:
 *   RECT          1
 *   HANN          0.5 - 0.5 cos(2 pi n / L)        (periodic)
 *   HAMMING       0.54 - 0.46 cos(2 pi n / L)      (periodic)
 *   SINC_HAMMING  the low-pass of cutoff fs / (2 M): sinc((n - (L - 1) / 2) / M) * (0.54 - 0.46 cos(2 pi n / (L - 1))),
 *                 divided by its f64 sum (unit DC gain); L = 1 gives 1
 * A bad kind or a zero size: AETH_E_ARG. */
AETH_API int aeth_chan_prototype(int kind, size_t channels, size_t taps_per_channel, float *out_host);

/* ---- averaged spectra: per-bin power sums and max hold over frames (no body in the reference) ---- */
/* The reference's `waterfall` (src/util/plot.rs:46-68) keeps the level of every bin of every frame.  Welch's averaged
 * periodogram and the max-hold trace of a spectrum analyser keep ONE row of `len` numbers per `block` frames; the
 * reduction over the frames is done here in f64, in an order that is part of the contract.
 *
 * Frames m = 0 .. F - 1 of len = M bins; q_m[k] = q(X_m[k]) = (double)re * re + (double)im * im of the bin (one f64
 * rounding, as for aeth_vec_stats) exactly as aeth_chan_exec / aeth_fft_exec would have stored it: scaled, and (where a
 * call has a `mirror` argument and it is not 0) after vec_mirror of the frame.
 *   rows    block = B frames per output row, 0 (or more than F) means one row over the whole call.  R = ceil(F / B); row r
 *           covers frames [r B, min(F, (r + 1) B)).
 *   chunks  a row is cut into chunks of C >= 1 frames counted from the row's first frame; the last chunk of a row may
 *           be short.
 *   sum     a chunk's sum starts from its first frame's q and adds the following frames' q in ascending order; the row's
 *           sum starts from chunk 0's sum and adds the following chunk sums in ascending order.  Every addition is one f64
 *           rounding.  NaN and +inf are carried the ordinary way.
 *   max     best = -inf; best = q > best ? q : best over the row's frames: a NaN q never enters, a column of NaNs gives
 *           -inf.  The rule is associative and commutative, so its tree is free.
 * The bytes of both planes are a function of the frames, B and C only: not of the CU count, pointer alignment, cache
 * policy (AETH_NT), which planes are requested, or the route taken.  A stream cut at a multiple of B frames and continued
 * with history gives the same rows.  There are no atomics; chunk results live in a scratch buffer of the context that
 * aeth_ctx_trim releases, and go straight to the caller's planes when a row is one chunk.
 *
 * Not built: a min-hold plane, exponential averaging, a one-kernel route for P > 1 or the stream phase, an
 * aeth_stream_op kind, host-slice flavours. */
enum { AETH_SUMS_GENERAL = 1 };          /* aeth_chan_exec_sums flag: never take the fused route (verification, measurement) */
/* No body in the reference (src/util/plot.rs:46-68 keeps every frame): the reduction alone over F = n / len frames of
 * cf32 in device memory, chunk = C.  sum_dev / max_dev: R * len doubles each, either may be NULL, not both; n_out ==
 * R * len.  A lane owns two adjacent columns (16-byte loads) or, for an odd len or a base that is only 8-byte aligned, one
 * column (8-byte loads).  Everything is refused before any device work: NULL ctx, frames or both planes AETH_E_ARG; n == 0,
 * len == 0, n not a multiple of len, chunk == 0 or a wrong n_out AETH_E_LEN; pointers not 8-byte aligned AETH_E_ALIGN; a plane
 * that overlaps the input or the other plane AETH_E_ARG.  Ordered on the context's in-order stream; does not wait. */
AETH_API int aeth_vec_frame_sums(aeth_ctx *ctx, const aeth_cf32 *frames_dev, size_t n, size_t len, size_t block, size_t chunk,
                                 double *sum_dev, double *max_dev, size_t n_out);
/* No body in the reference (src/util/plot.rs:46-68): the frames of aeth_chan_exec -- same framing, history, sign, Scale and
 * checks as aeth_chan_exec_levels -- reduced as above with C = aeth_chan_sums_chunk(chan); n_out == R * M.  By contract
 * byte-identical to aeth_chan_exec (then aeth_vec_mirror_frames if mirror != 0) followed by aeth_vec_frame_sums with that
 * chunk.  Two routes, the same bytes:
 *   fused    power-of-two M = 512 .. 4096 with ntaps == M and rot = 0 (AETH_CHAN_PHASE_FRAME, or hop == M): one kernel --
 *            window, register transform, q and the f64 accumulation per chunk -- plus the row fold: 8 bytes read per
 *            input sample, the spectrum is never written.
 *   general  every other (M, P, D), phase mode and plan route aeth_chan_create accepts (smaller power-of-two M included),
 *            and every shape under AETH_SUMS_GENERAL: fold, transform, chunk sums in slices of whole chunks through a
 *            bounded scratch, then the row fold.
 * flags: AETH_SUMS_GENERAL or 0; unknown bits AETH_E_ARG. */
AETH_API int aeth_chan_exec_sums(aeth_chan *chan, const aeth_cf32 *hist_dev, const aeth_cf32 *in_dev, size_t n,
                                 uint64_t first_frame, int sign, int scale_kind, float x, int mirror, size_t block, int flags,
                                 double *sum_dev, double *max_dev, size_t n_out);
/* No body in the reference: the frames per chunk of aeth_chan_exec_sums, like aeth_chan_tile: the launch geometry, for
 * tests that want to cross its edges.  A function of M alone (16 Ki bins: 8 .. 32 frames); 0 for NULL. */
AETH_API size_t aeth_chan_sums_chunk(const aeth_chan *chan);
/* No body in the reference: 1 if aeth_chan_exec_sums without AETH_SUMS_GENERAL takes the one-kernel route. */
AETH_API int aeth_chan_sums_fused(const aeth_chan *chan);
/* No body in the reference (util/plot.rs:65,127 takes the level of one bin): what a plot draws of a plane.
 * qbar = q_dev[i] / count (one f64 division), then the level formulas of aeth_vec_levels applied to qbar:
 *   NORM (float)sqrt(qbar); DB (float)(10 log10((double)(float)sqrt(qbar))); POWER_DB (float)(10 log10(qbar)).
 * count is the number of frames of a row for the sum plane, 1 for the max plane; it must be finite and > 0 (AETH_E_ARG).
 * n == 0 -> AETH_OK without a launch; q_dev 8-byte, levels_dev 4-byte aligned (AETH_E_ALIGN); no overlap (AETH_E_ARG). */
AETH_API int aeth_vec_sum_levels(aeth_ctx *ctx, const double *q_dev, size_t n, double count, int level_kind, float *levels_dev);

/* ---- polyphase synthesis filter bank (no body in the reference) -------------------------------- */
/* The transpose of aeth_chan: what puts a stream back together after aeth_chan_exec took it apart (the reference only
 * takes apart: `waterfall`, src/util/plot.rs:46-68).  Every frame's M time samples (an inverse transform of its M bins)
 * are extended periodically to L = P * M, weighted by a synthesis prototype and overlap-added at the hop D:
 *   P = 1, D < M   the inverse STFT (weighted overlap-add)     P > 1   the polyphase synthesis bank, a transmultiplexer
 * An aeth_synth is made of a REAL prototype g[0 .. L) (host floats, copied), channels = M, hop = D and a phase mode
 * (AETH_CHAN_PHASE_FRAME / _STREAM).  L = ntaps is a multiple of M, P = L / M in 1 .. 64, D in 1 .. M.
 * K = ceil(L / D) frames touch one output sample; K > 256 is refused (AETH_E_UNSUPPORTED).
 *
 * The frames: v_m[q] = frames_dev[m * M + q] for m = 0 .. F - 1, n_in = F * M.  The K - 1 frames in front of them,
 * m = -(K - 1) .. -1, are hist_dev[(m + K - 1) * M + q] (oldest frame first), or frames of +0.0 when hist_dev is NULL:
 * those are multiplied like any other frame.  hist_dev is ignored when K == 1.  The call writes F * D samples.
 *
 * The overlap-add is defined bit for bit (f32, no contraction).  For i = 0 .. F * D - 1:
 *     out[i] = sum over m, ascending, with 0 <= i - m * D < L, of  g[j] * v_m[(j + rot_m) mod M],   j = i - m * D
 * every product rounded, the sum started from the first product (not from +0), products added oldest frame first, re and
 * im independently, each as a real multiplication by g[j].  A frame that does not reach i adds nothing, not even a zero.
 *   AETH_CHAN_PHASE_FRAME   rot_m = 0.
 *   AETH_CHAN_PHASE_STREAM  rot_m = ((G + 1) * D) mod M with G = first_frame + m reduced modulo M (to 0 .. M - 1, also
 *                           for the history's frame numbers below zero when first_frame is 0).  rot is 0 when D == M.
 * This is the transpose of aeth_chan_fold: the analysis' frame m covers s[(m + 1) * D - L + j], the synthesis puts it at
 * m * D + j, so the output is the reconstruction DELAYED by L - D samples.  Every output is complete within its call:
 * the chunks of a stream concatenate exactly when the caller passes the previous K - 1 frames as history.
 *
 * All calls are ordered on the context's in-order stream and validate everything before any device work: NULL pointers
 * AETH_E_ARG; n_in == 0, n_in not a multiple of M, or n_out other than F * D AETH_E_LEN; pointers 8-byte aligned
 * (AETH_E_ALIGN); the output range clear of the input and the history (AETH_E_ARG).  Element counts are size_t. */
/* No body in the reference (src/util/plot.rs:46-68 never resynthesizes).  The inner plan is made by
 * aeth_fft_create(ctx, channels, ...): a transform length it refuses fails here with its code and its message naming the
 * length, and nothing stays allocated.  P > 64 or K > 256: AETH_E_UNSUPPORTED; any other violation of the rules above:
 * AETH_E_ARG.  max_frames > 0 sizes the scratch of exec at creation; it grows on demand like the plan's. */
AETH_API int aeth_synth_create(aeth_ctx *ctx, const float *proto_host, size_t ntaps, size_t channels, size_t hop, int phase,
                               size_t max_frames, aeth_synth **out);
/* No body in the reference (src/util/plot.rs:46-68 frames without an object).  Waits for the context's stream. */
AETH_API int aeth_synth_destroy(aeth_synth *synth);
/* No body in the reference (src/util/plot.rs:46-68: fft_len is an argument there): M, L, D and the phase mode. */
AETH_API size_t aeth_synth_channels(const aeth_synth *synth);
AETH_API size_t aeth_synth_ntaps(const aeth_synth *synth);
AETH_API size_t aeth_synth_hop(const aeth_synth *synth);
AETH_API int aeth_synth_phase(const aeth_synth *synth);
/* No body in the reference (src/util/plot.rs:46-68 plans inside the call): the inner plan's aeth_fft_route text, owned
 * by the object. */
AETH_API const char *aeth_synth_route(const aeth_synth *synth);
/* No body in the reference (src/util/plot.rs:46-68): consecutive hops one lane (D == M with P <= 8, or D < M dividing L
 * with K <= 8) or one workgroup (every other shape) makes, like aeth_chan_tile: the launch geometry, for tests that
 * want to cross its edges. */
AETH_API size_t aeth_synth_tile(const aeth_synth *synth);
/* No body in the reference (src/util/plot.rs:46-68 has no overlap): K - 1, the frames of history a call reads. */
AETH_API size_t aeth_synth_history(const aeth_synth *synth);
/* No body in the reference (src/util/plot.rs:46-68 has no way back to a stream): the back end alone, as defined above.
 * 8 * M bytes read and 8 * D written per frame when every frame comes from HBM once. */
AETH_API int aeth_synth_unfold(aeth_synth *synth, const aeth_cf32 *hist_dev, const aeth_cf32 *frames_dev, size_t n_in,
                               uint64_t first_frame, aeth_cf32 *out_dev, size_t n_out);
/* No body in the reference (src/util/plot.rs:46-68 only transforms forward): hist_dev and spec_dev hold SPECTRA.
 * aeth_fft_exec of the K - 1 history frames (when given) and of the F frames into the object's scratch of
 * (K - 1 + F) * M samples, then the unfold; bit-identical to those aeth_fft_exec calls followed by aeth_synth_unfold. */
AETH_API int aeth_synth_exec(aeth_synth *synth, const aeth_cf32 *hist_dev, const aeth_cf32 *spec_dev, size_t n_in,
                             uint64_t first_frame, int sign, int scale_kind, float x, aeth_cf32 *out_dev, size_t n_out);
/* No body in the reference (src/util/plot.rs:46-68 has no window).  Host only, needs no context: the synthesis window
 * that inverts a windowed, overlapped transform (P = 1, ntaps = M), j = 0 .. ntaps - 1:
 *     g[j] = w[j] / sum over j' = j (mod hop), 0 <= j' < ntaps, of w[j']^2
 * computed in f64 and rounded once to f32.  With it aeth_chan_exec (sign -1) followed by aeth_synth_exec (sign +1,
 * AETH_SCALE_N) returns the stream, delayed by ntaps - hop.  A null pointer, a zero size, hop > ntaps or a denominator
 * below 2^-20 (the periodic Hann window at hop == ntaps): AETH_E_ARG, the message names j; nothing is written. */
AETH_API int aeth_synth_dual_window(const float *w, size_t ntaps, size_t hop, float *out_host);

/* ---- polyphase rational resampler (no body in the reference) ----------------------------------- */
/* A stream converted by the ratio U / Q with a proper anti-alias / anti-image filter: upsample by U (zero stuffing),
 * filter with a real FIR h, keep every Q-th sample, in one pass (the reference's rate changes, src/sampling.rs:7-62, are
 * linear interpolation and sample picking).
 * An aeth_resamp is made of a REAL prototype h[0 .. T) (host floats, copied), up = U and down = Q.  T = ntaps is a
 * multiple of U, with P = T / U taps per phase.  U and Q are taken as given: a common factor is not reduced, because the
 * taps refer to the U that was passed.  U and Q in 1 .. 4096, P in 1 .. 64.
 *
 * The stream: s[i] = in_dev[i] for 0 <= i < n; for -(P - 1) <= i < 0 it is hist_dev[P - 1 + i].  When hist_dev is NULL
 * those samples are +0.0: they are multiplied like any others, as in aeth_synth.  hist_dev is ignored when P == 1.
 * n must be a multiple of Q.  A call over n = B * Q samples writes exactly B * U outputs: every call therefore starts at
 * phase 0, and no stream position has to be passed.
 *
 * The output is defined bit for bit (f32, no contraction).  For k = 0 .. B * U - 1, with a = floor(k * Q / U) and
 * r = (k * Q) mod U:
 *     out[k] = sum over p = 0 .. P - 1, ascending, of  h[p * U + r] * s[a - p]
 * every product rounded, the sum started from the p = 0 product (not from +0), products added left to right, re and im
 * independently, each as a real multiplication by the tap.  a <= n - 1 always holds, so every output is complete within
 * its call: the chunks of a stream concatenate bit for bit when the caller passes the previous P - 1 input samples as
 * history.
 *
 * aeth_resamp_exec is ordered on the context's in-order stream and validates everything before any device work: NULL
 * pointers AETH_E_ARG; n == 0, n not a multiple of Q, or n_out other than n / Q * U AETH_E_LEN; pointers 8-byte aligned
 * (AETH_E_ALIGN); the output range clear of the input and the history (AETH_E_ARG); an element count or a grid that
 * would overflow (n above SIZE_MAX / 16 / U, 2^31 workgroups) AETH_E_UNSUPPORTED.  Element counts are size_t. */
/* No body in the reference (src/sampling.rs:7-62 has only linear interpolation and sample picking).  ntaps == 0, ntaps
 * not a multiple of up, up == 0 or down == 0: AETH_E_ARG; P > 64, up > 4096 or down > 4096: AETH_E_UNSUPPORTED; the
 * message names the offending number, and nothing stays allocated. */
AETH_API int aeth_resamp_create(aeth_ctx *ctx, const float *taps_host, size_t ntaps, size_t up, size_t down, aeth_resamp **out);
/* No body in the reference (src/sampling.rs:7-62 resamples without an object).  Waits for the context's stream. */
AETH_API int aeth_resamp_destroy(aeth_resamp *resamp);
/* No body in the reference (src/sampling.rs:7-62: the factor is an argument there): U, Q and T; 0 for a null handle. */
AETH_API size_t aeth_resamp_up(const aeth_resamp *resamp);
AETH_API size_t aeth_resamp_down(const aeth_resamp *resamp);
AETH_API size_t aeth_resamp_ntaps(const aeth_resamp *resamp);
/* No body in the reference (src/sampling.rs:7-62 keeps no state between calls): P - 1, the input samples of history a
 * call reads. */
AETH_API size_t aeth_resamp_history(const aeth_resamp *resamp);
/* No body in the reference (src/sampling.rs:7-62): consecutive outputs one workgroup makes, like aeth_chan_tile: the
 * launch geometry, for tests that want to cross its edges. */
AETH_API size_t aeth_resamp_tile(const aeth_resamp *resamp);
/* No body in the reference (src/sampling.rs:7-62 has one loop): the kernel route, text owned by the object: "staged"
 * (the inputs of a tile of outputs go through LDS once) or "direct" (strong decimation: every output reads its own P
 * samples), followed by " u1" when up == 1 (one tap row for every lane).  "" for a null handle. */
AETH_API const char *aeth_resamp_route(const aeth_resamp *resamp);
/* No body in the reference (src/sampling.rs:7-62 sizes its output inside the call): n_in / Q * U, or 0 when n_in is not
 * a multiple of Q, would overflow, or the handle is null. */
AETH_API size_t aeth_resamp_out_count(const aeth_resamp *resamp, size_t n_in);
/* No body in the reference (src/sampling.rs:7-62 has only linear interpolation and sample picking): the resampler as
 * defined above.  8 n bytes read and 8 n U / Q written when every input comes from HBM once. */
AETH_API int aeth_resamp_exec(aeth_resamp *resamp, const aeth_cf32 *hist_dev, const aeth_cf32 *in_dev, size_t n,
                              aeth_cf32 *out_dev, size_t n_out);
/* No body in the reference (src/sampling.rs:7-62 has no filter).  Host only, needs no context: L = up * taps_per_phase
 * taps of the low-pass with cutoff 1 / (2 c) cycles per upsampled sample, c = max(up, down), n = 0 .. L - 1:
 *     sinc((n - (L - 1) / 2) / c) * (0.54 - 0.46 cos(2 pi n / (L - 1)))
 * scaled so that the taps sum to `up` (unit passband gain after zero stuffing), computed in f64 and rounded once to f32;
 * the second half mirrors the first bit for bit.  L == 1 gives 1.  A zero size or a null pointer: AETH_E_ARG. */
AETH_API int aeth_resamp_prototype(size_t up, size_t down, size_t taps_per_phase, float *out_host);

/* ---- arbitrary-ratio resampler: integer time word, interpolated taps (no body in the reference) -- */
/* A stream converted by a ratio that is no small fraction: a sample clock some parts per million off, a symbol rate that
 * is no simple fraction of the capture rate, 48 kHz to 44.1 kHz * (1 + 20 ppm).  A polyphase bank of L = 2^b phases whose
 * taps are linearly interpolated between neighbouring phases, addressed by a 64-bit fixed-point time word (the
 * reference's rate changes, src/sampling.rs:7-62, are linear interpolation and sample picking).
 *
 * Object.  An aeth_arb is made of a REAL prototype h[0 .. T) (host floats, copied): T = ntaps = P * L, L = 2^b,
 * b = log2_phases in 0 .. 12, P in 1 .. 64.  h[T] := +0.0, so the continuous impulse response ends at zero, and
 *     d[j] = fl32(h[j + 1] - h[j])    for j = 0 .. T - 1
 * computed on the host in f32 and rounded once.  aeth_resamp_prototype(L, down, P) designs a suitable low-pass; for a
 * decimating ratio take down = ceil(L * step).
 *
 * Time word.  Time is unsigned Q32.32 in a uint64_t: the top 32 bits are the input sample index relative to the call's
 * first sample, the low 32 bits the fraction.  Output m of a call sits at t(m) = phase + m * step, `step` being the input
 * samples per output sample, in [2^20, 2^44]: 1/4096 to 4096.  step and phase are arguments of a call, not part of the
 * object: a tracking loop may change step between chunks.
 *
 * The stream, as for aeth_resamp: s[i] = in_dev[i] for 0 <= i < n; for -(P - 1) <= i < 0 it is hist_dev[P - 1 + i].  When
 * hist_dev is NULL those samples are +0.0, multiplied like any others.  hist_dev is ignored when P == 1.
 *
 * Output count and next phase.  A call over n inputs makes every output whose newest sample is inside the call: all
 * m >= 0 with t(m) < n * 2^32.
 *     count = 0 if phase >= n * 2^32, else ceil((n * 2^32 - phase) / step)
 *     next phase = phase + count * step - n * 2^32
 * Both come from aeth_arb_advance.  n == 0 is a valid call that makes nothing.
 *
 * The sample is defined bit for bit.  Every operation is f32 and rounded on its own (no contraction).  For output m:
 *     a = t >> 32        f = (uint32)t        r = b ? f >> (32 - b) : 0
 *     mu24 = ((uint32)(f << b)) >> 8          mu = (float)mu24 * 2^-24           (exact)
 *     j_p = p * L + r
 *     c_p = h[j_p] + mu * d[j_p]                                      (the product rounded, then the sum rounded)
 *     out[m] = sum over p = 0 .. P - 1, ascending, of  c_p * s[a - p]
 * every product rounded, the sum started from the p = 0 product (not from +0), products added left to right, re and im
 * independently, each as a real multiplication by c_p.  a <= n - 1 always holds, so every output is complete within its
 * call: chunks cut anywhere concatenate bit for bit when the caller passes the previous P - 1 input samples as history
 * and the phase from aeth_arb_advance.  With step = Q * 2^32 / L exact and phase 0, mu is always 0 and the values are
 * those of aeth_resamp_exec with (up = L, down = Q) and the same taps (a tap of -0.0 becomes +0.0).
 *
 * aeth_arb_exec is ordered on the context's in-order stream and validates everything before any device work: NULL
 * pointers AETH_E_ARG; step, phase or n that aeth_arb_advance refuses AETH_E_UNSUPPORTED; n_out other than count
 * AETH_E_LEN; pointers 8-byte aligned (AETH_E_ALIGN); the output range clear of the input and the history (AETH_E_ARG);
 * 2^31 workgroups or more AETH_E_UNSUPPORTED.  n_out == 0 in a valid call returns AETH_OK without a launch: a short chunk
 * under strong decimation legitimately makes nothing. */
/* No body in the reference (src/sampling.rs:7-62 has no time word).  Host only, needs no context: count and next phase
 * as defined above, in unsigned 128-bit arithmetic.  AETH_E_UNSUPPORTED, the message naming the number: step outside
 * [2^20, 2^44]; phase >= 2^63; n > 2^31; any intermediate of 2^64 or more (none is left once the first three hold).  A
 * null result pointer: AETH_E_ARG.  Nothing is written when the call is refused. */
AETH_API int aeth_arb_advance(uint64_t step, uint64_t phase, size_t n, size_t *count, uint64_t *next_phase);
/* No body in the reference (src/sampling.rs:7-62 has only linear interpolation and sample picking).  NULL pointers,
 * ntaps == 0 or ntaps not a multiple of 2^log2_phases: AETH_E_ARG; log2_phases > 12 or P > 64: AETH_E_UNSUPPORTED; the
 * message names the offending number, every check comes before the context is used, and nothing stays allocated. */
AETH_API int aeth_arb_create(aeth_ctx *ctx, const float *taps_host, size_t ntaps, size_t log2_phases, aeth_arb **out);
/* No body in the reference (src/sampling.rs:7-62 resamples without an object).  Waits for the context's stream. */
AETH_API int aeth_arb_destroy(aeth_arb *arb);
/* No body in the reference (src/sampling.rs:7-62: the factor is an argument there): L and T; 0 for a null handle. */
AETH_API size_t aeth_arb_phases(const aeth_arb *arb);
AETH_API size_t aeth_arb_ntaps(const aeth_arb *arb);
/* No body in the reference (src/sampling.rs:7-62 keeps no state between calls): P - 1, the input samples of history a
 * call reads. */
AETH_API size_t aeth_arb_history(const aeth_arb *arb);
/* No body in the reference (src/sampling.rs:7-62): consecutive outputs one workgroup makes at this step, like
 * aeth_resamp_tile: the largest multiple of 256, at most 4096, with floor((2^32 - 1 + (tile - 1) * step) / 2^32) + P <=
 * 4096 samples, so that a tile's input span fits 32 KiB of LDS whatever the fraction of its first output is; 256 on the
 * direct route.  0 for a null handle or a step out of range. */
AETH_API size_t aeth_arb_tile(const aeth_arb *arb, uint64_t step);
/* No body in the reference (src/sampling.rs:7-62 has one loop): the kernel route at this step, static text: "staged" (the
 * inputs of a tile of outputs go through LDS once), followed by " tab" when the tap table, L rows of ceil(P / 2) 16-byte
 * slots, is at most 512 slots and lies in LDS as well, or "direct" (not even 256 outputs fit the span, which includes
 * every step that skips inputs: each output reads its own P samples).  "" for a null handle or a step out of range. */
AETH_API const char *aeth_arb_route(const aeth_arb *arb, uint64_t step);
/* No body in the reference (src/sampling.rs:7-62 has only linear interpolation and sample picking): the resampler as
 * defined above.  8 n bytes read and 8 n_out written when every input comes from HBM once. */
AETH_API int aeth_arb_exec(aeth_arb *arb, const aeth_cf32 *hist_dev, const aeth_cf32 *in_dev, size_t n, uint64_t step,
                           uint64_t phase, aeth_cf32 *out_dev, size_t n_out);

/* ---- numerically controlled oscillator: frequency shift, tone, chirp (no body in the reference) -- */
/* The multiplication of a stream by e^{j phi(n)}: what brings a channel at an offset to baseband in front of
 * aeth_resamp_exec, removes a carrier offset behind aeth_corr_search, and makes test tones and sounding chirps on the
 * device (the reference has no oscillator; its only phasors are the FFT's twiddles).
 *
 * An oscillator is three words, each a fraction of a turn scaled by 2^64: `phase`, `step` (turns per sample) and `rate`
 * (turns per sample per sample).  The phase word of sample n, n a uint64_t stream position, is
 *     w(n) = phase + n * step + T(n) * rate        (mod 2^64: plain unsigned wrap-around)
 *     T(n) = n (n - 1) / 2, computed as (n / 2) * (n - 1) for even n and n * ((n - 1) / 2) for odd n
 * which is exact for every n in [0, 2^64): a float phase accumulator drifts with the stream position, an integer word
 * cannot.  The instantaneous frequency from sample n to n + 1 is step + n * rate; rate == 0 is the plain shifter.
 *
 * The phasor (c, d) of a word is defined bit for bit.  Every operation is f32 and rounded on its own (no contraction):
 *     t = w >> 32                                   (uint32)
 *     k = ((t + 0x20000000) >> 30) & 3              (uint32 wrap-around: the nearest quarter turn)
 *     r = (int32)(t - (k << 30))                    (uint32 wrap-around, reinterpreted: -2^29 <= r < 2^29)
 *     a = (float)r * K          K = 0x1.921fb6p-30f, the f32 nearest 2 pi / 2^32; int -> float rounds to nearest even
 *     s = a * a
 *     ps = (S3 * s + S2) * s + S1          sn = (a * s) * ps + a
 *     pc = (C3 * s + C2) * s + C1          cs = (1 - 0.5 * s) + (s * s) * pc
 *     S1, S2, S3 = -1.6666654611e-1, 8.3321608736e-3, -1.9515295891e-4                   (each rounded once to f32)
 *     C1, C2, C3 = 4.166664568298827e-2, -1.388731625493765e-3, 2.443315711809948e-5
 *     (c, d) = (cs, sn), (-sn, cs), (-cs, -sn), (sn, -cs)     for k = 0, 1, 2, 3
 * (the classic single-precision minimax pair on [-pi/4, pi/4]).  The words 0, 2^62, 2^63 and 3 * 2^62 give exactly
 * (1, 0), (-0, 1), (-1, -0) and (0, -1).  Against exp(2 pi j w / 2^64) in f64 the phasor is within 1.5e-7.
 *
 *   mix    out[i].re = x.re * c - x.im * d,  out[i].im = x.re * d + x.im * c,  x = in[i], (c, d) the phasor of w(n0 + i):
 *          aeth_vec_mul's expression with the phasor as the second operand
 *   tone   out[i] = (amp * c, amp * d)
 * Each output depends only on in[i] and the words: a stream cut anywhere and continued with n0 advanced by the cut gives
 * the same bits.
 *
 * aeth_nco_mix and aeth_nco_tone are ordered on the context's in-order stream like the element-wise calls and validate
 * everything before any device work: NULL ctx, words or pointers AETH_E_ARG (n == 0 returns AETH_OK without a launch
 * once ctx and words are there, as for aeth_seq_*); pointers 8-byte aligned (AETH_E_ALIGN); n0 > UINT64_MAX - n
 * AETH_E_UNSUPPORTED, the message naming both numbers; 2^31 workgroups or more AETH_E_UNSUPPORTED; out_dev == in_dev runs
 * in place, any other overlap of the two ranges AETH_E_ARG. */
typedef struct aeth_nco_words { uint64_t phase, step, rate; } aeth_nco_words;
/* No body in the reference.  Host only: the word of `cycles` turns (or turns per sample).  With x = cycles -
 * floor(cycles) in f64 it is x * 2^64 truncated toward zero; 0 when x rounds to 1.0 and for NaN or +-Inf.  A negative
 * frequency is its two's complement: aeth_nco_word(-0.25) == 3 * 2^62. */
AETH_API uint64_t aeth_nco_word(double cycles);
/* No body in the reference.  Host only: w(n) as defined above; 0 for a null pointer. */
AETH_API uint64_t aeth_nco_word_at(const aeth_nco_words *w, uint64_t n);
/* No body in the reference.  Host only: the phasor of one word, by the same text the kernels run.  out_host NULL:
 * AETH_E_ARG. */
AETH_API int aeth_nco_phasor(uint64_t word, aeth_cf32 *out_host);
/* No body in the reference: the mix as defined above, 8 B read and 8 B written per sample. */
AETH_API int aeth_nco_mix(aeth_ctx *ctx, const aeth_nco_words *w, uint64_t n0, const aeth_cf32 *in_dev, aeth_cf32 *out_dev,
                          size_t n);
/* No body in the reference: the tone (a chirp when rate != 0) as defined above, 8 B written per sample. */
AETH_API int aeth_nco_tone(aeth_ctx *ctx, const aeth_nco_words *w, uint64_t n0, float amp, aeth_cf32 *out_dev, size_t n);

/* ---- synchronisation estimators (no body in the reference) ---- */
/* What tells a receiver the offsets that aeth_nco_mix and aeth_arb_exec remove: the classical feed-forward estimators,
 * each a read-only reduction over a device-resident stream (8 B per sample), none of whose samples leaves the device.
 *   symbol timing      the spectral line of the square law at the symbol rate (Oerder and Meyr): aeth_sync_line with
 *                      AETH_SYNC_SQUARE and step = aeth_nco_word(-1 / sps); aeth_sync_timing_phase turns it into the
 *                      aeth_arb_exec phase of the first symbol instant
 *   carrier phase      the M-th power sum: aeth_sync_line with AETH_SYNC_POW<M> (and NULL words); turns / M is the phase
 *                      of the carrier, up to the M-fold ambiguity and the constellation's own angle
 *   carrier frequency  the delay-and-multiply sum of the M-th power: aeth_sync_lag; aeth_sync_freq_step turns it into the
 *                      aeth_nco_words.step that removes the offset
 *
 * The terms are defined bit for bit.  Every f32 operation is rounded on its own (no contraction):
 *     sq(a)    = (a.re * a.re - a.im * a.im,  (a.re * a.im) + (a.re * a.im))
 *     pw_M(x)  = x, sq(x), sq(sq(x)), sq(sq(sq(x)))               for M = 1, 2, 4, 8
 *     q(c)     = (double)c.re * c.re + (double)c.im * c.im         as for aeth_vec_stats
 * and every f64 expression below multiplies values that came from f32, so each product is exact and each line is ONE
 * rounding, the same bits with or without fma.
 *   line term i   (c, d) = the phasor of w(n0 + i), w as defined for the oscillator above (chirp term included; NULL
 *                 words are three zeros, whose phasor is exactly (1, +0)), widened to f64
 *                 AETH_SYNC_SQUARE:  f = q(x_i);  t = (f * c, f * d);  weight f
 *                 AETH_SYNC_POW<M>:  z = pw_M(x_i) widened;  t.re = z.re * c - z.im * d,  t.im = z.re * d + z.im * c;
 *                                    weight q(z)
 *   lag term i    a = pw_M(x_i), b = pw_M(x_{i - L}), both widened, L = lag >= 1:
 *                 t.re = a.re * b.re + a.im * b.im,  t.im = a.im * b.re - a.re * b.im;  weight q(a)
 *                 (t = a * conj(b)).  For i < L, x_{i - L} is hist_dev[L + (i - L)] = hist_dev[i]: the L samples in front
 *                 of the call, the library's usual history.  With hist_dev NULL the terms i < L do not exist: they are
 *                 neither summed nor counted in n.
 * A record holds the sum of its terms (re, im), the sum of their weights (mass: |sum| / mass is the strength of the
 * line, 1 for a noise-free constant-modulus signal on the line), the number of terms and the number of terms with a NaN
 * or infinite re or im.  Those terms ARE summed: IEEE decides the sum, n_nonfinite tells why.
 *
 * Blocks.  The n samples of a call are cut into blocks of `block` samples (0: one block of n), the last one may be short;
 * term i belongs to block i / block and rec_dev receives ceil(n / block) records, one per block.  Any block >= 1 is
 * accepted; blocks shorter than aeth_sync_chunk() samples take a whole workgroup each and may be slow.
 *
 * The order of the additions is a function of the index inside the block and of the block's length only.  A block of
 * `len` samples is cut into chunks of C = aeth_sync_chunk() = 4096 samples, the last one short.  Inside a chunk of `left`
 * samples the pair (2 p, 2 p + 1) with 2 p + 1 < left belongs to lane p % 256, round p / 256; the last sample of an odd
 * `left` belongs to lane ((left - 1) / 2) % 256.
 *   1. a lane starts re, im and mass from -0.0 -- the identity of IEEE addition, so the record of ONE term is that term,
 *      the sign of a zero included -- and adds the terms of its pairs in round order, first sample then second, then the
 *      odd last sample if it owns it (ascending index); a term that does not exist is skipped;
 *   2. the 64 lanes of a wave combine by the xor butterfly 32, 16, 8, 4, 2, 1 (a + b == b + a bit for bit), the four
 *      waves as (w0 + w1) + (w2 + w3): the chunk's record;
 *   3. a block of one chunk is that record.  Otherwise lane t of one workgroup adds the chunk records t, t + 256, ... in
 *      that order, from -0.0, followed by step 2;
 *   4. the total is step 3 over the block records (an order that depends on the block count only).
 * A record without terms is handed out with +0.0 sums.  Consequences: a block's record has the same 48 bytes at every
 * pointer alignment (the kernels read 16 bytes per lane at any 8-byte-aligned base: no head / body / tail split), under
 * either cache policy (AETH_NT) and on any CU count; and a stream cut at a block boundary and continued -- n0 advanced by
 * the cut, the last L samples passed as history -- gives the same block records bit for bit.
 *
 * With total_host NULL a call does not wait: it is ordered on the context's in-order stream like the element-wise
 * calls.  With total_host set it waits once; the total travels through the context's pinned bounce buffer like the
 * record of aeth_vec_stats.  The chunk records live in a scratch buffer of the context that aeth_ctx_trim releases.
 * Everything is validated before any device work: NULL ctx or x_dev, or both outputs NULL, AETH_E_ARG; n == 0 AETH_E_LEN
 * as for aeth_vec_stats; an unknown kind or power AETH_E_ARG; lag == 0 or lag > 2^20 AETH_E_ARG; pointers 8-byte aligned
 * (AETH_E_ALIGN); 2^31 workgroups or more AETH_E_UNSUPPORTED; rec_dev overlapping x_dev or hist_dev AETH_E_ARG;
 * n0 > UINT64_MAX - n AETH_E_UNSUPPORTED, the message naming both numbers. */
enum { AETH_SYNC_SQUARE = 0, AETH_SYNC_POW1 = 1, AETH_SYNC_POW2 = 2, AETH_SYNC_POW4 = 4, AETH_SYNC_POW8 = 8 };
typedef struct aeth_sync_record {
    double   re, im;        /* the complex sum                                                                 */
    double   mass;          /* sum of the non-negative weights: |sum| / mass is the line's strength            */
    uint64_t n;             /* terms summed                                                                    */
    uint64_t n_nonfinite;   /* terms with a NaN or infinite component (they ARE summed; IEEE decides the sum)  */
    uint64_t reserved;      /* 0                                                                               */
} aeth_sync_record;         /* 48 bytes, 8-byte aligned */
/* No body in the reference.  Host only: C, the samples one workgroup sums. */
AETH_API size_t aeth_sync_chunk(void);
/* No body in the reference: the line terms as defined above; `kind` is an AETH_SYNC_* value, w may be NULL (plain
 * sums), rec_dev (ceil(n / block) records on the device) or total_host may be NULL, not both. */
AETH_API int aeth_sync_line(aeth_ctx *ctx, int kind, const aeth_nco_words *w, uint64_t n0, const aeth_cf32 *x_dev, size_t n,
                            size_t block, aeth_sync_record *rec_dev, aeth_sync_record *total_host);
/* No body in the reference: the lag terms as defined above; power is 1, 2, 4 or 8, hist_dev holds `lag` samples or is
 * NULL. */
AETH_API int aeth_sync_lag(aeth_ctx *ctx, int power, size_t lag, const aeth_cf32 *hist_dev, const aeth_cf32 *x_dev, size_t n,
                           size_t block, aeth_sync_record *rec_dev, aeth_sync_record *total_host);
/* No body in the reference.  Host only, no context: atan2(im, re) / (2 pi) in f64, in [-0.5, 0.5]; 0 for NULL or a
 * (0, 0) sum. */
AETH_API double aeth_sync_turns(const aeth_sync_record *r);
/* No body in the reference.  Host only: aeth_nco_word(-turns / (power * lag)), the step that REMOVES the offset a lag
 * sum of that power and lag has seen; 0 for power <= 0 or lag == 0. */
AETH_API uint64_t aeth_sync_freq_step(const aeth_sync_record *r, int power, size_t lag);
/* No body in the reference.  Host only: unsigned Q32.32 of frac(-turns) * sps, truncated: the aeth_arb_exec phase of the
 * first symbol instant, for a line taken with step = aeth_nco_word(-1 / sps) from the call's first sample.  0 unless
 * 0 < sps <= 2^31. */
AETH_API uint64_t aeth_sync_timing_phase(const aeth_sync_record *r, double sps);

/* ---- moving-window detectors (no body in the reference) ---- */
/* What a burst receiver starts with: a sliding window over a device-resident stream, one value per sample, no known
 * sequence.  One kernel family serves three uses:
 *   timing metric     delay-and-correlate over a repeated training half (Schmidl and Cox: L = W = N / 2) or over the
 *                     cyclic prefix (L = N, W = the prefix): AETH_MOV_LAG
 *   energy detector   squelch, burst edges, the level an AGC follows: AETH_MOV_POWER
 *   carrier offset    the angle of the lag sum at the detected instant: aeth_mov_freq_step of a search record
 *
 * Terms.  Every f64 line is one rounding of products of widened f32 values, as for the estimators above:
 *     e_j = q(x_j) = (double)re * re + (double)im * im
 *     c_j = x_j * conj(x_{j - L}):  c.re = a.re * b.re + a.im * b.im,  c.im = a.im * b.re - a.re * b.im,  a = x_j, b = x_{j - L}
 * (the lag term of aeth_sync_lag at power 1).  x_j for j < 0 is hist_dev[H + j], H = aeth_mov_history(kind, window, lag):
 * W - 1 + L samples for the lag kind, W - 1 for the power kind.  A NULL hist_dev means ZEROS: the system is causal with
 * zero initial state, like the FIR.  (This differs from aeth_sync_lag, where terms in front of the call without history
 * do not exist.)
 *
 * Windows.  For every output i in [0, n), W = window:
 *     P(i) = sum of c_j,  R(i) = sum of e_j,  j = i - W + 1 .. i
 * The partner power of the lag kind is R(i - L): the same sum further back, not a third quantity.
 *
 * Metric, in f64, each multiplication, the addition and the division rounded on its own (these products are not exact:
 * the library is built without contraction), then rounded to f32:
 *     AETH_MOV_LAG     num = P.re * P.re + P.im * P.im;  den = R(i) * R(i - L);  M(i) = den == 0 ? +0.0f : (float)(num / den)
 *                      (M <= 1 up to rounding by Cauchy-Schwarz; 1 where the window repeats exactly, and at W = 1 for
 *                      any finite non-zero pair)
 *     AETH_MOV_POWER   (lag must be 0)  M(i) = (float)(R(i) / (double)W): the moving mean power
 *
 * The order of the additions is a function of W and of the output's index in the call only: not of the pointer, the
 * cache policy (AETH_NT), the CU count, `block`, or the planes requested; aeth_mov_exec and aeth_mov_search see the same
 * f64 sums.  A window sum adds that window's own W terms and nothing else (no running sum is differenced: a window behind
 * a strong burst does not inherit the burst's rounding error).  It is van Herk's scheme over segments [s W, (s + 1) W)
 * counted from the call's index 0 (history lies in segments -1, -2, ...).  Term j has position k = j - s W in its segment
 * and lies in cell c = k / 32; a segment has cps = ceil(W / 32) cells, the last one short when 32 does not divide W:
 *     a(k) = the cell's terms from its first through k, added in ascending order from -0.0
 *     d(k) = the cell's terms from its last down to k, added in descending order from -0.0
 *     T_c  = a(last k of cell c)
 *     v    = the log-step scan of T_0 .. T_{cps - 1}: for s = 1, 2, 4, ... < cps:  v[c] = v[c - s] + v[c] for all c >= s at once
 *     u    = the same scan of the totals in reverse order, T_{cps - 1} .. T_0
 *     h(k) = a(k) for c == 0, else v[c - 1] + a(k)                 (the segment's terms 0 .. k)
 *     g(k) = d(k) for c == cps - 1, else u[cps - 2 - c] + d(k)     (the segment's terms k .. W - 1)
 *     S(i) = h(W - 1) of i's segment when i mod W == W - 1, else g(k + 1) of the segment in front + h(k) of i's own, k = i mod W
 * Sums start from -0.0 (the identity of IEEE addition), so W = 1 hands out each term itself, the sign of a zero included.
 * tests/mov_truth.py restates this in numpy.  Cuts: aeth_mov_grid(kind, window) = W.  A stream cut at a multiple of it
 * and continued with the last H samples as history (zeros where the stream is shorter than H) gives planes byte for byte
 * those of one call.
 *
 * aeth_mov_exec writes the planes that are not NULL -- p_dev: cf32 ((float)P.re, (float)P.im), lag kind only; r_dev:
 * (float)R(i); m_dev: M(i) -- 8 B read per sample (the partner range is a second read that the caches serve for small L),
 * 4 or 8 B written per plane.  It is stream-ordered and does not wait.
 *
 * aeth_mov_search writes no plane: one 64-byte record per `block` samples (0: one block of n; the last block may be
 * short; peaks_dev holds ceil(n / block) records; blocks shorter than 1024 samples take a workgroup each).  Output i is a
 * CANDIDATE when M(i) is not NaN, R(i) >= r_min and, for the lag kind, R(i - L) >= r_min.  `index` is the candidate with
 * the largest M, ties to the lowest index, counted from the call's first sample; `first` the lowest candidate with
 * (double)M >= threshold (n when there is none); p_re, p_im, r, r_lag the f64 sums at `index` (the power kind: r only, the
 * others +0.0); metric = M(index); n_nan the block's count of outputs whose M is NaN, saturating.  A block without a
 * candidate reports index = first = n, metric = NaN and +0.0 sums.  best_host (may be NULL; not both outputs NULL) waits
 * once and returns the same record over the whole call; it travels through the context's pinned bounce buffer like the
 * total of aeth_sync_*.  Chunk records live in a scratch buffer of the context that aeth_ctx_trim releases.  No
 * floating-point atomics anywhere.
 *
 * Everything is refused before any device work, the message naming the offending value: NULL ctx or x_dev, or every
 * output NULL, AETH_E_ARG; n == 0 AETH_E_LEN; an unknown kind AETH_E_ARG; window == 0 AETH_E_ARG; window > 4096
 * AETH_E_UNSUPPORTED; the lag kind with lag == 0 AETH_E_ARG, with lag > 65536 AETH_E_UNSUPPORTED; the power kind with
 * lag != 0 or with p_dev AETH_E_ARG; r_min negative or NaN, threshold NaN AETH_E_ARG; x_dev, hist_dev, p_dev, peaks_dev
 * (or best_host) not 8-byte aligned, r_dev or m_dev not 4-byte aligned AETH_E_ALIGN; any output overlapping an input or
 * another output AETH_E_ARG; 2^31 workgroups or more AETH_E_UNSUPPORTED. */
enum { AETH_MOV_LAG = 0, AETH_MOV_POWER = 1 };
typedef struct aeth_mov_peak {
    uint64_t index;         /* the candidate with the largest metric (lowest index of equals); n when there is none */
    uint64_t first;         /* the lowest candidate with metric >= threshold; n when there is none                  */
    double   p_re, p_im;    /* P(index)                                                                             */
    double   r, r_lag;      /* R(index), R(index - L)                                                               */
    float    metric;        /* M(index); NaN when there is no candidate                                             */
    uint32_t n_nan;         /* outputs whose M is NaN (saturating)                                                  */
    uint64_t reserved;      /* 0                                                                                    */
} aeth_mov_peak;            /* 64 bytes, 8-byte aligned */
/* No body in the reference.  Host only: H, the samples of history a call takes; 0 for an unknown kind or window == 0. */
AETH_API size_t aeth_mov_history(int kind, size_t window, size_t lag);
/* No body in the reference.  Host only: the cut granularity G = window; 0 for an unknown kind or a window the calls
 * refuse. */
AETH_API size_t aeth_mov_grid(int kind, size_t window);
/* No body in the reference.  Host only: aeth_nco_word(-atan2(p_im, p_re) / (2 pi lag)), the step that REMOVES the offset
 * the lag sum of the record has seen (aeth_sync_freq_step at power 1); 0 for NULL, a zero sum or lag == 0. */
AETH_API uint64_t aeth_mov_freq_step(const aeth_mov_peak *p, size_t lag);
/* No body in the reference: the planes as defined above; any of p_dev, r_dev, m_dev may be NULL, not all. */
AETH_API int aeth_mov_exec(aeth_ctx *ctx, int kind, size_t window, size_t lag, const aeth_cf32 *hist_dev, const aeth_cf32 *x_dev,
                           size_t n, aeth_cf32 *p_dev, float *r_dev, float *m_dev);
/* No body in the reference: the search records as defined above; peaks_dev or best_host may be NULL, not both. */
AETH_API int aeth_mov_search(aeth_ctx *ctx, int kind, size_t window, size_t lag, double r_min, double threshold,
                             const aeth_cf32 *hist_dev, const aeth_cf32 *x_dev, size_t n, size_t block, aeth_mov_peak *peaks_dev,
                             aeth_mov_peak *best_host);

/* ---- convolutional codes: encoder and soft-decision Viterbi decoder (no body in the reference) ---- */
/* Forward error correction between the bits and the symbols: the rate 1/n codes of constraint length k = 3 .. 7 (the
 * K = 7 codes of 802.11, DVB-S, CCSDS and LTE have 64 states, one per lane of a wave).  Everything is integer and defined
 * bit for bit.  Bits are one byte per bit as everywhere in the library.
 *
 * The code.  3 <= k <= 7, 2 <= n <= 4, 0 < poly[j] < 2^k in the usual octal convention with the current bit at the MSB
 * (K = 7: 0171, 0133):
 *     reg_t = sum_{i < k} u[t - i] * 2^(k - 1 - i)          c[n t + j] = parity(reg_t & poly[j])
 * u[t] for t < 0 is the caller's history of k - 1 bits (hist[i] = u[i - (k - 1)]), or zero for NULL.  Input bytes are
 * taken & 1.  Each output needs k input bits and nothing else, so the chunks of a stream concatenate bit for bit when
 * each call gets the last k - 1 bits of the one before as its history.
 *
 * The decoder.  Soft values are int8_t, one per coded bit in the encoder's output order; positive means bit 0 is
 * likelier, 0 is an erasure (a stream depunctured by aeth_remap_exec carries zeros).  A call has N = nbits steps; its history is
 * A + T steps of n values each before step 0, NULL meaning erasures.
 *   Delay.    out[o] is the decision for step o - T: the decoder is a causal system with delay T.
 *   Blocks.   Output block b is o in [b D, min(N, (b + 1) D)).  Its window is steps [b D - T - A, min(N, (b + 1) D)).
 *   Metrics.  Every window starts with all S = 2^(k-1) state metrics at 0, held as int32.  No normalisation is needed:
 *             |metric| <= 8192 * 4 * 128.
 *   States.   State s holds u[t-1] at bit k-2 down to u[t-k+1] at bit 0.  Step t enters state j from p0 = (2 j) mod S
 *             or p1 = p0 + 1 with input bit u = j >> (k-2);
 *                 cand_d = m[p_d] + sum_q (1 - 2 c_q(u, p_d)) * v[n t + q],
 *             c_q(u, p) = parity((u 2^(k-1) + p) & poly[q]).  p1 is taken only if cand_1 > cand_0; a tie takes p0.
 *   Traceback.  At the window's end take the state with the largest metric, ties to the smallest state, and trace
 *             back, emitting u of every step that maps to an output of the block.  The first A steps of a window store
 *             no decisions.
 * Consequences: two calls equal one call, bit for bit, when the first call's N is a multiple of D and the second gets
 * the first's last A + T steps as history.  A known zero start state is a history of +127s.  A stream is flushed by T
 * steps of erasures (the first T outputs of a stream are decisions about its history).
 *
 * aeth_cc_create: block D >= 1, D + T <= 4096, A <= 4096.  k = 8 and 9 (two and four states per lane) are refused with
 * AETH_E_UNSUPPORTED, the message naming k; every other violation is AETH_E_ARG naming the offending value.  The object
 * owns no device memory.  aeth_cc_history is A + T, in trellis steps.
 * aeth_cc_encode: ncoded != nbits * n is AETH_E_LEN.  aeth_cc_decode: nsoft != nbits * n is AETH_E_LEN.  Pointers may
 * have any byte alignment; an output range that shares a byte with an input or history range is AETH_E_ARG.  Both are
 * ordered on the context's stream and validate everything before any device work; a length of 0 launches nothing. */
typedef struct aeth_cc_code { uint32_t k; uint32_t n; uint32_t poly[4]; } aeth_cc_code;
AETH_API int aeth_cc_create(aeth_ctx *ctx, const aeth_cc_code *code, size_t block, size_t warmup, size_t traceback, aeth_cc **out);
AETH_API int aeth_cc_destroy(aeth_cc *cc);
AETH_API size_t aeth_cc_k(const aeth_cc *cc);
AETH_API size_t aeth_cc_n(const aeth_cc *cc);
AETH_API size_t aeth_cc_block(const aeth_cc *cc);
AETH_API size_t aeth_cc_warmup(const aeth_cc *cc);
AETH_API size_t aeth_cc_traceback(const aeth_cc *cc);
AETH_API size_t aeth_cc_history(const aeth_cc *cc);
AETH_API int aeth_cc_encode(aeth_cc *cc, const uint8_t *hist_bits_dev, const uint8_t *bits_dev, size_t nbits, uint8_t *coded_dev,
                            size_t ncoded);
AETH_API int aeth_cc_decode(aeth_cc *cc, const int8_t *hist_soft_dev, const int8_t *soft_dev, size_t nsoft, uint8_t *bits_dev,
                            size_t nbits);

/* ---- rate matching: periodic byte maps for puncturing and interleaving (no body in the reference) ---- */
/* What stands between the coder and the mapper of a coded link, and its inverse between aeth_demod_soft and
 * aeth_cc_decode: puncturing (rate 2/3 and 3/4 from the K = 7 rate 1/2 code), depuncturing to erasures, a block
 * interleaver, or any chain of them.  All are one operation, a periodic gather of bytes with a constant where nothing is
 * gathered.
 *
 * An aeth_remap holds an input period R_in, an output period R_out and a table map[R_out] of int32_t, each entry -1 or an
 * index in [0, R_in).  Elements are bytes that the kernel never interprets: the same call moves uint8_t bits and int8_t
 * soft values.
 *     out[q R_out + i] = map[i] < 0 ? fill : in[q R_in + map[i]]          q = 0, 1, ...;  0 <= i < R_out
 * `fill` is a byte argument of the exec call (0: erasures in front of the decoder).  An input index may appear any
 * number of times (repetition) or not at all (puncturing).
 *
 * A call writes n_out bytes: Q = n_out div R_out whole periods, then a partial last period of n_out mod R_out outputs.  It
 * reads only inside the first aeth_remap_in_count(rm, n_out) input bytes: Q R_in, plus one more than the largest
 * non-negative map[i] with i < n_out mod R_out (plus 0 when there is none).  n_in below that count is AETH_E_LEN, the
 * message naming both numbers; a larger n_in is allowed.  A period needs nothing from its neighbours, so the chunks of a
 * stream cut at any multiple of R_out outputs and R_in inputs concatenate byte for byte with no history.
 *
 * Limits, all checked before any device work, the offending value in the message: 1 <= R_in, R_out <= 2^20 and table
 * entries in [-1, R_in) (the position and the value are named), else AETH_E_ARG; n_in or n_out at or above 2^32 is
 * AETH_E_UNSUPPORTED (the caller cuts at a period, which costs nothing); an output range that shares a byte with the input
 * range is AETH_E_ARG.  Pointers may have any byte alignment; n_out = 0 launches nothing.  The object owns the device copy
 * of its table (uint16_t offsets of a whole tile on the tile route, the int32_t table on the gather route);
 * aeth_remap_destroy frees it, and a refused create leaves the device's free memory unchanged.
 *
 * aeth_remap_route says which kernel a call takes: AETH_REMAP_ROUTE_TILE when a tile of g = aeth_remap_tile(rm) >= 1 whole
 * periods and its table fit 32 KiB of LDS (the inputs are staged there and every lane assembles 16 output bytes), else
 * AETH_REMAP_ROUTE_GATHER (table and inputs from global memory; aeth_remap_tile is 0).  The results do not depend on it.
 *
 * Not built: elements wider than a byte (cf32 symbol interleavers, pilot insertion), maps that reach into earlier periods
 * (Forney / convolutional interleavers), maps over bit-packed streams (aeth_bits_unpack first), an aeth_stream_op kind, host-slice flavours. */
#define AETH_REMAP_ROUTE_TILE 1
#define AETH_REMAP_ROUTE_GATHER 2
AETH_API int aeth_remap_create(aeth_ctx *ctx, const int32_t *map, size_t r_out, size_t r_in, aeth_remap **out);
AETH_API int aeth_remap_destroy(aeth_remap *rm);
AETH_API size_t aeth_remap_in_period(const aeth_remap *rm);
AETH_API size_t aeth_remap_out_period(const aeth_remap *rm);
AETH_API size_t aeth_remap_in_count(const aeth_remap *rm, size_t n_out);
AETH_API int aeth_remap_route(const aeth_remap *rm);
AETH_API size_t aeth_remap_tile(const aeth_remap *rm);
AETH_API int aeth_remap_exec(aeth_remap *rm, const void *in_dev, size_t n_in, void *out_dev, size_t n_out, uint8_t fill);
/* Host-only table builders: pure integer arithmetic, no context.  Each writes into caller memory; where it takes a
 * capacity, too small a one is AETH_E_LEN with the needed size in the message.
 *   puncture   keep[i] & 1 says whether coded bit i of a period of p is sent: R_in = p, R_out = *r_out = the number kept,
 *              map = the kept positions ascending.  An all-zero keep is AETH_E_ARG.
 *   invert     inv has r_in entries: inv[j] is the smallest i with map[i] == j, or -1 -- the depuncturer of a puncturer,
 *              the deinterleaver of an interleaver, the first copy of a repetition.
 *   compose    b applied to the output of a.  With m = lcm(a_out, b_in): *r_in = a_in m / a_out, *r_out = b_out m / b_in;
 *              a -1 in either table propagates; a period above 2^20 is AETH_E_UNSUPPORTED.
 *   rows_cols  written row by row, read column by column: map[c rows + r] = r cols + c (rows cols entries).
 *   bicm16     the two-step permutation of 802.11a 17.3.5.6 from its formulas: s = max(n_bpsc / 2, 1), coded bit k goes to
 *              i = (n_cbps / 16) (k mod 16) + k div 16, then to j = s (i div s) + (i + n_cbps - (16 i) div n_cbps) mod s;
 *              map is the gather form, map[j] = k (n_cbps entries).  n_cbps must be a multiple of 16 s and of n_bpsc,
 *              else AETH_E_ARG. */
AETH_API int aeth_remap_puncture(const uint8_t *keep, size_t p, int32_t *map, size_t cap, size_t *r_out);
AETH_API int aeth_remap_invert(const int32_t *map, size_t r_out, size_t r_in, int32_t *inv);
AETH_API int aeth_remap_compose(const int32_t *a, size_t a_out, size_t a_in, const int32_t *b, size_t b_out, size_t b_in, int32_t *map,
                                size_t cap, size_t *r_out, size_t *r_in);
AETH_API int aeth_remap_rows_cols(size_t rows, size_t cols, int32_t *map);
AETH_API int aeth_remap_bicm16(size_t n_cbps, size_t n_bpsc, int32_t *map);

/* ---- frame checks: CRC attach and check over bit frames, bit packing (no body in the reference) ---- */
/* The last step of every frame format: the 802.11 FCS, CRC-24A/B on LTE transport and code blocks, the RNTI-masked
 * CRC-16 of a control channel.  Everything is integer arithmetic and defined byte for byte.
 *
 * An aeth_crc object holds a width r with 1 <= r <= 64.  It holds poly, the low r coefficients of the generator; x^r is
 * implied and bit 0 must be set.  It holds init and xorout, both below 2^r.
 *
 * A message is a run of bytes, one per bit.  Only the lowest bit of each byte counts, as in aeth_seq_scramble.  Per
 * message bit b, in stream order:
 *     fb  = ((reg >> (r-1)) & 1) ^ b
 *     reg = (reg << 1) & (2^r - 1);   if fb: reg ^= poly
 * The register of a frame is reg after its last bit, starting from init.  The check value is reg ^ xorout.  The check
 * bits are c[j] = (value >> (r-1-j)) & 1 for j = 0 .. r-1, highest coefficient first.  That is the transmission order of
 * 802.11 and 3GPP.  "Reflected" catalogue entries are this definition applied to bytes unpacked LSB first.
 *
 * aeth_crc_named (host only) fills the parameters of a catalogue name; an unknown name is AETH_E_ARG and the message
 * lists the known ones: crc-8, crc-8/lte, crc-16/xmodem (the LTE CRC-16), crc-16/ibm-3740, crc-16/genibus, crc-24/lte-a,
 * crc-24/lte-b, crc-32/bzip2, crc-64/ecma-182, and crc-32 (802.3, the 802.11 FCS): the parameters of crc-32/bzip2, for a
 * caller that unpacks bytes LSB first (aeth_bits_unpack with AETH_BITS_LSB_FIRST); the 32 check bits packed LSB first
 * are then the four bytes of the usual CRC-32, lowest first.
 * aeth_crc_residue is host arithmetic: the register (before xorout) that any frame followed by its own check bits leaves
 * (0xC704DD7B for crc-32).  aeth_crc_host runs the definition on host memory with no context; *reg is the register.
 *
 * aeth_crc_exec, the streaming primitive: F frames of L bits, contiguous.  state_out[f] (uint64_t) is the register of
 * frame f started from state_in[f], or from init when state_in_dev is NULL; xorout is not applied.  A frame cut at any
 * bit, the first call's state_out given as the second call's state_in, gives the bytes of one call.  L = 0 returns the
 * start state.
 * aeth_crc_attach: the output is F frames of L + r bytes, each the message with every byte reduced to & 1, followed by
 * the check bits.
 * aeth_crc_check: the input is F frames of L + r bytes.  Per frame, diff[f] = (received check bits read as a word, first
 * bit highest) ^ (check value of the L message bits) ^ mask; mask is below 2^r, 0 for a plain check or an RNTI-style
 * scrambling word.  A frame is good when diff == 0; mask = 0 on a masked frame returns the mask in diff.  payload_dev
 * (F L bytes, & 1) and diff_dev are optional; summary_dev receives {n_bad, first_bad}, first_bad = F when no frame is
 * bad, made by a fold of per-workgroup records and so the same in every run.  At least one of the three must be non-NULL.
 * aeth_bits_pack takes & 1 of every byte and needs nbytes == ceil(nbits / 8); bit i goes to byte i div 8, at bit i mod 8
 * (AETH_BITS_LSB_FIRST) or 7 - i mod 8 (AETH_BITS_MSB_FIRST); the unused bits of the last byte are 0.  aeth_bits_unpack
 * needs nbits <= 8 nbytes and writes 0 / 1.
 *
 * All device calls are ordered on the context's stream and none waits.  Everything is validated before any device work,
 * the offending value in the message: null handles or pointers, r outside 1 .. 64, an even poly, poly, init, xorout or
 * mask at or above 2^r, an unknown order AETH_E_ARG; a wrong nbytes or nbits AETH_E_LEN; a call whose input or output
 * reaches 2^32 bytes AETH_E_UNSUPPORTED (the caller cuts and carries the state); an output range that shares a byte with
 * an input range (or another output) AETH_E_ARG.  Pointers to bits and bytes may have any byte alignment; the uint64_t
 * arrays and the summary are 8-byte aligned (AETH_E_ALIGN).  F = 0 launches nothing, except
 * that check still writes the summary {0, 0}.  aeth_crc_destroy(NULL) is AETH_OK and getters on NULL return 0.
 *
 * Routes.  aeth_crc_route(crc, L, F) is AETH_CRC_ROUTE_FRAMES for L <= aeth_crc_route_frame_bits(crc) (16384): a group of
 * 4 .. 64 lanes owns a frame, aeth_crc_frames_per_workgroup(crc, frame bytes) frames share a workgroup, and attach and
 * check store from the kernel that forms the registers.  Longer frames take AETH_CRC_ROUTE_LONG: chunks of 16384 bits
 * over many workgroups, their registers in a scratch the object owns (freed by aeth_crc_destroy), a second launch that
 * combines them, and a third that stores for attach and check.  The results never depend on the route.  The object also
 * owns its weight table (129 KiB of device memory).
 *
 * Not built: frames of differing length in one call, strided frames, soft-value input, an aeth_stream_op kind, host-slice
 * flavours, generator polynomials above degree 64. */
#define AETH_CRC_ROUTE_FRAMES 1
#define AETH_CRC_ROUTE_LONG 2
#define AETH_BITS_LSB_FIRST 0
#define AETH_BITS_MSB_FIRST 1
typedef struct aeth_crc_summary { uint64_t n_bad; uint64_t first_bad; } aeth_crc_summary;
AETH_API int aeth_crc_create(aeth_ctx *ctx, uint32_t r, uint64_t poly, uint64_t init, uint64_t xorout, aeth_crc **out);
AETH_API int aeth_crc_destroy(aeth_crc *crc);
AETH_API uint32_t aeth_crc_width(const aeth_crc *crc);
AETH_API uint64_t aeth_crc_poly(const aeth_crc *crc);
AETH_API uint64_t aeth_crc_init(const aeth_crc *crc);
AETH_API uint64_t aeth_crc_xorout(const aeth_crc *crc);
AETH_API uint64_t aeth_crc_residue(const aeth_crc *crc);
AETH_API int aeth_crc_route(const aeth_crc *crc, size_t L, size_t F);
AETH_API size_t aeth_crc_route_frame_bits(const aeth_crc *crc);
AETH_API size_t aeth_crc_frames_per_workgroup(const aeth_crc *crc, size_t frame_bytes);
AETH_API int aeth_crc_named(const char *name, uint32_t *r, uint64_t *poly, uint64_t *init, uint64_t *xorout);
AETH_API int aeth_crc_host(uint32_t r, uint64_t poly, uint64_t init, uint64_t xorout, const uint8_t *bits_host, size_t L, uint64_t *reg);
AETH_API int aeth_crc_exec(aeth_crc *crc, const uint8_t *bits_dev, size_t L, size_t F, const uint64_t *state_in_dev, uint64_t *state_out_dev);
AETH_API int aeth_crc_attach(aeth_crc *crc, const uint8_t *in_dev, size_t L, size_t F, uint8_t *out_dev);
AETH_API int aeth_crc_check(aeth_crc *crc, const uint8_t *in_dev, size_t L, size_t F, uint64_t mask, uint64_t *diff_dev, uint8_t *payload_dev,
                            aeth_crc_summary *summary_dev);
AETH_API int aeth_bits_pack(aeth_ctx *ctx, const uint8_t *bits_dev, size_t nbits, int order, uint8_t *bytes_dev, size_t nbytes);
AETH_API int aeth_bits_unpack(aeth_ctx *ctx, const uint8_t *bytes_dev, size_t nbytes, int order, uint8_t *bits_dev, size_t nbits);

/* ---- LDPC codes: quasi-cyclic encoder and a layered min-sum decoder (no body in the reference) ---- */
/* The block code of 802.11n/ac/ax, 5G NR data and DVB-S2, behind aeth_demod_soft.  Everything is integer arithmetic and
 * defined byte for byte.
 *
 * The code.  aeth_ldpc_code is a table of rows x cols circulant blocks of size z, row-major: shift[r cols + c] is -1 for
 * a zero block, else s in [0, z): the z x z identity shifted so that row i of the block has its one at column
 * (i + s) mod z.  N = cols z, M = rows z, K = N - M.  Bits are one byte per bit (taken & 1); soft values are int8_t,
 * positive means bit 0 is likelier and 0 is an erasure (aeth_cc_decode, aeth_demod_soft).  Punctured and shortened
 * positions are the caller's job with aeth_remap_exec (fill 0 or 127).
 *
 * Limits, all refused before any device work with the offending value in the message: 1 <= rows < cols, rows <= 256,
 * 1 <= z (AETH_E_ARG); every entry in [-1, z) (the message names position and value); every row holds at least one
 * block (the message names the row); the decoder state of 2 N + E z bytes, E the number of non-negative entries, is at
 * most 64 KiB (AETH_E_UNSUPPORTED, naming both numbers); the parity part -- the last `rows` block columns as a dense
 * M x M matrix over GF(2) -- is invertible (AETH_E_ARG, "parity part singular").  A refused create leaves the device's
 * free memory unchanged.
 *
 * Encoder, systematic: coded[f N .. f N + K) = u_f & 1, then the M parity bits p = P u over GF(2), where H = [A | B] and
 * P = B^-1 A (M x K), computed once at create on the host by Gaussian elimination on 64-bit words.
 * aeth_ldpc_generator is a host function with no context: row i of P in ceil(K / 64) words, bit j at word j / 64, bit
 * j % 64; nwords below M ceil(K / 64) is AETH_E_LEN.  aeth_ldpc_create uploads P; the object owns P and the shift table
 * on the device.  aeth_ldpc_encode: nbits = F K and ncoded = F N, else AETH_E_LEN; any byte alignment; overlapping ranges
 * AETH_E_ARG; F = 0 launches nothing.
 *
 * Decoder: layered normalised min-sum, all arithmetic int32.  Per codeword Q[v] = soft[v] for v < N and R[e] = 0 for
 * every edge.  The edges of check (r, i) are the columns c ascending with shift[r][c] >= 0, at variable
 * v = c z + (i + shift[r][c]) mod z.  One iteration visits the layers r = 0 .. rows - 1 in order; for every check (r, i)
 * of the layer:
 *     1. T_e = Q[v_e] - R[e];  neg_e = T_e < 0 (zero counts as positive)
 *     2. m1 <= m2 are the two smallest |T_e|; both start at 32767, and a value replaces m1 only if strictly smaller, so
 *        the first of equal minima is the argmin a
 *     3. mag_e = min((3 (e == a ? m2 : m1)) >> 2, 127)
 *     4. R[e] = (parity of all neg) xor neg_e ? -mag_e : mag_e
 *     5. Q[v_e] = T_e + R[e]
 * The checks of a layer touch disjoint variables, so their order does not matter; layers are ordered.  Nothing
 * saturates: Q = soft + sum R throughout, so |Q| <= 128 + 127 rows < 2^15, which is why rows <= 256.
 * After each full iteration `unsat` is the number of checks whose hard decisions (Q[v] < 0) have odd parity; with
 * AETH_LDPC_EARLY the codeword stops when unsat == 0.  max_iter = 0 is allowed: the hard decisions of the input and
 * their unsat.  Output bits are Q[v] < 0 for all N positions, with AETH_LDPC_PAYLOAD only the first K.  rec_dev (may be
 * NULL; 4-byte aligned, AETH_E_ALIGN) receives {iterations run, unsat after the last} per codeword.
 * aeth_ldpc_decode: nsoft = F N, nbits = F N or F K by flag, else AETH_E_LEN; max_iter > 1000, unknown flag bits, ranges
 * that share a byte AETH_E_ARG; any byte alignment of soft and bits.  Codewords are independent: a call cut at any
 * codeword equals two calls byte for byte, and nothing depends on aeth_ldpc_group.
 *
 * Kernel.  aeth_ldpc_group codewords share a workgroup -- as many as keep G z <= 256 lanes and G states within 64 KiB of
 * LDS (aeth_ldpc_lds_bytes), at least one; a lane owns one check of the current layer; Q is int16 and R int8 in LDS; one
 * workgroup barrier per layer.  Getters return 0 for NULL and aeth_ldpc_destroy(NULL) is AETH_OK.  All device calls are
 * ordered on the context's stream and none waits.
 *
 * Not built: codes above the 64 KiB LDS state (5G base graph 1 at large Z), standard base-matrix catalogues, soft
 * (posterior) output, offset min-sum, a structured encoder that avoids the dense P, an aeth_stream_op kind, host-slice
 * flavours. */
#define AETH_LDPC_EARLY 1u
#define AETH_LDPC_PAYLOAD 2u
typedef struct aeth_ldpc_code { uint32_t rows, cols, z; const int32_t *shift; } aeth_ldpc_code;   /* shift[rows*cols], row-major */
typedef struct aeth_ldpc_record { uint32_t iterations, unsatisfied; } aeth_ldpc_record;
AETH_API int aeth_ldpc_generator(const aeth_ldpc_code *code, uint64_t *p_out, size_t nwords);
AETH_API int aeth_ldpc_create(aeth_ctx *ctx, const aeth_ldpc_code *code, aeth_ldpc **out);
AETH_API int aeth_ldpc_destroy(aeth_ldpc *ldpc);
AETH_API size_t aeth_ldpc_n(const aeth_ldpc *ldpc);
AETH_API size_t aeth_ldpc_k(const aeth_ldpc *ldpc);
AETH_API uint32_t aeth_ldpc_rows(const aeth_ldpc *ldpc);
AETH_API uint32_t aeth_ldpc_cols(const aeth_ldpc *ldpc);
AETH_API uint32_t aeth_ldpc_z(const aeth_ldpc *ldpc);
AETH_API size_t aeth_ldpc_edges(const aeth_ldpc *ldpc);
AETH_API size_t aeth_ldpc_lds_bytes(const aeth_ldpc *ldpc);     /* dynamic LDS of a decoder workgroup */
AETH_API uint32_t aeth_ldpc_group(const aeth_ldpc *ldpc);       /* codewords per decoder workgroup */
AETH_API int aeth_ldpc_encode(aeth_ldpc *ldpc, const uint8_t *bits_dev, size_t nbits, uint8_t *coded_dev, size_t ncoded);
AETH_API int aeth_ldpc_decode(aeth_ldpc *ldpc, const int8_t *soft_dev, size_t nsoft, uint32_t max_iter, uint32_t flags,
                              uint8_t *bits_dev, size_t nbits, aeth_ldpc_record *rec_dev);

/* ---- Reed-Solomon codes: systematic encoder, errors-and-erasures decoder (no body in the reference) ---- */
/* The outer code of CCSDS telemetry (RS(255, 223) around the K = 7 code of aeth_cc_*), of DVB-S / DVB-T (RS(204, 188)),
 * of DAB+, ATSC, DSL, CD/DVD, QR codes and RAID-6: the code over symbols that repairs the bursts a Viterbi decoder
 * leaves.  Everything is integer arithmetic and defined byte for byte.
 *
 * The code.  Symbols are bytes over GF(2^m), 3 <= m <= 8, N0 = 2^m - 1; every input byte is taken & N0.  poly is the
 * field polynomial with its x^m term (0x11d, 0x187, 0x13, 0xb) and must be primitive (x has order N0), else AETH_E_ARG
 * "polynomial not primitive".  beta = alpha^prim with gcd(prim, N0) = 1, 0 <= fcr < N0, and
 *     g(x) = prod over j < r of (x - beta^(fcr + j)),  r = nroots,  1 <= r <= 64,  r < n <= N0,  k = n - r;
 * n < N0 is the shortened code.  r > 64 is AETH_E_UNSUPPORTED, every other violation AETH_E_ARG, refused before any
 * device work with the offending value in the message.  Symbol 0 of a codeword is the highest coefficient and is
 * transmitted first: c(x) = sum c_j x^(n-1-j).  A codeword is k data symbols followed by r parity symbols, the remainder
 * of d(x) x^r modulo g.
 * Interleaving is an argument of every call: depth I, 1 <= I <= 64.  A frame is I n bytes (I k on the data side); symbol
 * j of codeword i of frame f sits at byte f I n + j I + i.  I = 1 is plain contiguous codewords, I = 4 or 5 the CCSDS
 * frame.  The data part of an encoded frame is the input frame in place (& N0) and the I r parity bytes follow it.
 * aeth_rs_named (host only) knows ccsds-255-223 (0x187, fcr 112, prim 11; conventional basis), ccsds-255-239 (fcr 120),
 * dvb-204-188 (0x11d, fcr 0, prim 1) and rs-15-11 (0x13, fcr 1); an unknown name is AETH_E_ARG and the message lists the
 * known ones.
 *
 * Host functions with no context: aeth_rs_generator writes g_out[i] = the coefficient of x^i, i <= r (ng < r + 1 is
 * AETH_E_LEN); aeth_rs_host_encode and aeth_rs_host_decode run the definition on host memory with the rules of the
 * device calls (their record and summary pointers need no alignment).
 *
 * Decode, per codeword.  E is the set of erased positions (era[pos] != 0; era_dev is NULL or as long as the input),
 * f = |E|.  For a codeword c of the (shortened) code e(c) is the number of positions outside E where c differs from the
 * masked input.  If some c has 2 e(c) + f <= r it is unique, and the output is c (its first k symbols with
 * AETH_RS_PAYLOAD) with the record {corrected = the number of all n positions where c differs from the masked input,
 * status = 0}.  Otherwise the output is the masked input (or its first k symbols) and the record is {0, 1}; f > r is
 * such a failure, not an error.  The decoder establishes the bound itself: it fails unless deg Lambda = L,
 * 2 (L - f) + f <= r, Lambda has exactly deg Lambda distinct roots, all at positions below n, and no Forney
 * denominator vanishes.  rec_dev (may be NULL; 4-byte aligned) receives one record per codeword, codeword i of frame f
 * at f I + i.  summary_dev (may be NULL; 8-byte aligned) receives {n_failed, n_corrected}: written, not accumulated,
 * by a fixed fold of per-workgroup records and so the same in every run.
 *
 * Call rules.  Codewords are independent: a call cut at any frame equals two calls byte for byte.  Lengths are whole
 * frames and the same number of them on both sides (AETH_E_LEN); ranges that share a byte, unknown flags, depth outside
 * 1 .. 64 AETH_E_ARG; rec_dev or summary_dev misaligned AETH_E_ALIGN; data pointers may have any byte alignment.  Zero
 * frames launch nothing but decode still writes the summary {0, 0}.  All device calls are ordered on the context's
 * stream and none waits.  Getters return 0 for NULL and aeth_rs_destroy(NULL) is AETH_OK.
 *
 * Kernel.  A codeword belongs to a group of R2 lanes, R2 the power of two at or above r; aeth_rs_group = 256 / R2
 * codewords share a workgroup.  Encoder and syndromes multiply by a per-lane constant with eight select-XORs on the
 * constant's images in two registers; only damaged codewords run erasure locator, Berlekamp-Massey, Chien and Forney,
 * on log / antilog tables and aeth_rs_lds_bytes(rs, depth) bytes of dynamic LDS per workgroup.
 *
 * Not built: the CCSDS dual-basis representation, symbols wider than 8 bits, BCH codes over GF(2), a convolutional
 * (Forney) byte interleaver, soft-decision decoding, an aeth_stream_op kind and host-slice flavours. */
#define AETH_RS_PAYLOAD 1u
typedef struct aeth_rs_code { uint32_t m, poly, fcr, prim, nroots, n; } aeth_rs_code;
typedef struct aeth_rs_record { uint32_t corrected, status; } aeth_rs_record;
typedef struct aeth_rs_summary { uint64_t n_failed; uint64_t n_corrected; } aeth_rs_summary;
AETH_API int aeth_rs_named(const char *name, aeth_rs_code *code);
AETH_API int aeth_rs_generator(const aeth_rs_code *code, uint8_t *g_out, size_t ng);
AETH_API int aeth_rs_host_encode(const aeth_rs_code *code, const uint8_t *data_host, size_t ndata, uint32_t depth, uint8_t *coded_host, size_t ncoded);
AETH_API int aeth_rs_host_decode(const aeth_rs_code *code, const uint8_t *in_host, size_t nin, const uint8_t *era_host, uint32_t depth,
                                 uint32_t flags, uint8_t *out_host, size_t nout, aeth_rs_record *rec_host, aeth_rs_summary *summary_host);
AETH_API int aeth_rs_create(aeth_ctx *ctx, const aeth_rs_code *code, aeth_rs **out);
AETH_API int aeth_rs_destroy(aeth_rs *rs);
AETH_API size_t aeth_rs_n(const aeth_rs *rs);
AETH_API size_t aeth_rs_k(const aeth_rs *rs);
AETH_API uint32_t aeth_rs_nroots(const aeth_rs *rs);
AETH_API uint32_t aeth_rs_m(const aeth_rs *rs);
AETH_API uint32_t aeth_rs_group(const aeth_rs *rs);                  /* codewords per workgroup */
AETH_API size_t aeth_rs_lds_bytes(const aeth_rs *rs, uint32_t depth);   /* dynamic LDS of a decoder workgroup */
AETH_API int aeth_rs_encode(aeth_rs *rs, const uint8_t *data_dev, size_t ndata, uint32_t depth, uint8_t *coded_dev, size_t ncoded);
AETH_API int aeth_rs_decode(aeth_rs *rs, const uint8_t *in_dev, size_t nin, const uint8_t *era_dev, uint32_t depth, uint32_t flags,
                            uint8_t *out_dev, size_t nout, aeth_rs_record *rec_dev, aeth_rs_summary *summary_dev);

/* ---- Polar codes: encoder, successive-cancellation decoder with bit flips (no body in the reference) ---- */
/* The code of the 5G NR control channels (PDCCH, PBCH, PUCCH) and the short-block code (N <= 1024) that LDPC serves
 * badly, behind aeth_demod_soft and aeth_remap and in front of aeth_crc_check.  Everything is integer arithmetic and
 * defined byte for byte.
 *
 * The code.  N = 2^n with 3 <= n <= 10.  mask is N bytes on the host, each 0 (frozen) or 1 (information); K is the
 * number of ones, 1 <= K <= N.  Bits are one byte per bit, taken & 1.  Soft values are int8_t; positive means bit 0 is
 * likelier and 0 is an erasure, as in aeth_cc_decode and aeth_ldpc_decode.  Punctured positions enter as 0 and shortened
 * positions as +127, both through aeth_remap.
 *
 * Transform (natural order, no bit reversal; the 5G convention):
 *     x = u; for s = 0 .. n - 1: for every i with bit s of i clear: x[i] ^= x[i + 2^s].
 *
 * Encoder.  u[i] = 0 where mask[i] = 0; the K information bits of a codeword go to the ones of the mask in ascending i;
 * coded = transform(u).  nbits = F K and ncoded = F N, anything else is AETH_E_LEN; any byte alignment; overlapping
 * ranges AETH_E_ARG; F = 0 launches nothing.
 *
 * Decoder: successive cancellation with the min-sum f, all arithmetic int32.  Nothing saturates: a value d levels below
 * the channel is at most 128 * 2^d in magnitude, below 2^18.  dec(L[0..m), base):
 *     m = 1, the leaf i = base: frozen: u[i] = 0; information: u[i] = (L[0] < 0), inverted if i == flip.  Returns [u[i]].
 *     m > 1, h = m / 2, a = L[0..h), b = L[h..m):
 *         x1 = dec(f(a, b), base),  f(a, b) = sgn(a) sgn(b) min(|a|, |b|), 0 when either argument is 0
 *         x2 = dec(g, base + h),    g[j] = b[j] + a[j] if x1[j] == 0, else b[j] - a[j]
 *         returns [x1 ^ x2 | x2]
 * The codeword's result is dec(soft as int32, 0); its return value is the re-encoded decision x^.
 * flip_dev may be NULL; otherwise F uint32_t, 4-byte aligned (else AETH_E_ALIGN), one position per codeword.
 * AETH_POLAR_NONE, a frozen position or a value >= N never matches an information leaf: all three are legal and have no
 * effect, so device data needs no validation.  The output is the K information decisions in ascending i, with
 * AETH_POLAR_CODEWORD the N bits of x^.  Codewords are independent: a call cut at any codeword equals two calls byte for
 * byte, and nothing depends on the grouping getters.
 *
 * Record.  rec_dev may be NULL; 4-byte aligned, one aeth_polar_record per codeword: the four information leaves with the
 * least (|L|, i) in lexicographic order, ascending, L the value the leaf decided on in this pass; slots beyond K hold
 * 0xFFFFFFFF in both fields.  These are the SC-Flip candidates: decode, check the CRC (aeth_crc_check), and decode the
 * failed frames again with flip = index[r].
 *
 * Construction (host, no context).  aeth_polar_rank writes the N positions, most reliable first, by the integer
 * polarization weight W(i) = sum over j of bit_j(i) (q[j mod 4] << (j div 4)),
 * q = {4294967296, 5107605667, 6074001000, 7223245206} = round(2^(r/4) 2^32): larger W first, ties to the larger i
 * (there are none for n <= 10).  n = 3 gives 7 6 5 3 4 2 1 0.  count < N is AETH_E_LEN.  aeth_polar_mask sets the first
 * K positions of that order to 1.  aeth_polar_create takes any mask: a caller with the 5G sequence, or a design for one
 * SNR, passes their own.
 *
 * Refusals, each naming the value, before any device work: a null ctx, mask or out; n outside 3 .. 10
 * (AETH_E_UNSUPPORTED); a mask byte above 1 (AETH_E_ARG, naming the index); K = 0; wrong lengths (AETH_E_LEN); unknown
 * flag bits; ranges that share a byte; a misaligned flip_dev or rec_dev (AETH_E_ALIGN).  Getters return 0 for NULL and
 * aeth_polar_destroy(NULL) is AETH_OK.  All device calls are ordered on the context's stream and none waits.
 *
 * Kernel.  aeth_polar_lanes lanes share a codeword (4, 8 or 16, chosen at create from n) and a workgroup is one wave of
 * aeth_polar_group = 64 / lanes codewords on aeth_polar_lds_bytes of dynamic LDS.  Levels above `lanes` values are int16
 * in LDS, those below live in registers and exchange across lanes; partial sums are packed bits; the tree walk is a
 * schedule built at create, wholly frozen subtrees pruned.
 *
 * Not built: rate-1 / SPC / repetition node shortcuts (they skip the leaf values the record needs); the 5G reliability
 * sequence, sub-block interleaver and parity-check bits; systematic polar encoding; n > 10; an aeth_stream_op kind and
 * host-slice flavours.  List decoding is aeth_polar_list below. */
#define AETH_POLAR_CODEWORD 1u
#define AETH_POLAR_NONE 0xFFFFFFFFu
typedef struct aeth_polar_record { uint32_t index[4]; uint32_t abs[4]; } aeth_polar_record;
AETH_API int aeth_polar_rank(uint32_t n, uint32_t *order_out, size_t count);
AETH_API int aeth_polar_mask(uint32_t n, uint32_t K, uint8_t *mask_out, size_t count);
AETH_API int aeth_polar_create(aeth_ctx *ctx, uint32_t n, const uint8_t *mask, aeth_polar **out);
AETH_API int aeth_polar_destroy(aeth_polar *polar);
AETH_API size_t aeth_polar_n(const aeth_polar *polar);
AETH_API size_t aeth_polar_k(const aeth_polar *polar);
AETH_API uint32_t aeth_polar_lanes(const aeth_polar *polar);       /* lanes per codeword */
AETH_API uint32_t aeth_polar_group(const aeth_polar *polar);       /* codewords per decoder workgroup */
AETH_API size_t aeth_polar_lds_bytes(const aeth_polar *polar);     /* dynamic LDS of a decoder workgroup */
AETH_API int aeth_polar_encode(aeth_polar *polar, const uint8_t *bits_dev, size_t nbits, uint8_t *coded_dev, size_t ncoded);
AETH_API int aeth_polar_decode(aeth_polar *polar, const int8_t *soft_dev, size_t nsoft, const uint32_t *flip_dev, uint32_t flags,
                               uint8_t *bits_dev, size_t nbits, aeth_polar_record *rec_dev);

/* ---- Polar codes: successive-cancellation list decoder and the CRC's pick among its paths (no body in the reference) ---- */
/* The decoder the 5G control channels are specified around: L paths per codeword, and a CRC that chooses among them on the
 * device (aeth_crc_check over the F L rows, then aeth_polar_list_pick).  A handle of its own beside aeth_polar.  n, mask, N,
 * K and the bit and soft conventions are exactly those of aeth_polar_create; L is 1, 2, 4 or 8 (else AETH_E_ARG), and
 * 2^K < L is refused (AETH_E_ARG): the code has fewer words than paths.  Everything is integer arithmetic and defined byte
 * for byte.
 *
 * State.  An ordered list of A paths, A = 1 at the start.  A path holds its decisions u[0..i) and a metric PM (uint32_t,
 * 0 at the start).
 *
 * Leaf walk.  Leaves are taken in ascending i.  For path p, lambda_p is the value that dec of the SC definition above
 * reaches at leaf i under that path's own earlier decisions: the same f and g, and nothing saturates.
 *     frozen leaf: u_i = 0; PM_p += |lambda_p| if lambda_p < 0; the list order is unchanged.
 *     information leaf: each (p, b), b in {0, 1}, is a candidate of metric PM_p + (|lambda_p| if b != (lambda_p < 0), else
 *         0).  The candidates are sorted ascending by (metric, p, b); the first min(2 A, L) become the new list in that
 *         order, each with u_i = b.
 * Final order.  After leaf N - 1 the list is sorted once more by (PM, position); this matters when frozen leaves trail.
 *
 * Output.  Without AETH_POLAR_ALL path 0's K information decisions in ascending i, nbits = F K; with it all L paths in
 * list order, nbits = F L K.  With AETH_POLAR_CODEWORD the N re-encoded bits x^ = transform(u) take the place of the K
 * decisions.  Anything else is AETH_E_LEN.  Codewords are independent: a call cut at any codeword equals two calls byte
 * for byte, and nothing depends on the grouping getters.
 *
 * Record.  rec_dev may be NULL; 4-byte aligned, one aeth_polar_list_record per codeword: metric[0..L) the final metrics,
 * ascending, slots L .. 7 hold 0xFFFFFFFF.
 *
 * Two facts, both checked against a plain restatement (tests/polar_list_truth.py):
 *   - L = 1 is aeth_polar_decode with flip = NULL, byte for byte.
 *   - A finished path's metric equals sum over j of |soft_j| [x^_j != (soft_j < 0)] over its re-encoded codeword x^.
 *     Hence PM <= 128 N <= 2^17, and the sort key metric 2 L + 2 p + b fits 32 bits.
 * The same induction shows that a wholly frozen subtree adds sum over j of |v_j| [v_j < 0] over the node's own values
 * v; the kernel uses that instead of walking the subtree, the restatement walks every leaf.
 *
 * aeth_polar_list_pick.  rows_dev holds F L rows of row_bytes bytes (the ALL output, or the payload aeth_crc_check
 * stripped from it) and diff_dev that check's F L words.  Per codeword f: which[f] is the least r with diff[f L + r] == 0,
 * else AETH_POLAR_NONE; out row f is row which[f] of the codeword, or row 0 when none passes.  One pass; any alignment for
 * the bytes; diff_dev 8-byte and which_dev 4-byte aligned (else AETH_E_ALIGN); which_dev may be NULL.  1 <= L <= 8 here
 * (else AETH_E_ARG), row_bytes = 0 is AETH_E_LEN and row_bytes > 2^30 AETH_E_UNSUPPORTED; F = 0 launches nothing.
 *
 * Refusals as for aeth_polar, each naming the value, before any device work; getters return 0 for NULL and
 * aeth_polar_list_destroy(NULL) is AETH_OK.  All device calls are ordered on the context's stream and none waits.
 *
 * Kernel.  aeth_polar_list_lanes lanes share a path and lanes x paths <= 64 a codeword, which never leaves its wave; a
 * workgroup is one wave of aeth_polar_list_group = 64 / (lanes paths) codewords on aeth_polar_list_lds_bytes of dynamic LDS.
 * The paths walk one schedule in lockstep, each in the slot of its list position; a fork moves the registers and the packed
 * partial sums, never a level.  lanes is the largest T <= 16 with T L <= 64 and 2 T <= N until it is measured.
 *
 * Not built: rate-1 / SPC / repetition node shortcuts; L > 8; the 5G sequence and parity-check bits; n > 10; an
 * aeth_stream_op kind and host-slice flavours; a summary of the pick. */
#define AETH_POLAR_ALL 2u
typedef struct aeth_polar_list_record { uint32_t metric[8]; } aeth_polar_list_record;
AETH_API int aeth_polar_list_create(aeth_ctx *ctx, uint32_t n, const uint8_t *mask, uint32_t L, aeth_polar_list **out);
AETH_API int aeth_polar_list_destroy(aeth_polar_list *list);
AETH_API size_t aeth_polar_list_n(const aeth_polar_list *list);
AETH_API size_t aeth_polar_list_k(const aeth_polar_list *list);
AETH_API uint32_t aeth_polar_list_paths(const aeth_polar_list *list);     /* L */
AETH_API uint32_t aeth_polar_list_lanes(const aeth_polar_list *list);     /* lanes per path */
AETH_API uint32_t aeth_polar_list_group(const aeth_polar_list *list);     /* codewords per workgroup */
AETH_API size_t aeth_polar_list_lds_bytes(const aeth_polar_list *list);   /* dynamic LDS of a workgroup */
AETH_API int aeth_polar_list_decode(aeth_polar_list *list, const int8_t *soft_dev, size_t nsoft, uint32_t flags, uint8_t *bits_dev,
                                    size_t nbits, aeth_polar_list_record *rec_dev);
AETH_API int aeth_polar_list_pick(aeth_ctx *ctx, const uint8_t *rows_dev, size_t row_bytes, size_t F, uint32_t L, const uint64_t *diff_dev,
                                  uint8_t *out_dev, uint32_t *which_dev);

/* ---- Turbo codes: RSC encoder, windowed max-log-MAP iterative decoder (no body in the reference) ---- */
/* The channel code of the LTE and UMTS data channels and of CCSDS 131.0-B telemetry, behind aeth_demod_soft and aeth_remap
 * and in front of aeth_crc_check.  Everything is integer arithmetic and defined byte for byte.  Bits are one byte per bit,
 * taken & 1.  Soft values are int8_t; positive means bit 0 is likelier and 0 is an erasure.
 *
 * Constituent code.  Recursive systematic, constraint length 3 <= k <= 5, nu = k - 1, S = 2^nu states.  fb and ff are
 * polynomials below 2^k with the current bit as the MSB (as in aeth_cc); fb must have bits k - 1 and 0 set, ff bit 0.
 * State s holds a[t-1] at bit nu - 1 down to a[t-nu] at bit 0.  Step t with input u:
 *     a = u ^ parity(s & fb & (S - 1));  reg = a 2^nu + s;  z = parity(reg & ff);  s' = reg >> 1.
 * aeth_turbo_named knows "lte" (also UMTS: k = 4, fb = 013, ff = 015), "ccsds" (k = 5, fb = 023, ff = 033) and "k3"
 * (k = 3, fb = 07, ff = 05, the test code).
 *
 * Encoder.  8 <= K <= 8192 information bits u and a permutation pi of K entries.  Encoder 1 runs on u[i], encoder 2 on
 * u[pi[i]], both from state 0; each is then terminated by nu tail steps with u_tail = parity(s & fb & (S - 1)), which
 * forces a = 0 and ends in state 0, and each tail step emits (u_tail, z).  A coded frame has N = 3 K + 4 nu bytes, planar:
 *     [0, K) u;  [K, 2K) z of encoder 1;  [2K, 3K) z' of encoder 2;
 *     3K + 2j, 3K + 2j + 1: tail (x, z) of encoder 1, j < nu;  3K + 2 nu + 2j, + 1: tail (x', z') of encoder 2.
 * LTE's d0 / d1 / d2 order with its multiplexed tail is an aeth_remap table of period N.
 *
 * One soft-in soft-out pass siso(x, p).  x[t] (systematic plus a-priori) and p[t] (parity) are int32 for t < K + nu; all
 * arithmetic is int32; NEG = -2^28.  The branch from s with input u carries g = (1 - 2u) x[t] + (1 - 2 z(s, u)) p[t].
 * Forward and backward recursions take the max over the two branches into a state or out of it.  The K information steps
 * are cut into windows [w W, min((w + 1) W, K)) with end e; window W and warm-up A are set at create.
 *     Forward.   If w W - A <= 0 start at step 0 with alpha = {0, NEG, ...}, else at step w W - A with all states 0.
 *     Backward.  If e + A >= K start at step K + nu with beta = {0, NEG, ...} and run back through the tail, else at step
 *                e + A with all states 0.
 *     Output.    D[t] = max_s(alpha_t[s] + g(0) + beta_{t+1}[s'(s, 0)]) - max_s(alpha_t[s] + g(1) + beta_{t+1}[s'(s, 1)]).
 * W >= K, or A >= K, is the exact max-log-MAP of the terminated trellis.  Windows do not depend on each other, so the
 * result does not depend on how a kernel distributes them.  Nothing overflows: |x| <= 128 + 2047, |p| <= 128, a path stays
 * below 1.9e7, alpha + g + beta above -2^31 even with two sentinels, and both hypotheses are always finite.
 *
 * Iterations.  scale(e) = sign(e) min((3 |e|) >> 3, 2047).  Per codeword: systematic s[0 .. K), parities p1 and p2 each
 * followed by its tail parities, tail systematics t1 and t2, a1 = 0.  Iteration i = 1 .. max_iter:
 *     x1 = s + a1;  D1 = siso(x1 | t1, p1)  (tail steps carry no a-priori);  e1 = D1 - 2 x1;  a2[i] = scale(e1)[pi[i]];
 *     x2[i] = s[pi[i]] + a2[i];  D2 = siso(x2 | t2, p2);  e2 = D2 - 2 x2;  a1[pi[i]] = scale(e2)[i];
 *     h1 = D1 < 0;  h2[pi[i]] = D2[i] < 0  (zero decides bit 0);  disagreements = #{h1 != h2}.
 * With AETH_TURBO_EARLY a codeword stops after an iteration with disagreements == 0.  The output is h2 of the last
 * iteration run, K bytes per codeword; rec_dev (may be NULL, 4-byte aligned) receives {iterations run, disagreements after
 * the last} per codeword.  Codewords are independent: a call cut at any codeword equals two calls byte for byte.
 *
 * aeth_turbo_qpp fills pi[i] = (f1 i + f2 i^2) mod K in 64-bit arithmetic (host, no context): K outside 8 .. 8192 and a
 * result that is no permutation are AETH_E_ARG, count < K AETH_E_LEN; a refused call writes nothing.
 *
 * Refusals, each naming the value, before any device work.  Create: k outside 3 .. 5 (AETH_E_UNSUPPORTED); a bad fb or ff;
 * K outside 8 .. 8192; window = 0 or warmup > 8192; pi NULL, an entry >= K or a repeated entry (naming index and value);
 * more than 1024 windows per codeword (AETH_E_UNSUPPORTED).  Encode: nbits != F K or ncoded != F N (AETH_E_LEN).  Decode:
 * max_iter outside 1 .. 64; unknown flag bits; nsoft != F N or nbits != F K (AETH_E_LEN); ranges that share a byte; a
 * misaligned rec_dev (AETH_E_ALIGN); 2^31 or more workgroups of aeth_turbo_group codewords (AETH_E_UNSUPPORTED).  soft and
 * bits may have any byte alignment; F = 0 launches nothing.  Getters return 0 for NULL, aeth_turbo_destroy(NULL) is
 * AETH_OK.  All device calls are ordered on the context's stream and none waits.
 *
 * Kernel.  A lane owns one window with all S state metrics in registers; a workgroup owns aeth_turbo_group codewords on
 * aeth_turbo_lds_bytes of dynamic LDS (the frame's soft values, the interleaved systematics and both a-priori arrays stay
 * there for the whole call) and keeps the forward metrics of its windows as int32 in device memory the object owns,
 * [step][state][lane].  The object also owns pi and its inverse on the device.
 *
 * Not built: soft posterior output; true log-MAP with a correction table; next-iteration initialisation of window edges;
 * duo-binary (DVB-RCS) codes; K > 8192 (which rules out CCSDS K = 8920); the LTE (f1, f2) catalogue and sub-block rate
 * matching; an aeth_stream_op kind and host-slice flavours. */
#define AETH_TURBO_EARLY 1u
typedef struct aeth_turbo_code { uint32_t k, fb, ff; } aeth_turbo_code;
typedef struct aeth_turbo_record { uint32_t iterations, disagreements; } aeth_turbo_record;
AETH_API int aeth_turbo_named(const char *name, aeth_turbo_code *code_out);
AETH_API int aeth_turbo_qpp(uint32_t K, uint32_t f1, uint32_t f2, uint32_t *pi_out, size_t count);
AETH_API int aeth_turbo_create(aeth_ctx *ctx, const aeth_turbo_code *code, uint32_t K, const uint32_t *pi_host, uint32_t window,
                               uint32_t warmup, aeth_turbo **out);
AETH_API int aeth_turbo_destroy(aeth_turbo *turbo);
AETH_API size_t aeth_turbo_k(const aeth_turbo *turbo);             /* information bits of a codeword */
AETH_API size_t aeth_turbo_n(const aeth_turbo *turbo);             /* coded bytes of a codeword, 3 K + 4 nu */
AETH_API uint32_t aeth_turbo_states(const aeth_turbo *turbo);
AETH_API uint32_t aeth_turbo_window(const aeth_turbo *turbo);
AETH_API uint32_t aeth_turbo_warmup(const aeth_turbo *turbo);
AETH_API uint32_t aeth_turbo_windows(const aeth_turbo *turbo);     /* windows, and decoder lanes, per codeword */
AETH_API uint32_t aeth_turbo_group(const aeth_turbo *turbo);       /* codewords per decoder workgroup */
AETH_API size_t aeth_turbo_lds_bytes(const aeth_turbo *turbo);     /* dynamic LDS of a decoder workgroup */
AETH_API int aeth_turbo_encode(aeth_turbo *turbo, const uint8_t *bits_dev, size_t nbits, uint8_t *coded_dev, size_t ncoded);
AETH_API int aeth_turbo_decode(aeth_turbo *turbo, const int8_t *soft_dev, size_t nsoft, uint32_t max_iter, uint32_t flags, uint8_t *bits_dev,
                               size_t nbits, aeth_turbo_record *rec_dev);

/* ---- OFDM symbols (no body in the reference: it has Fft, VecOps::vec_mul and chunks_mut(fft_len) framing only) ---- */
/* The framing and the one-tap equaliser of an OFDM link; everything else such a link needs is above (aeth_seq_scramble,
 * aeth_cc_*, aeth_modulate, aeth_demod_soft, aeth_corr_search on a preamble, aeth_sync_lag at lag = n_fft with
 * aeth_sync_freq_step(r, 1, n_fft) for the fractional carrier offset, aeth_nco_mix to remove it).
 *
 * An object is a transform length N = n_fft, a cyclic prefix of G = cp samples (0 <= G <= N), so a symbol of L = N + G
 * samples, and a carrier list: bins[k] is the FFT bin of carrier k, in the caller's output order; K = n_bins entries,
 * distinct and below N.
 *
 * Demod.  Symbol s is the window in[s L + e], e < N; the caller points in_dev at the first window sample (a timing
 * advance into the prefix is pointer arithmetic, and the phase ramp it leaves is part of the channel the estimator sees).
 * n_in >= aeth_ofdm_span(n_sym) = (n_sym - 1) L + N samples are read.  Y[s] is the transform of the window with the sign
 * of Fft::fwd (AETH_SIGN_REF_FWD) and the Scale of the call, exactly the bins aeth_fft_exec gives for the same N samples.
 *     out[s K + k] = Y[s][bins[k]]                                                 eq_dev NULL
 *     out[s K + k] = (Y.re W.re - Y.im W.im,  Y.re W.im + Y.im W.re),  W = eq[k]   otherwise
 * every f32 operation rounded on its own: the product aeth_vec_mul_frames makes.
 *
 * Mod.  Each symbol's grid is zero except grid[bins[k]] = car[s K + k]; it is transformed with the sign of Fft::bwd and the
 * Scale of the call; time sample e goes to out[s L + G + e] and the last G of them also to out[s L + e - (N - G)].
 * n_car = n_sym K, n_out = n_sym L.  mod followed by demod with AETH_SCALE_N on one side returns the carriers.
 *
 * Estimate.  y_dev holds n_sym received training symbols of K carriers (what demod wrote), x_dev the known ones: x_sym = 1
 * (one symbol, repeated) or x_sym = n_sym.  Per carrier k, with xs = (x_sym == 1 ? 0 : s), in f64, s ascending, both sums
 * starting from +0.0, the operands widened f32 values (so every term is ONE rounding with or without fma):
 *     num += (yr xr + yi xi,  yi xr - yr xi)            Y[s,k] conj(X[xs,k])
 *     den += xr xr + xi xi
 *     H   = ((float)(num.re / den), (float)(num.im / den)), (0, 0) where den == 0
 *     p   = hr hr + hi hi  from the rounded H widened again;   d = p + (eq_kind == AETH_OFDM_EQ_MMSE ? (double)nv : 0)
 *     W   = ((float)(hr / d), (float)(-hi / d)), (0, 0) where d == 0;   AETH_OFDM_EQ_MATCHED: W = (hr, -hi)
 *     csi = (float)p
 * h_dev[k] = H, eq_dev[k] = W, csi_dev[k] = csi; any of the three may be NULL, not all.  MATCHED turns PSK carriers into
 * CSI-weighted soft values for aeth_demod_soft with no further work.
 *
 * Routes.  "fused": N in {64, 128, 256, 512, 1024, 2048, 4096} -- one kernel per call, 8 (N + K) bytes per symbol (8 (L + K)
 * for mod).  "general: <aeth_fft_route of the inner plan>": every other length aeth_fft_create accepts, and every length
 * with AETH_OFDM_GENERAL -- windows copied to a scratch of n_sym N samples (sized at create from max_symbols; grown on
 * demand when max_symbols is 0), the plan's transform, then the pick.  Both give the same bytes, and the bytes of
 * aeth_fft_exec on the windows followed by aeth_vec_mul_frames.
 *
 * All calls are ordered on the context's stream and none waits.  Everything is validated before any device work: a NULL
 * handle or pointer AETH_E_ARG; n_fft < 2, cp > n_fft, n_bins == 0 or > n_fft, a bin >= n_fft or listed twice, unknown flags
 * AETH_E_ARG, the message naming the value; a length aeth_fft_create refuses: its status; n_sym above a non-zero max_symbols
 * AETH_E_ARG; n_in < span, n_out or n_car not n_sym K resp. n_sym L AETH_E_LEN; x_sym not 1 or n_sym AETH_E_ARG; pointers
 * 8-byte aligned (AETH_E_ALIGN; csi_dev 4); an output range that shares a byte with an input AETH_E_ARG (in place is not
 * supported).  n_sym == 0 is an empty success for demod and mod; an estimate from no symbols is AETH_E_LEN. */
enum { AETH_OFDM_GENERAL = 1 };          /* create flag: never take the fused route (verification, measurement) */
enum { AETH_OFDM_EQ_ZF = 0, AETH_OFDM_EQ_MMSE = 1, AETH_OFDM_EQ_MATCHED = 2 };
AETH_API int aeth_ofdm_create(aeth_ctx *ctx, size_t n_fft, size_t cp, const uint32_t *bins_host, size_t n_bins, size_t max_symbols,
                              int flags, aeth_ofdm **out);
AETH_API int aeth_ofdm_destroy(aeth_ofdm *ofdm);
AETH_API size_t aeth_ofdm_len(const aeth_ofdm *ofdm);
AETH_API size_t aeth_ofdm_cp(const aeth_ofdm *ofdm);
AETH_API size_t aeth_ofdm_symbol(const aeth_ofdm *ofdm);       /* n_fft + cp */
AETH_API size_t aeth_ofdm_carriers(const aeth_ofdm *ofdm);
AETH_API const char *aeth_ofdm_route(const aeth_ofdm *ofdm);   /* "fused" or "general: " + the inner plan's aeth_fft_route */
AETH_API size_t aeth_ofdm_span(const aeth_ofdm *ofdm, size_t n_sym);   /* samples demod reads; 0 for n_sym = 0 */
AETH_API int aeth_ofdm_demod(aeth_ofdm *ofdm, const aeth_cf32 *in_dev, size_t n_in, size_t n_sym, const aeth_cf32 *eq_dev,
                             int scale_kind, float x, aeth_cf32 *out_dev, size_t n_out);
AETH_API int aeth_ofdm_mod(aeth_ofdm *ofdm, const aeth_cf32 *car_dev, size_t n_car, size_t n_sym, int scale_kind, float x,
                           aeth_cf32 *out_dev, size_t n_out);
AETH_API int aeth_ofdm_estimate(aeth_ofdm *ofdm, const aeth_cf32 *y_dev, const aeth_cf32 *x_dev, size_t n_sym, size_t x_sym, float nv,
                                int eq_kind, aeth_cf32 *h_dev, aeth_cf32 *eq_dev, float *csi_dev);

/* ---- pinned host buffers: src/pool.rs:43-221 -------------------------------------------------- */
/* The reference's object pool ("useful for large buffers and other time expensive objects", :9-10) with pinned
 * (hipHostMalloc) elements of elem_bytes each: the maker allocates one element, the resetter optionally zeroes it.
 * Samples produced INTO pool elements (file reads, receivers, generators) cross PCIe with true asynchronous copies
 * and no staging; the library never page-locks memory it did not allocate unless asked to (aeth_host_register).
 * Thread-safe like the reference's Arc<Mutex<..>> (take / give_back from any thread). */
enum { AETH_POOL_ZERO_ON_RETURN = 1 };                                  /* resetter: memset 0 (pool.rs:47,175-178) */
AETH_API int aeth_pool_create(aeth_ctx *ctx, size_t elem_bytes, size_t initial_len, int flags, aeth_pool **out); /* pool::make :43-69 */
AETH_API int aeth_pool_destroy(aeth_pool *pool);              /* refused (AETH_E_ARG) while elements are checked out   */
AETH_API int aeth_pool_take(aeth_pool *pool, void **buf);     /* Pool::take :78-97: *buf = NULL when the pool is empty */
AETH_API int aeth_pool_take_or_make(aeth_pool *pool, void **buf);       /* Pool::take_or_make :115-132 (grows the pool) */
AETH_API int aeth_pool_give_back(aeth_pool *pool, void *buf); /* Elem::drop -> give_back :175-208                      */
AETH_API size_t aeth_pool_len(aeth_pool *pool);               /* Pool::len :138-140: elements currently checked in     */
AETH_API size_t aeth_pool_cap(aeth_pool *pool);               /* Pool::cap :157-159: elements the pool owns            */
AETH_API size_t aeth_pool_elem_bytes(const aeth_pool *pool);
/* Explicit opt-in for memory the caller owns (no reference counterpart): page-lock [ptr, ptr + bytes) so that the
 * host pipeline copies from / to it directly.  The range must start on a page boundary and cover whole pages
 * (AETH_E_ALIGN) and must not touch a pool element or a range registered before (AETH_E_ARG); every runtime return
 * code is checked.  The caller keeps it alive and mapped until aeth_host_unregister has returned AETH_OK. */
AETH_API int aeth_host_register(aeth_ctx *ctx, void *ptr, size_t bytes);
AETH_API int aeth_host_unregister(aeth_ctx *ctx, void *ptr);
AETH_API int aeth_host_is_pinned(const void *ptr, size_t bytes);        /* 1: inside one pool element / registered range */

/* Host-resident stream through the device at PCIe rate (SURVEY 8f "next" #4): chunks through five stages -- copy-in
 * (caller slice -> pinned pool element, host threads) | upload | compute | download (three HIP streams, three device
 * slots handed on by events) | copy-out (host threads) -- so that both copy engines run back to back: the counterpart
 * of the reference's thread-per-stage pipeline over pooled buffers (src/pipeline.rs:52-137, src/pool.rs:43-221).
 *
 * The reference's pipeline takes any closure as a stage (src/pipeline.rs:24-41 `add_stage<F: FnMut(O) -> U>`,
 * :123-137 `new`); a closure cannot cross this boundary (as for vec_mutate), so the compute stage is described by an
 * aeth_stream_op: one of the library's device ops applied chunk by chunk.  Input and output differ per op:
 *   AETH_STREAM_FIR                 fir                      n cf32 in -> n cf32 out (hop-aligned chunks; = aeth_fir_exec)
 *   AETH_STREAM_FFT                 fft, sign, scale_kind_fwd / x_fwd          frames of len cf32 -> the same (= aeth_fft_exec)
 *   AETH_STREAM_FFT_MUL_IFFT        fft, sig_dev, both scales                  frames -> frames (= aeth_fft_mul_ifft)
 *   AETH_STREAM_FFT_MUL_IFFT_DEMOD  ... + bits_per_symbol, table_host, compat  8 B in -> bits_per_symbol BYTES out per sample
 *   AETH_STREAM_FFT_INTERPOLATE     fft, sign, scale, n_between, compat (= compat_im)   len in -> len + (len-1)*n_between out per frame
 *   AETH_STREAM_MODULATE_AWGN       bits_per_symbol, table_host, x_fwd = noise power, seed, offset   BIT BYTES in -> symbols out (= aeth_modulate_awgn;
 *                                   the one op whose input is not cf32: in_host holds n_in bytes; in a chain it has to be the first stage)
 *   AETH_STREAM_FIR_DECIM           fir, n_between = dec (must divide aeth_fir_hop and n_in)   n in -> n / dec out (= aeth_fir_exec_decim)
 * Every op's output is bit-identical to its device flavour on the whole slice.  n_in counts input samples, n_out
 * output ELEMENTS of the op's type and must equal aeth_stream_out_count(ctx, op, n_in) (AETH_E_LEN otherwise; the frame
 * ops need whole frames: "Input and FFT must be the same length").  The two host ranges must not overlap (AETH_E_ARG).
 *
 * A side that is already page-locked (aeth_host_is_pinned: a pool element, a registered range) skips its host stage
 * and is copied from / to directly; caller memory is never registered by these calls.  stats->pinned = 1 * (in direct)
 * + 2 * (out direct); an input that needs staging takes the output through the host stage as well (measured: the
 * mixed form is the slow one; AETH_PIPE_MIXED below).  chunk_samples = 0 picks 32 MiB on the larger side per chunk
 * (an eighth of a short stream, at least 1 MiB), rounded to whole hops / frames.
 *
 * What a context keeps between calls: the three stage streams, three device slots per side, three pinned staging
 * elements per side (only for pageable caller memory) and the copy threads, sized by the largest chunk seen.  A slot is
 * at most 64 MiB (a larger chunk_samples is split internally; one frame of more than that still gets its slot), so the
 * retained memory is bounded by 6 x 64 MiB of device memory and 6 x 64 MiB of pinned memory; aeth_ctx_trim gives all
 * of it back (and the device scratch of the host-slice flavours), aeth_ctx_destroy does the same. */
typedef struct { double seconds, samples, chunks, pinned; } aeth_pipe_stats;
enum { AETH_STREAM_FIR = 0, AETH_STREAM_FFT = 1, AETH_STREAM_FFT_MUL_IFFT = 2, AETH_STREAM_FFT_MUL_IFFT_DEMOD = 3,
       AETH_STREAM_FFT_INTERPOLATE = 4, AETH_STREAM_FIR_DECIM = 5, AETH_STREAM_MODULATE_AWGN = 6 };
typedef struct aeth_stream_op {
    int kind;                          /* AETH_STREAM_*                                                          */
    aeth_fir *fir;                     /* FIR                                                                    */
    aeth_fft *fft;                     /* the frame ops: frames of aeth_fft_len(fft) samples                     */
    const aeth_cf32 *sig_dev;          /* MUL_IFFT, MUL_IFFT_DEMOD: the multiplier, DEVICE memory, n_sig = len   */
    size_t n_sig;
    int sign;                          /* FFT, FFT_INTERPOLATE: AETH_SIGN_REF_FWD / _BWD                         */
    int scale_kind_fwd; float x_fwd;   /* Scale of the (forward) transform                                       */
    int scale_kind_bwd; float x_bwd;   /* MUL_IFFT, MUL_IFFT_DEMOD: Scale of the way back                        */
    int bits_per_symbol;               /* MUL_IFFT_DEMOD: 1 (BPSK) or 2 (QPSK)                                   */
    const aeth_cf32 *table_host;       /*   symbol table (host), NULL = the generic tables                       */
    int compat;                        /*   as aeth_demod_naive; FFT_INTERPOLATE: compat_im of aeth_interpolate  */
    size_t n_between;                  /* FFT_INTERPOLATE; FIR_DECIM: the decimation                             */
    uint64_t seed, offset;             /* MODULATE_AWGN: noise stream and the position of the first symbol in it  */
} aeth_stream_op;
AETH_API size_t aeth_stream_out_count(aeth_ctx *ctx, const aeth_stream_op *op, size_t n_in);   /* 0 for a bad op */
AETH_API int aeth_stream_host(aeth_ctx *ctx, const aeth_stream_op *op, const void *in_host, size_t n_in,
                              void *out_host, size_t n_out, size_t chunk_samples, aeth_pipe_stats *stats);
/* The same run with the per-stage report of the reference's pipeline (src/pipeline.rs:89-114: items processed, rate and
 * "Utilisation" = time active / time elapsed, per stage): seconds each of the stages was busy -- upload, compute, download
 * from timed events around every stage operation, the two host stages from the wall clock between hand-over and completion
 * of each chunk.  Utilisation of a stage = active_x / seconds. */
typedef struct { double seconds, samples, chunks, pinned, active_upload, active_kernel, active_download,
                 active_copy_in, active_copy_out; /* the two host stages (0 for a side copied directly) */ } aeth_pipe_util;
AETH_API int aeth_stream_host_util(aeth_ctx *ctx, const aeth_stream_op *op, const void *in_host, size_t n_in,
                                   void *out_host, size_t n_out, size_t chunk_samples, aeth_pipe_util *util);
/* Several ops as ONE compute stage -- `pipeline::new(..).add_stage(a).add_stage(b)` (src/pipeline.rs:24-41): stage i's output
 * is stage i + 1's input on the device, only the first stage sees host data and only the last one's output goes back (so
 * e.g. FIR -> FFT frames -> correlate + demod moves 8 B up and 2 B down per sample).  1 .. 8 ops; a filter can only be the
 * first stage, a stage that emits bits only the last; n_in has to be a whole number of the chain's granule (the smallest
 * count every stage takes in whole hops / frames).  Bit-identical to the ops' device flavours applied one after the
 * other.  stats and util may each be NULL. */
AETH_API size_t aeth_stream_chain_out_count(aeth_ctx *ctx, const aeth_stream_op *ops, size_t n_ops, size_t n_in);
AETH_API int aeth_stream_host_chain(aeth_ctx *ctx, const aeth_stream_op *ops, size_t n_ops, const void *in_host, size_t n_in,
                                    void *out_host, size_t n_out, size_t chunk_samples, aeth_pipe_stats *stats,
                                    aeth_pipe_util *util);
/* AETH_STREAM_FIR with the filter as the only argument (output bit-identical to aeth_fir_exec_host on the whole slice) */
AETH_API int aeth_fir_stream_host(aeth_fir *fir, const aeth_cf32 *in_host, size_t n, aeth_cf32 *out_host,
                                  size_t chunk_samples, aeth_pipe_stats *stats);
AETH_API int aeth_fir_stream_host_util(aeth_fir *fir, const aeth_cf32 *in_host, size_t n, aeth_cf32 *out_host,
                                       size_t chunk_samples, aeth_pipe_util *util);
/* Releases what the context retains between calls (see above); the next call that needs it creates it again. */
AETH_API int aeth_ctx_trim(aeth_ctx *ctx);
/* Test support (tests/test_gpu_pool.py): the n-th pinned staging element the pipeline takes from now on fails right
 * after it has been taken (once), so that the give-back of every error path can be checked. */
AETH_API void aeth_test_fail_staging_after(int n);

/* ---- raw sample files (SURVEY 8f "next" #3): src/util/file.rs:12-107 ------------------------ */
/* The reference's binary files are header-less native-endian dumps of back-to-back structs;
 * for cf32 that is exactly the byte layout of a device buffer. */
AETH_API int aeth_file_count_structs(const char *path, size_t elem_size, size_t *count);            /* :12-25  */
AETH_API int aeth_file_read(const char *path, size_t offset_structs, void *dst_host, size_t n, size_t elem_size);  /* BinaryReader::read :46-57 */
AETH_API int aeth_file_write(const char *path, const void *src_host, size_t n, size_t elem_size, int append);      /* binary_writer + write :83-109 */
/* raw cf32 file -> one of the pipeline's ops -> raw file of its output type (cf32, or bit bytes for the demodulating stage)
 * through the pipeline above (both files mapped; the two paths must not name the same file) */
AETH_API int aeth_stream_file(aeth_ctx *ctx, const aeth_stream_op *op, const char *in_path, const char *out_path,
                              size_t chunk_samples, aeth_pipe_stats *stats);
/* raw cf32 file -> FIR -> raw cf32 file */
AETH_API int aeth_fir_stream_file(aeth_fir *fir, const char *in_path, const char *out_path, size_t chunk_samples,
                                  aeth_pipe_stats *stats);

/* ---- sampling: src/sampling.rs ---------------------------------------------- */
/* interpolate (:7-24): writes n_src + (n_src-1)*n_between elements to dst
 * (the Rust wrapper reserves that much spare Vec capacity, passes its end, then
 * set_len's: the reference APPENDS, :17,:23).  compat_im != 0 reproduces
 * `im: x1.re + i*rate.1` (:19).  n_src == 0 -> AETH_E_LEN (reference panics, :23). */
AETH_API int aeth_interpolate(aeth_ctx *ctx, const aeth_cf32 *src_dev, size_t n_src,
                              aeth_cf32 *dst_dev, size_t dst_capacity, size_t n_between,
                              int compat_im, size_t *n_written);
/* the same for `batch` independent frames of frame_len (BASELINE config 5) */
AETH_API int aeth_interpolate_frames(aeth_ctx *ctx, const aeth_cf32 *src_dev, size_t frame_len,
                                     size_t batch, aeth_cf32 *dst_dev, size_t dst_capacity,
                                     size_t n_between, int compat_im, size_t *n_written);
AETH_API int aeth_host_interpolate(aeth_ctx *ctx, const aeth_cf32 *src, size_t n_src,
                                   aeth_cf32 *dst, size_t dst_capacity, size_t n_between,
                                   int compat_im, size_t *n_written);
/* downsample / downsample_sb (:28-42 / :49-62): dst[i] = src[i*(n_src/n_dst)],
 * generic T: Copy via elem_size (1,2,4,8,16 bytes).  n_src % n_dst != 0 ->
 * AETH_E_LEN with "Only even decimations are supported" (:32-36). */
AETH_API int aeth_downsample(aeth_ctx *ctx, const void *src_dev, size_t n_src,
                             void *dst_dev, size_t n_dst, size_t elem_size);
AETH_API int aeth_host_downsample(aeth_ctx *ctx, const void *src, size_t n_src,
                                  void *dst, size_t n_dst, size_t elem_size);
/* The two entry points above are the reference as `cargo build` / `cargo test` compile it (DEBUG build): the
 * divisibility check of :32-36 is a debug_assert_eq! and panics there.  The two below are the reference as
 * `cargo build --release` / `cargo bench` compile it (RELEASE build, the one its own benchmark runs at
 * benches/benches.rs:113,130 with the shape 8096 -> 512): the assert is compiled out, dec = n_src / n_dst FLOORS and
 * dst[i] = src[i*dec] for every i < n_dst (:38-41).  What still panics in a release build is an error here too
 * (AETH_E_LEN): n_dst == 0 (division by zero), n_src == 0 (src[0] out of bounds); n_src < n_dst gives dec = 0, which
 * downsample runs as dst[i] = src[0] and downsample_sb (step_by != 0) refuses, as step_by(0) panics (:58-61). */
AETH_API int aeth_downsample_release(aeth_ctx *ctx, const void *src_dev, size_t n_src,
                                     void *dst_dev, size_t n_dst, size_t elem_size, int step_by);
AETH_API int aeth_host_downsample_release(aeth_ctx *ctx, const void *src, size_t n_src,
                                          void *dst, size_t n_dst, size_t elem_size, int step_by);

/* ---- modulation (SURVEY 8f "next" #1): src/modulation.rs --------------------------- */
/* Modulation::modulate (:115-121): one symbol per `bits_per_symbol` input bytes (each byte is
 * one bit, taken modulo 2 as the trait's default index() does, :107); index =
 * bits[0] for BPSK (:9-12), (bits[1] << 1) + bits[0] for QPSK (:21-24); out[s] = table[index].
 * table_host: 2 or 4 symbols, NULL = GENERIC_BPSK_TABLE / GENERIC_QPSK_TABLE (:77-92).
 * nbits must be a multiple of bits_per_symbol (AETH_E_LEN) and n_out == nbits / bits_per_symbol. */
AETH_API int aeth_modulate(aeth_ctx *ctx, const uint8_t *bits_dev, size_t nbits, int bits_per_symbol,
                           const aeth_cf32 *table_host, aeth_cf32 *out_dev, size_t n_out);
/* modulate followed by Awgn::apply on the fresh symbols (examples/modem.rs:19-26) in one pass over memory:
 * out[s] = table[index] + (z * scale) * scale with z = position offset + s of stream `seed` (see aeth_awgn_apply).
 * BPSK / QPSK tables; bit-identical to aeth_modulate + aeth_awgn_apply. */
AETH_API int aeth_modulate_awgn(aeth_ctx *ctx, const uint8_t *bits_dev, size_t nbits, int bits_per_symbol,
                                const aeth_cf32 *table_host, aeth_cf32 *out_dev, size_t n_out, float power,
                                uint64_t seed, uint64_t offset);
/* Modulation::demod_naive: nearest table symbol by squared distance, folded exactly as the reference's
 * min_by(|d, e| d.partial_cmp(e).unwrap_or(Ordering::Greater)) (:46, :139): of equal distances the FIRST stays, a
 * strictly smaller one replaces it, and so does an unordered pair -- a sample with a NaN component decodes as the
 * last candidate scanned.  compat != 0 reproduces the QPSK specialisation's
 * output exactly (:33-56): it pushes `idx & 1` and `idx & 1u8 << 1` == idx & 2, i.e. the
 * second bit comes out as 0 or 2; compat == 0 emits (idx >> 1) & 1.  BPSK follows the
 * trait default (:133-144).  bits_out_dev receives nsym * bits_per_symbol bytes. */
AETH_API int aeth_demod_naive(aeth_ctx *ctx, const aeth_cf32 *sym_dev, size_t nsym, int bits_per_symbol,
                              const aeth_cf32 *table_host, uint8_t *bits_out_dev, size_t nbits_out, int compat);
/* No body in the reference (hence no `compat`): soft decisions for aeth_cc_decode.  bits_per_symbol 1 .. 8 and the tables
 * of aeth_modulate (NULL: the generic BPSK / QPSK table).  For bit i of the index, at out[bits_per_symbol * s + i]:
 *     L = (min_{idx: bit i = 1} d2(idx) - min_{idx: bit i = 0} d2(idx)) * scale
 * with dre = sym.re - table[idx].re, dim likewise, d2 = dre * dre + dim * dim, every operation f32 and rounded on its
 * own; each minimum starts at +Inf and is a running `d < best ? d : best` over ascending idx.  The output is rintf(L)
 * clamped to [-127, 127]; NaN gives 0.  Positive means bit 0 is likelier.  nout != nsym * bits_per_symbol: AETH_E_LEN. */
AETH_API int aeth_demod_soft(aeth_ctx *ctx, const aeth_cf32 *sym_dev, size_t nsym, int bits_per_symbol,
                             const aeth_cf32 *table_host, float scale, int8_t *out_dev, size_t nout);

/* ---- noise (SURVEY 8f "next" #1): src/noise.rs ------------------------------------- */
/* Awgn::apply (:53-59) on a device-resident signal: s[i] += next().scale(scale) with
 * scale = sqrt(power) (:35) and next() = (z.re * scale, z.im * scale) (:39-43) -- the
 * reference scales twice, so the noise amplitude is proportional to `power`; reproduced.
 * z comes from the library's own counter-based generator (Philox4x32-7 + Box-Muller,
 * position `offset + i` of stream `seed`; DEFAULT seed of the reference is 815, :6): the
 * reference's StdRng stream is not reproducible, results agree bit for bit with the CPU
 * restatement of THIS generator only.  Consecutive calls continue a stream by passing
 * offset += n, as the reference's generator object would. */
AETH_API int aeth_awgn_apply(aeth_ctx *ctx, aeth_cf32 *signal_dev, size_t n, float power, uint64_t seed,
                             uint64_t offset);
/* Awgn::fill / Awgn::iter (src/noise.rs:61-84): target[i] = next() = (z.re * scale, z.im * scale) -- scaled
 * ONCE, unlike apply -- for positions offset .. offset+n of stream `seed`.  The reference fills a Vec up to its
 * capacity; here the capacity is `n`. */
AETH_API int aeth_awgn_fill(aeth_ctx *ctx, aeth_cf32 *target_dev, size_t n, float power, uint64_t seed,
                            uint64_t offset);
/* The generator's integer stage by itself (replaces rand::StdRng, src/noise.rs:2-4,23,33): out[i][0..3] =
 * Philox4x32-R of counter ctr_key[i][0..3] under key ctr_key[i][4..5] (Salmon et al., SC'11), R = 7 (what the
 * generator draws with since round 4: the smallest Crush-resistant round count of this width) or 10; the Random123
 * known-answer vectors of both are in tests/golden/philox4x32_{7,10}_kat.json.  Device pointers, n x 6 and n x 4 words. */
AETH_API int aeth_rng_philox4x32(aeth_ctx *ctx, const uint32_t *ctr_key_dev, size_t n, int rounds, uint32_t *out_dev);
AETH_API int aeth_rng_philox4x32_10(aeth_ctx *ctx, const uint32_t *ctr_key_dev, size_t n, uint32_t *out_dev);
/* The generator's floating-point stage by itself (replaces rand_distr::Normal, src/noise.rs:3,39-43): out[i] = the
 * complex standard normal the generator makes of the 32-bit word pair (ab[i][0], ab[i][1]) -- radius from the first
 * word (u = ((a >> 8) | 1) / 2^24, r = sqrt(-2 ln u)), angle from the second.  Exists so that the stage can be pinned
 * over its WHOLE radius argument (all 2^24 values of a >> 8: the device takes r from v_rsq_f32 plus one correcting
 * step, the oracle from sqrtf) instead of on the samples a stream happens to draw; tests/test_gpu_modulation.py does
 * that.  Device pointers, n x 2 words in, n samples out. */
AETH_API int aeth_rng_normal_pairs(aeth_ctx *ctx, const uint32_t *ab_dev, size_t n, aeth_cf32 *out_dev);

#ifdef __cplusplus
}
#endif
#endif /* AETHER_HIP_H */
