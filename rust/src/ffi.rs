//! `extern "C"` declarations: one to one with include/aether_hip.h.
#![allow(non_camel_case_types)]
use aether_primitives::cf32;
use std::os::raw::{c_char, c_double, c_float, c_int, c_uint, c_void};

#[repr(C)] pub struct aeth_ctx { _p: [u8; 0] }
#[repr(C)] pub struct aeth_fft { _p: [u8; 0] }
#[repr(C)] pub struct aeth_fir { _p: [u8; 0] }
#[repr(C)] pub struct aeth_corr { _p: [u8; 0] }
#[repr(C)] pub struct aeth_seq { _p: [u8; 0] }
#[repr(C)] pub struct aeth_chan { _p: [u8; 0] }
#[repr(C)] pub struct aeth_synth { _p: [u8; 0] }
#[repr(C)] pub struct aeth_resamp { _p: [u8; 0] }
#[repr(C)] pub struct aeth_arb { _p: [u8; 0] }
#[repr(C)] pub struct aeth_cc { _p: [u8; 0] }
#[repr(C)] pub struct aeth_remap { _p: [u8; 0] }
pub const AETH_REMAP_ROUTE_TILE: c_int = 1; pub const AETH_REMAP_ROUTE_GATHER: c_int = 2;
#[repr(C)] pub struct aeth_crc { _p: [u8; 0] }
pub const AETH_CRC_ROUTE_FRAMES: c_int = 1; pub const AETH_CRC_ROUTE_LONG: c_int = 2;
pub const AETH_BITS_LSB_FIRST: c_int = 0; pub const AETH_BITS_MSB_FIRST: c_int = 1;
#[repr(C)] #[derive(Clone, Copy, Debug, Default, PartialEq, Eq)] pub struct aeth_crc_summary { pub n_bad: u64, pub first_bad: u64 }
#[repr(C)] pub struct aeth_ldpc { _p: [u8; 0] }
pub const AETH_LDPC_EARLY: u32 = 1; pub const AETH_LDPC_PAYLOAD: u32 = 2;
/// aeth_ldpc_code: rows x cols circulant blocks of size z; shift[rows * cols], row-major, -1 for a zero block
#[repr(C)] #[derive(Clone, Copy)] pub struct aeth_ldpc_code { pub rows: u32, pub cols: u32, pub z: u32, pub shift: *const i32 }
#[repr(C)] #[derive(Clone, Copy, Debug, Default, PartialEq, Eq)] pub struct aeth_ldpc_record { pub iterations: u32, pub unsatisfied: u32 }
#[repr(C)] pub struct aeth_rs { _p: [u8; 0] }
pub const AETH_RS_PAYLOAD: u32 = 1;
/// aeth_rs_code: RS(n, n - nroots) over GF(2^m); poly carries its x^m term
#[repr(C)] #[derive(Clone, Copy, Debug, Default, PartialEq, Eq)] pub struct aeth_rs_code { pub m: u32, pub poly: u32, pub fcr: u32, pub prim: u32, pub nroots: u32, pub n: u32 }
#[repr(C)] #[derive(Clone, Copy, Debug, Default, PartialEq, Eq)] pub struct aeth_rs_record { pub corrected: u32, pub status: u32 }
#[repr(C)] #[derive(Clone, Copy, Debug, Default, PartialEq, Eq)] pub struct aeth_rs_summary { pub n_failed: u64, pub n_corrected: u64 }
#[repr(C)] pub struct aeth_polar { _p: [u8; 0] }
#[repr(C)] pub struct aeth_polar_list { _p: [u8; 0] }
pub const AETH_POLAR_CODEWORD: u32 = 1; pub const AETH_POLAR_NONE: u32 = 0xFFFF_FFFF;
/// aeth_polar_record: the four information leaves with the least (|L|, i), ascending; empty slots hold 0xFFFFFFFF
#[repr(C)] #[derive(Clone, Copy, Debug, Default, PartialEq, Eq)] pub struct aeth_polar_record { pub index: [u32; 4], pub abs: [u32; 4] }
/// aeth_polar_list_record: the final metrics of the L paths, ascending; slots L .. 7 hold 0xFFFFFFFF
#[repr(C)] #[derive(Clone, Copy, Debug, Default, PartialEq, Eq)] pub struct aeth_polar_list_record { pub metric: [u32; 8] }
#[repr(C)] pub struct aeth_turbo { _p: [u8; 0] }
pub const AETH_TURBO_EARLY: u32 = 1;
/// aeth_turbo_code: a recursive systematic constituent code, constraint length k, polynomials with the current bit as the MSB
#[repr(C)] #[derive(Clone, Copy, Debug, Default, PartialEq, Eq)] pub struct aeth_turbo_code { pub k: u32, pub fb: u32, pub ff: u32 }
#[repr(C)] #[derive(Clone, Copy, Debug, Default, PartialEq, Eq)] pub struct aeth_turbo_record { pub iterations: u32, pub disagreements: u32 }
#[repr(C)] pub struct aeth_ofdm { _p: [u8; 0] }
#[repr(C)] pub struct aeth_event { _p: [u8; 0] }
#[repr(C)] pub struct aeth_pool { _p: [u8; 0] }
pub const AETH_POOL_ZERO_ON_RETURN: c_int = 1;
/// aeth_pipe_stats: what the three-stage host-stream pipeline reports
#[repr(C)] #[derive(Default, Clone, Copy)]
pub struct aeth_pipe_stats { pub seconds: f64, pub samples: f64, pub chunks: f64, pub pinned: f64 }
/// aeth_vec_step: one link of aeth_vec_chain (op = AETH_VEC_*)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct aeth_vec_step { pub op: c_int, pub other_dev: *const cf32, pub n_other: usize, pub scale: c_float }
pub const AETH_VEC_SCALE: c_int = 0; pub const AETH_VEC_MUL: c_int = 1; pub const AETH_VEC_DIV: c_int = 2; pub const AETH_VEC_CONJ: c_int = 3;
pub const AETH_VEC_ADD: c_int = 4; pub const AETH_VEC_SUB: c_int = 5; pub const AETH_VEC_CLONE: c_int = 6; pub const AETH_VEC_ZERO: c_int = 7;
/// aeth_vec_stats (the struct): what aeth_vec_stats / aeth_host_vec_stats (the functions) fill in
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aeth_vec_stats_t { pub n: usize, pub n_nan: usize, pub min_index: usize, pub max_index: usize, pub min_norm: c_float,
                              pub max_norm: c_float, pub mean_re: f64, pub mean_im: f64, pub power: f64 }
/// aeth_corr_peak: one record of aeth_corr_search (16 bytes, no padding)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aeth_corr_peak { pub index: usize, pub norm: c_float, pub n_nan: c_uint }
/// aeth_seq_reg: one register of a sequence object, seq[n] = XOR seq[n - delays[k]] (src/sequence.rs:42)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct aeth_seq_reg { pub delays: *const u32, pub ndelays: usize }
/// aeth_nco_words: an oscillator, each word a fraction of a turn scaled by 2^64; w(n) = phase + n step + n (n - 1) / 2 rate
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct aeth_nco_words { pub phase: u64, pub step: u64, pub rate: u64 }
/// aeth_sync_record: one block's (or the total's) complex f64 sum, the sum of the weights and the term counts; 48 bytes
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct aeth_sync_record { pub re: f64, pub im: f64, pub mass: f64, pub n: u64, pub n_nonfinite: u64, pub reserved: u64 }
/// aeth_mov_peak: the best candidate of a block of moving-window outputs (or of the call), the f64 sums there; 64 bytes
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq)]
pub struct aeth_mov_peak { pub index: u64, pub first: u64, pub p_re: f64, pub p_im: f64, pub r: f64, pub r_lag: f64, pub metric: f32,
                           pub n_nan: u32, pub reserved: u64 }
pub const AETH_MOV_LAG: c_int = 0; pub const AETH_MOV_POWER: c_int = 1;
/// aeth_cc_code: a rate 1/n convolutional code of constraint length k; polynomials in the octal convention, current bit at the MSB
#[repr(C)]
#[derive(Clone, Copy, Debug, Default, PartialEq, Eq)]
pub struct aeth_cc_code { pub k: u32, pub n: u32, pub poly: [u32; 4] }
pub const AETH_CHAN_PHASE_FRAME: c_int = 0; pub const AETH_CHAN_PHASE_STREAM: c_int = 1;
pub const AETH_CHAN_PROTO_RECT: c_int = 0; pub const AETH_CHAN_PROTO_HANN: c_int = 1; pub const AETH_CHAN_PROTO_HAMMING: c_int = 2;
pub const AETH_CHAN_PROTO_SINC_HAMMING: c_int = 3;
pub const AETH_LEVEL_NORM: c_int = 0; pub const AETH_LEVEL_DB: c_int = 1; pub const AETH_LEVEL_POWER_DB: c_int = 2;
/// aeth_stream_op: the compute stage of the host pipeline (src/pipeline.rs:24-41 takes a closure; a closure cannot
/// cross the C ABI, so the stage is one of the library's device ops, described field by field as in aether_hip.h)
#[repr(C)]
#[derive(Clone, Copy)]
pub struct aeth_stream_op { pub kind: c_int, pub fir: *mut aeth_fir, pub fft: *mut aeth_fft, pub sig_dev: *const cf32, pub n_sig: usize,
                            pub sign: c_int, pub scale_kind_fwd: c_int, pub x_fwd: c_float, pub scale_kind_bwd: c_int, pub x_bwd: c_float,
                            pub bits_per_symbol: c_int, pub table_host: *const cf32, pub compat: c_int, pub n_between: usize,
                            pub seed: u64, pub offset: u64 }
pub const AETH_STREAM_FIR: c_int = 0;
pub const AETH_STREAM_FFT: c_int = 1;
pub const AETH_STREAM_FFT_MUL_IFFT: c_int = 2;
pub const AETH_STREAM_FFT_MUL_IFFT_DEMOD: c_int = 3;
pub const AETH_STREAM_FFT_INTERPOLATE: c_int = 4;
pub const AETH_STREAM_FIR_DECIM: c_int = 5;
pub const AETH_STREAM_MODULATE_AWGN: c_int = 6;
/// aeth_pipe_util: the same plus the seconds each stage (upload, kernel, download) was active -- the per-stage
/// utilisation report of src/pipeline.rs:89-114
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct aeth_pipe_util { pub seconds: f64, pub samples: f64, pub chunks: f64, pub pinned: f64,
                            pub active_upload: f64, pub active_kernel: f64, pub active_download: f64,
                            pub active_copy_in: f64, pub active_copy_out: f64 }

pub const AETH_OK: c_int = 0;
pub const AETH_E_LEN: c_int = -1;
pub const AETH_SCALE_NONE: c_int = 0;
pub const AETH_SCALE_SN: c_int = 1;
pub const AETH_SCALE_N: c_int = 2;
pub const AETH_SCALE_X: c_int = 3;
/// The ONE place where the reference's method names meet an exponent sign:
/// `Cfft::with_len` plans `fwd` with `FFTplanner::new(true)` (rustfft "inverse", +j)
/// and `bwd` with `FFTplanner::new(false)` (src/fft.rs:148,150).
pub const AETH_SIGN_REF_FWD: c_int = 1;
pub const AETH_SIGN_REF_BWD: c_int = -1;
pub const AETH_OFDM_GENERAL: c_int = 1;
pub const AETH_SUMS_GENERAL: c_int = 1;
pub const AETH_OFDM_EQ_ZF: c_int = 0;
pub const AETH_OFDM_EQ_MMSE: c_int = 1;
pub const AETH_OFDM_EQ_MATCHED: c_int = 2;

// cf32 = Complex<f32> is repr(C) {re, im} (src/lib.rs:8-12) == aeth_cf32
extern "C" {
    pub fn aeth_last_error() -> *const c_char;
    pub fn aeth_version() -> c_int;
    pub fn aeth_device_count(count: *mut c_int) -> c_int;
    pub fn aeth_ctx_create(device: c_int, out: *mut *mut aeth_ctx) -> c_int;
    pub fn aeth_ctx_create_on_stream(device: c_int, hip_stream: *mut c_void, out: *mut *mut aeth_ctx) -> c_int;
    pub fn aeth_ctx_stream(ctx: *mut aeth_ctx) -> *mut c_void;
    pub fn aeth_ctx_device(ctx: *const aeth_ctx) -> c_int;
    pub fn aeth_copy_dev(ctx: *mut aeth_ctx, dst: *mut c_void, src: *const c_void, bytes: usize) -> c_int;
    pub fn aeth_event_create(ctx: *mut aeth_ctx, out: *mut *mut aeth_event) -> c_int;
    pub fn aeth_event_destroy(ev: *mut aeth_event) -> c_int;
    pub fn aeth_event_record(ev: *mut aeth_event) -> c_int;
    pub fn aeth_event_sync(ev: *mut aeth_event) -> c_int;
    pub fn aeth_event_elapsed_ms(start: *mut aeth_event, stop: *mut aeth_event, ms: *mut c_float) -> c_int;
    pub fn aeth_ctx_destroy(ctx: *mut aeth_ctx) -> c_int;
    pub fn aeth_ctx_sync(ctx: *mut aeth_ctx) -> c_int;
    pub fn aeth_ctx_set_overlap(ctx: *mut aeth_ctx, enable: c_int) -> c_int;
    pub fn aeth_ctx_overlap(ctx: *const aeth_ctx) -> c_int;
    pub fn aeth_ctx_lane_counts(ctx: *const aeth_ctx, packets: *mut u64, joins: *mut u64) -> c_int;
    pub fn aeth_dev_alloc(ctx: *mut aeth_ctx, bytes: usize, dptr: *mut *mut c_void) -> c_int;
    pub fn aeth_dev_free(ctx: *mut aeth_ctx, dptr: *mut c_void) -> c_int;
    pub fn aeth_upload(ctx: *mut aeth_ctx, dst: *mut c_void, src: *const c_void, bytes: usize) -> c_int;
    pub fn aeth_download(ctx: *mut aeth_ctx, dst: *mut c_void, src: *const c_void, bytes: usize) -> c_int;

    pub fn aeth_vec_scale(ctx: *mut aeth_ctx, s: *mut cf32, n: usize, scale: c_float) -> c_int;
    pub fn aeth_vec_mul(ctx: *mut aeth_ctx, s: *mut cf32, n: usize, o: *const cf32, no: usize) -> c_int;
    pub fn aeth_vec_mul_frames(ctx: *mut aeth_ctx, frames: *mut cf32, frame_len: usize, batch: usize, sig: *const cf32, n_sig: usize) -> c_int;
    pub fn aeth_vec_div(ctx: *mut aeth_ctx, s: *mut cf32, n: usize, o: *const cf32, no: usize) -> c_int;
    pub fn aeth_vec_conj(ctx: *mut aeth_ctx, s: *mut cf32, n: usize) -> c_int;
    pub fn aeth_vec_add(ctx: *mut aeth_ctx, s: *mut cf32, n: usize, o: *const cf32, no: usize) -> c_int;
    pub fn aeth_vec_sub(ctx: *mut aeth_ctx, s: *mut cf32, n: usize, o: *const cf32, no: usize) -> c_int;
    pub fn aeth_vec_mirror(ctx: *mut aeth_ctx, s: *mut cf32, n: usize) -> c_int;
    pub fn aeth_vec_clone(ctx: *mut aeth_ctx, s: *mut cf32, n: usize, o: *const cf32, no: usize) -> c_int;
    pub fn aeth_vec_zero(ctx: *mut aeth_ctx, s: *mut cf32, n: usize) -> c_int;
    pub fn aeth_vec_mirror_frames(ctx: *mut aeth_ctx, s: *mut cf32, frame_len: usize, batch: usize) -> c_int;
    pub fn aeth_vec_stats(ctx: *mut aeth_ctx, x: *const cf32, n: usize, out: *mut aeth_vec_stats_t) -> c_int;
    pub fn aeth_host_vec_stats(ctx: *mut aeth_ctx, x: *const cf32, n: usize, out: *mut aeth_vec_stats_t) -> c_int;
    pub fn aeth_vec_levels(ctx: *mut aeth_ctx, x: *const cf32, n: usize, level_kind: c_int, levels: *mut c_float, n_levels: usize) -> c_int;
    // host-slice flavours: the literal `impl VecOps for [cf32]` semantics, one H2D + D2H per call
    pub fn aeth_host_vec_scale(ctx: *mut aeth_ctx, s: *mut cf32, n: usize, scale: c_float) -> c_int;
    pub fn aeth_host_vec_mul(ctx: *mut aeth_ctx, s: *mut cf32, n: usize, o: *const cf32, no: usize) -> c_int;
    pub fn aeth_host_vec_div(ctx: *mut aeth_ctx, s: *mut cf32, n: usize, o: *const cf32, no: usize) -> c_int;
    pub fn aeth_host_vec_conj(ctx: *mut aeth_ctx, s: *mut cf32, n: usize) -> c_int;
    pub fn aeth_host_vec_add(ctx: *mut aeth_ctx, s: *mut cf32, n: usize, o: *const cf32, no: usize) -> c_int;
    pub fn aeth_host_vec_sub(ctx: *mut aeth_ctx, s: *mut cf32, n: usize, o: *const cf32, no: usize) -> c_int;
    pub fn aeth_host_vec_mirror(ctx: *mut aeth_ctx, s: *mut cf32, n: usize) -> c_int;
    pub fn aeth_host_vec_clone(ctx: *mut aeth_ctx, s: *mut cf32, n: usize, o: *const cf32, no: usize) -> c_int;
    pub fn aeth_host_vec_zero(ctx: *mut aeth_ctx, s: *mut cf32, n: usize) -> c_int;
    pub fn aeth_scale_factor(kind: c_int, n: usize, x: c_float) -> c_float;
    pub fn aeth_scale_apply(ctx: *mut aeth_ctx, kind: c_int, x: c_float, data: *mut cf32, n: usize) -> c_int;

    pub fn aeth_fft_create(ctx: *mut aeth_ctx, len: usize, max_batch: usize, out: *mut *mut aeth_fft) -> c_int;
    pub fn aeth_fft_destroy(plan: *mut aeth_fft) -> c_int;
    pub fn aeth_fft_len(plan: *const aeth_fft) -> usize;
    pub fn aeth_fft_algorithm(plan: *const aeth_fft) -> *const c_char;
    pub fn aeth_fft_route(plan: *const aeth_fft) -> *const c_char;
    pub fn aeth_fft_exec_tmp(plan: *mut aeth_fft, inp: *const cf32, n_in: usize, batch: usize, sign: c_int,
                             scale_kind: c_int, x: c_float, view: *mut *const cf32) -> c_int;
    pub fn aeth_fft_exec(plan: *mut aeth_fft, inp: *const cf32, n_in: usize, out: *mut cf32, batch: usize,
                         sign: c_int, scale_kind: c_int, x: c_float) -> c_int;
    pub fn aeth_fft_exec_mirrored(plan: *mut aeth_fft, inp: *const cf32, n_in: usize, out: *mut cf32, batch: usize, sign: c_int, kind: c_int, x: c_float) -> c_int;
    pub fn aeth_fft_exec_levels(plan: *mut aeth_fft, inp: *const cf32, n_in: usize, batch: usize, sign: c_int, kind: c_int, x: c_float,
                                mirror: c_int, level_kind: c_int, levels: *mut c_float, n_levels: usize) -> c_int;
    pub fn aeth_fft_exec_interpolate(plan: *mut aeth_fft, inp: *const cf32, n_in: usize, batch: usize, sign: c_int, kind: c_int, x: c_float,
                                     dst: *mut cf32, dst_cap: usize, n_between: usize, compat_im: c_int, n_written: *mut usize) -> c_int;
    pub fn aeth_fft_exec_host(plan: *mut aeth_fft, inp: *const cf32, n_in: usize, out: *mut cf32, n_out: usize,
                              sign: c_int, scale_kind: c_int, x: c_float) -> c_int;
    pub fn aeth_fft_exec_tmp_host(plan: *mut aeth_fft, inp: *const cf32, n_in: usize, sign: c_int,
                                  scale_kind: c_int, x: c_float, view: *mut *const cf32) -> c_int;
    pub fn aeth_fft_mul_ifft(plan: *mut aeth_fft, frames: *mut cf32, n_total: usize, batch: usize,
                             sig: *const cf32, n_sig: usize, kf: c_int, xf: c_float, kb: c_int, xb: c_float) -> c_int;
    pub fn aeth_fft_mul_ifft_demod(plan: *mut aeth_fft, frames: *const cf32, n_total: usize, batch: usize, sig: *const cf32, n_sig: usize,
                                   kind_fwd: c_int, x_fwd: c_float, kind_bwd: c_int, x_bwd: c_float, bps: c_int,
                                   table: *const cf32, bits_out: *mut u8, nbits_out: usize, compat: c_int) -> c_int;

    pub fn aeth_fir_create(ctx: *mut aeth_ctx, taps: *const cf32, ntaps: usize, fft_len: usize,
                           out: *mut *mut aeth_fir) -> c_int;
    pub fn aeth_fir_destroy(fir: *mut aeth_fir) -> c_int;
    pub fn aeth_fir_exec(fir: *mut aeth_fir, hist: *const cf32, inp: *const cf32, n: usize, out: *mut cf32) -> c_int;
    pub fn aeth_fir_exec_decim(fir: *mut aeth_fir, hist: *const cf32, inp: *const cf32, n: usize, out: *mut cf32, n_out: usize) -> c_int;
    pub fn aeth_fir_exec_host(fir: *mut aeth_fir, hist: *const cf32, inp: *const cf32, n: usize, out: *mut cf32) -> c_int;
    pub fn aeth_fir_ntaps(fir: *const aeth_fir) -> usize;
    pub fn aeth_fir_fft_len(fir: *const aeth_fir) -> usize;
    pub fn aeth_fir_hop(fir: *const aeth_fir) -> usize;
    // streaming correlator: c[j] = sum_k conj(s[M-1-k]) * x[j-k] (the reference's open item, README.md:95)
    pub fn aeth_corr_create(ctx: *mut aeth_ctx, reference: *const cf32, nref: usize, fft_len: usize,
                            out: *mut *mut aeth_corr) -> c_int;
    pub fn aeth_corr_destroy(corr: *mut aeth_corr) -> c_int;
    pub fn aeth_corr_nref(corr: *const aeth_corr) -> usize;
    pub fn aeth_corr_fft_len(corr: *const aeth_corr) -> usize;
    pub fn aeth_corr_hop(corr: *const aeth_corr) -> usize;
    pub fn aeth_corr_exec(corr: *mut aeth_corr, hist: *const cf32, inp: *const cf32, n: usize, out: *mut cf32) -> c_int;
    pub fn aeth_corr_exec_levels(corr: *mut aeth_corr, hist: *const cf32, inp: *const cf32, n: usize, level_kind: c_int,
                                 levels: *mut c_float, n_levels: usize) -> c_int;
    pub fn aeth_corr_search(corr: *mut aeth_corr, hist: *const cf32, inp: *const cf32, n: usize, peaks: *mut aeth_corr_peak,
                            n_peaks: usize, best: *mut aeth_corr_peak) -> c_int;
    // sequence::generate for linear generators (src/sequence.rs:47-53): init = one word per register on the host
    pub fn aeth_seq_window(reg: *const aeth_seq_reg, init: u64, skip: u64, window: *mut u64) -> c_int;
    pub fn aeth_seq_create(ctx: *mut aeth_ctx, regs: *const aeth_seq_reg, nregs: usize, out: *mut *mut aeth_seq) -> c_int;
    pub fn aeth_seq_destroy(seq: *mut aeth_seq) -> c_int;
    pub fn aeth_seq_nregs(seq: *const aeth_seq) -> usize;
    pub fn aeth_seq_order(seq: *const aeth_seq, reg: usize) -> usize;
    pub fn aeth_seq_chunk(seq: *const aeth_seq) -> usize;
    pub fn aeth_seq_bits(seq: *mut aeth_seq, init: *const u64, skip: u64, bits: *mut u8, n: usize) -> c_int;
    pub fn aeth_seq_scramble(seq: *mut aeth_seq, init: *const u64, skip: u64, inp: *const u8, out: *mut u8, n: usize) -> c_int;
    pub fn aeth_seq_chips(seq: *mut aeth_seq, init: *const u64, skip: u64, zero: cf32, one: cf32, out: *mut cf32, n: usize) -> c_int;
    pub fn aeth_seq_spread(seq: *mut aeth_seq, init: *const u64, skip: u64, sym: *const cf32, nsym: usize, sf: usize,
                           out: *mut cf32, n_out: usize) -> c_int;
    pub fn aeth_host_seq_bits(seq: *mut aeth_seq, init: *const u64, skip: u64, bits: *mut u8, n: usize) -> c_int;
    pub fn aeth_chan_create(ctx: *mut aeth_ctx, proto_host: *const c_float, ntaps: usize, channels: usize, hop: usize, phase: c_int,
                            max_frames: usize, out: *mut *mut aeth_chan) -> c_int;
    pub fn aeth_chan_destroy(chan: *mut aeth_chan) -> c_int;
    pub fn aeth_chan_channels(chan: *const aeth_chan) -> usize;
    pub fn aeth_chan_ntaps(chan: *const aeth_chan) -> usize;
    pub fn aeth_chan_hop(chan: *const aeth_chan) -> usize;
    pub fn aeth_chan_phase(chan: *const aeth_chan) -> c_int;
    pub fn aeth_chan_route(chan: *const aeth_chan) -> *const c_char;
    pub fn aeth_chan_tile(chan: *const aeth_chan) -> usize;
    pub fn aeth_chan_fold(chan: *mut aeth_chan, hist_dev: *const cf32, in_dev: *const cf32, n: usize, first_frame: u64,
                          out_dev: *mut cf32, n_out: usize) -> c_int;
    pub fn aeth_chan_exec(chan: *mut aeth_chan, hist_dev: *const cf32, in_dev: *const cf32, n: usize, first_frame: u64, sign: c_int,
                          scale_kind: c_int, x: c_float, out_dev: *mut cf32, n_out: usize) -> c_int;
    pub fn aeth_chan_exec_levels(chan: *mut aeth_chan, hist_dev: *const cf32, in_dev: *const cf32, n: usize, first_frame: u64,
                                 sign: c_int, scale_kind: c_int, x: c_float, mirror: c_int, level_kind: c_int,
                                 levels_dev: *mut c_float, n_levels: usize) -> c_int;
    pub fn aeth_chan_prototype(kind: c_int, channels: usize, taps_per_channel: usize, out_host: *mut c_float) -> c_int;
    // averaged spectra: per-bin power sums and max hold over frames
    pub fn aeth_vec_frame_sums(ctx: *mut aeth_ctx, frames_dev: *const cf32, n: usize, len: usize, block: usize, chunk: usize,
                               sum_dev: *mut c_double, max_dev: *mut c_double, n_out: usize) -> c_int;
    pub fn aeth_chan_exec_sums(chan: *mut aeth_chan, hist_dev: *const cf32, in_dev: *const cf32, n: usize, first_frame: u64, sign: c_int,
                               scale_kind: c_int, x: c_float, mirror: c_int, block: usize, flags: c_int, sum_dev: *mut c_double,
                               max_dev: *mut c_double, n_out: usize) -> c_int;
    pub fn aeth_chan_sums_chunk(chan: *const aeth_chan) -> usize;
    pub fn aeth_chan_sums_fused(chan: *const aeth_chan) -> c_int;
    pub fn aeth_vec_sum_levels(ctx: *mut aeth_ctx, q_dev: *const c_double, n: usize, count: c_double, level_kind: c_int,
                               levels_dev: *mut c_float) -> c_int;
    pub fn aeth_synth_create(ctx: *mut aeth_ctx, proto_host: *const c_float, ntaps: usize, channels: usize, hop: usize, phase: c_int,
                             max_frames: usize, out: *mut *mut aeth_synth) -> c_int;
    pub fn aeth_synth_destroy(synth: *mut aeth_synth) -> c_int;
    pub fn aeth_synth_channels(synth: *const aeth_synth) -> usize;
    pub fn aeth_synth_ntaps(synth: *const aeth_synth) -> usize;
    pub fn aeth_synth_hop(synth: *const aeth_synth) -> usize;
    pub fn aeth_synth_phase(synth: *const aeth_synth) -> c_int;
    pub fn aeth_synth_route(synth: *const aeth_synth) -> *const c_char;
    pub fn aeth_synth_tile(synth: *const aeth_synth) -> usize;
    pub fn aeth_synth_history(synth: *const aeth_synth) -> usize;
    pub fn aeth_synth_unfold(synth: *mut aeth_synth, hist_dev: *const cf32, frames_dev: *const cf32, n_in: usize, first_frame: u64,
                             out_dev: *mut cf32, n_out: usize) -> c_int;
    pub fn aeth_synth_exec(synth: *mut aeth_synth, hist_dev: *const cf32, spec_dev: *const cf32, n_in: usize, first_frame: u64,
                           sign: c_int, scale_kind: c_int, x: c_float, out_dev: *mut cf32, n_out: usize) -> c_int;
    pub fn aeth_synth_dual_window(w: *const c_float, ntaps: usize, hop: usize, out_host: *mut c_float) -> c_int;
    pub fn aeth_resamp_create(ctx: *mut aeth_ctx, taps_host: *const c_float, ntaps: usize, up: usize, down: usize,
                              out: *mut *mut aeth_resamp) -> c_int;
    pub fn aeth_resamp_destroy(resamp: *mut aeth_resamp) -> c_int;
    pub fn aeth_resamp_up(resamp: *const aeth_resamp) -> usize;
    pub fn aeth_resamp_down(resamp: *const aeth_resamp) -> usize;
    pub fn aeth_resamp_ntaps(resamp: *const aeth_resamp) -> usize;
    pub fn aeth_resamp_history(resamp: *const aeth_resamp) -> usize;
    pub fn aeth_resamp_tile(resamp: *const aeth_resamp) -> usize;
    pub fn aeth_resamp_route(resamp: *const aeth_resamp) -> *const c_char;
    pub fn aeth_resamp_out_count(resamp: *const aeth_resamp, n_in: usize) -> usize;
    pub fn aeth_resamp_exec(resamp: *mut aeth_resamp, hist_dev: *const cf32, in_dev: *const cf32, n: usize, out_dev: *mut cf32,
                            n_out: usize) -> c_int;
    pub fn aeth_resamp_prototype(up: usize, down: usize, taps_per_phase: usize, out_host: *mut c_float) -> c_int;
    pub fn aeth_arb_advance(step: u64, phase: u64, n: usize, count: *mut usize, next_phase: *mut u64) -> c_int;
    pub fn aeth_arb_create(ctx: *mut aeth_ctx, taps_host: *const c_float, ntaps: usize, log2_phases: usize,
                           out: *mut *mut aeth_arb) -> c_int;
    pub fn aeth_arb_destroy(arb: *mut aeth_arb) -> c_int;
    pub fn aeth_arb_phases(arb: *const aeth_arb) -> usize;
    pub fn aeth_arb_ntaps(arb: *const aeth_arb) -> usize;
    pub fn aeth_arb_history(arb: *const aeth_arb) -> usize;
    pub fn aeth_arb_tile(arb: *const aeth_arb, step: u64) -> usize;
    pub fn aeth_arb_route(arb: *const aeth_arb, step: u64) -> *const c_char;
    pub fn aeth_arb_exec(arb: *mut aeth_arb, hist_dev: *const cf32, in_dev: *const cf32, n: usize, step: u64, phase: u64,
                         out_dev: *mut cf32, n_out: usize) -> c_int;
    pub fn aeth_nco_word(cycles: f64) -> u64;
    pub fn aeth_nco_word_at(w: *const aeth_nco_words, n: u64) -> u64;
    pub fn aeth_nco_phasor(word: u64, out_host: *mut cf32) -> c_int;
    pub fn aeth_nco_mix(ctx: *mut aeth_ctx, w: *const aeth_nco_words, n0: u64, in_dev: *const cf32, out_dev: *mut cf32, n: usize) -> c_int;
    pub fn aeth_nco_tone(ctx: *mut aeth_ctx, w: *const aeth_nco_words, n0: u64, amp: c_float, out_dev: *mut cf32, n: usize) -> c_int;
    pub fn aeth_sync_chunk() -> usize;
    pub fn aeth_sync_line(ctx: *mut aeth_ctx, kind: c_int, w: *const aeth_nco_words, n0: u64, x_dev: *const cf32, n: usize, block: usize,
                          rec_dev: *mut aeth_sync_record, total_host: *mut aeth_sync_record) -> c_int;
    pub fn aeth_sync_lag(ctx: *mut aeth_ctx, power: c_int, lag: usize, hist_dev: *const cf32, x_dev: *const cf32, n: usize, block: usize,
                         rec_dev: *mut aeth_sync_record, total_host: *mut aeth_sync_record) -> c_int;
    pub fn aeth_sync_turns(r: *const aeth_sync_record) -> f64;
    pub fn aeth_sync_freq_step(r: *const aeth_sync_record, power: c_int, lag: usize) -> u64;
    pub fn aeth_sync_timing_phase(r: *const aeth_sync_record, sps: f64) -> u64;
    pub fn aeth_mov_history(kind: c_int, window: usize, lag: usize) -> usize;
    pub fn aeth_mov_grid(kind: c_int, window: usize) -> usize;
    pub fn aeth_mov_freq_step(p: *const aeth_mov_peak, lag: usize) -> u64;
    pub fn aeth_mov_exec(ctx: *mut aeth_ctx, kind: c_int, window: usize, lag: usize, hist_dev: *const cf32, x_dev: *const cf32, n: usize,
                         p_dev: *mut cf32, r_dev: *mut f32, m_dev: *mut f32) -> c_int;
    pub fn aeth_mov_search(ctx: *mut aeth_ctx, kind: c_int, window: usize, lag: usize, r_min: f64, threshold: f64, hist_dev: *const cf32,
                           x_dev: *const cf32, n: usize, block: usize, peaks_dev: *mut aeth_mov_peak, best_host: *mut aeth_mov_peak) -> c_int;
    pub fn aeth_ofdm_create(ctx: *mut aeth_ctx, n_fft: usize, cp: usize, bins_host: *const u32, n_bins: usize, max_symbols: usize,
                            flags: c_int, out: *mut *mut aeth_ofdm) -> c_int;
    pub fn aeth_ofdm_destroy(ofdm: *mut aeth_ofdm) -> c_int;
    pub fn aeth_ofdm_len(ofdm: *const aeth_ofdm) -> usize;
    pub fn aeth_ofdm_cp(ofdm: *const aeth_ofdm) -> usize;
    pub fn aeth_ofdm_symbol(ofdm: *const aeth_ofdm) -> usize;
    pub fn aeth_ofdm_carriers(ofdm: *const aeth_ofdm) -> usize;
    pub fn aeth_ofdm_route(ofdm: *const aeth_ofdm) -> *const c_char;
    pub fn aeth_ofdm_span(ofdm: *const aeth_ofdm, n_sym: usize) -> usize;
    pub fn aeth_ofdm_demod(ofdm: *mut aeth_ofdm, in_dev: *const cf32, n_in: usize, n_sym: usize, eq_dev: *const cf32, scale_kind: c_int,
                           x: c_float, out_dev: *mut cf32, n_out: usize) -> c_int;
    pub fn aeth_ofdm_mod(ofdm: *mut aeth_ofdm, car_dev: *const cf32, n_car: usize, n_sym: usize, scale_kind: c_int, x: c_float,
                         out_dev: *mut cf32, n_out: usize) -> c_int;
    pub fn aeth_ofdm_estimate(ofdm: *mut aeth_ofdm, y_dev: *const cf32, x_dev: *const cf32, n_sym: usize, x_sym: usize, nv: c_float,
                              eq_kind: c_int, h_dev: *mut cf32, eq_dev: *mut cf32, csi_dev: *mut c_float) -> c_int;
    pub fn aeth_cc_create(ctx: *mut aeth_ctx, code: *const aeth_cc_code, block: usize, warmup: usize, traceback: usize,
                          out: *mut *mut aeth_cc) -> c_int;
    pub fn aeth_cc_destroy(cc: *mut aeth_cc) -> c_int;
    pub fn aeth_cc_k(cc: *const aeth_cc) -> usize;
    pub fn aeth_cc_n(cc: *const aeth_cc) -> usize;
    pub fn aeth_cc_block(cc: *const aeth_cc) -> usize;
    pub fn aeth_cc_warmup(cc: *const aeth_cc) -> usize;
    pub fn aeth_cc_traceback(cc: *const aeth_cc) -> usize;
    pub fn aeth_cc_history(cc: *const aeth_cc) -> usize;
    pub fn aeth_cc_encode(cc: *mut aeth_cc, hist_bits_dev: *const u8, bits_dev: *const u8, nbits: usize, coded_dev: *mut u8,
                          ncoded: usize) -> c_int;
    pub fn aeth_cc_decode(cc: *mut aeth_cc, hist_soft_dev: *const i8, soft_dev: *const i8, nsoft: usize, bits_dev: *mut u8,
                          nbits: usize) -> c_int;
    pub fn aeth_remap_create(ctx: *mut aeth_ctx, map: *const i32, r_out: usize, r_in: usize, out: *mut *mut aeth_remap) -> c_int;
    pub fn aeth_remap_destroy(rm: *mut aeth_remap) -> c_int;
    pub fn aeth_remap_in_period(rm: *const aeth_remap) -> usize;
    pub fn aeth_remap_out_period(rm: *const aeth_remap) -> usize;
    pub fn aeth_remap_in_count(rm: *const aeth_remap, n_out: usize) -> usize;
    pub fn aeth_remap_route(rm: *const aeth_remap) -> c_int;
    pub fn aeth_remap_tile(rm: *const aeth_remap) -> usize;
    pub fn aeth_remap_exec(rm: *mut aeth_remap, in_dev: *const c_void, n_in: usize, out_dev: *mut c_void, n_out: usize, fill: u8) -> c_int;
    pub fn aeth_remap_puncture(keep: *const u8, p: usize, map: *mut i32, cap: usize, r_out: *mut usize) -> c_int;
    pub fn aeth_remap_invert(map: *const i32, r_out: usize, r_in: usize, inv: *mut i32) -> c_int;
    pub fn aeth_remap_compose(a: *const i32, a_out: usize, a_in: usize, b: *const i32, b_out: usize, b_in: usize, map: *mut i32,
                              cap: usize, r_out: *mut usize, r_in: *mut usize) -> c_int;
    pub fn aeth_remap_rows_cols(rows: usize, cols: usize, map: *mut i32) -> c_int;
    pub fn aeth_remap_bicm16(n_cbps: usize, n_bpsc: usize, map: *mut i32) -> c_int;
    pub fn aeth_crc_create(ctx: *mut aeth_ctx, r: u32, poly: u64, init: u64, xorout: u64, out: *mut *mut aeth_crc) -> c_int;
    pub fn aeth_crc_destroy(crc: *mut aeth_crc) -> c_int;
    pub fn aeth_crc_width(crc: *const aeth_crc) -> u32;
    pub fn aeth_crc_poly(crc: *const aeth_crc) -> u64;
    pub fn aeth_crc_init(crc: *const aeth_crc) -> u64;
    pub fn aeth_crc_xorout(crc: *const aeth_crc) -> u64;
    pub fn aeth_crc_residue(crc: *const aeth_crc) -> u64;
    pub fn aeth_crc_route(crc: *const aeth_crc, l: usize, f: usize) -> c_int;
    pub fn aeth_crc_route_frame_bits(crc: *const aeth_crc) -> usize;
    pub fn aeth_crc_frames_per_workgroup(crc: *const aeth_crc, frame_bytes: usize) -> usize;
    pub fn aeth_crc_named(name: *const c_char, r: *mut u32, poly: *mut u64, init: *mut u64, xorout: *mut u64) -> c_int;
    pub fn aeth_crc_host(r: u32, poly: u64, init: u64, xorout: u64, bits_host: *const u8, l: usize, reg: *mut u64) -> c_int;
    pub fn aeth_crc_exec(crc: *mut aeth_crc, bits_dev: *const u8, l: usize, f: usize, state_in_dev: *const u64,
                         state_out_dev: *mut u64) -> c_int;
    pub fn aeth_crc_attach(crc: *mut aeth_crc, in_dev: *const u8, l: usize, f: usize, out_dev: *mut u8) -> c_int;
    pub fn aeth_crc_check(crc: *mut aeth_crc, in_dev: *const u8, l: usize, f: usize, mask: u64, diff_dev: *mut u64,
                          payload_dev: *mut u8, summary_dev: *mut aeth_crc_summary) -> c_int;
    pub fn aeth_bits_pack(ctx: *mut aeth_ctx, bits_dev: *const u8, nbits: usize, order: c_int, bytes_dev: *mut u8, nbytes: usize) -> c_int;
    pub fn aeth_bits_unpack(ctx: *mut aeth_ctx, bytes_dev: *const u8, nbytes: usize, order: c_int, bits_dev: *mut u8, nbits: usize) -> c_int;
    pub fn aeth_ldpc_generator(code: *const aeth_ldpc_code, p_out: *mut u64, nwords: usize) -> c_int;
    pub fn aeth_ldpc_create(ctx: *mut aeth_ctx, code: *const aeth_ldpc_code, out: *mut *mut aeth_ldpc) -> c_int;
    pub fn aeth_ldpc_destroy(ldpc: *mut aeth_ldpc) -> c_int;
    pub fn aeth_ldpc_n(ldpc: *const aeth_ldpc) -> usize;
    pub fn aeth_ldpc_k(ldpc: *const aeth_ldpc) -> usize;
    pub fn aeth_ldpc_rows(ldpc: *const aeth_ldpc) -> u32;
    pub fn aeth_ldpc_cols(ldpc: *const aeth_ldpc) -> u32;
    pub fn aeth_ldpc_z(ldpc: *const aeth_ldpc) -> u32;
    pub fn aeth_ldpc_edges(ldpc: *const aeth_ldpc) -> usize;
    pub fn aeth_ldpc_lds_bytes(ldpc: *const aeth_ldpc) -> usize;
    pub fn aeth_ldpc_group(ldpc: *const aeth_ldpc) -> u32;
    pub fn aeth_ldpc_encode(ldpc: *mut aeth_ldpc, bits_dev: *const u8, nbits: usize, coded_dev: *mut u8, ncoded: usize) -> c_int;
    pub fn aeth_ldpc_decode(ldpc: *mut aeth_ldpc, soft_dev: *const i8, nsoft: usize, max_iter: u32, flags: u32, bits_dev: *mut u8,
                            nbits: usize, rec_dev: *mut aeth_ldpc_record) -> c_int;
    pub fn aeth_rs_named(name: *const c_char, code: *mut aeth_rs_code) -> c_int;
    pub fn aeth_rs_generator(code: *const aeth_rs_code, g_out: *mut u8, ng: usize) -> c_int;
    pub fn aeth_rs_host_encode(code: *const aeth_rs_code, data_host: *const u8, ndata: usize, depth: u32, coded_host: *mut u8, ncoded: usize) -> c_int;
    pub fn aeth_rs_host_decode(code: *const aeth_rs_code, in_host: *const u8, nin: usize, era_host: *const u8, depth: u32, flags: u32,
                               out_host: *mut u8, nout: usize, rec_host: *mut aeth_rs_record, summary_host: *mut aeth_rs_summary) -> c_int;
    pub fn aeth_rs_create(ctx: *mut aeth_ctx, code: *const aeth_rs_code, out: *mut *mut aeth_rs) -> c_int;
    pub fn aeth_rs_destroy(rs: *mut aeth_rs) -> c_int;
    pub fn aeth_rs_n(rs: *const aeth_rs) -> usize;
    pub fn aeth_rs_k(rs: *const aeth_rs) -> usize;
    pub fn aeth_rs_nroots(rs: *const aeth_rs) -> u32;
    pub fn aeth_rs_m(rs: *const aeth_rs) -> u32;
    pub fn aeth_rs_group(rs: *const aeth_rs) -> u32;
    pub fn aeth_rs_lds_bytes(rs: *const aeth_rs, depth: u32) -> usize;
    pub fn aeth_rs_encode(rs: *mut aeth_rs, data_dev: *const u8, ndata: usize, depth: u32, coded_dev: *mut u8, ncoded: usize) -> c_int;
    pub fn aeth_rs_decode(rs: *mut aeth_rs, in_dev: *const u8, nin: usize, era_dev: *const u8, depth: u32, flags: u32, out_dev: *mut u8,
                          nout: usize, rec_dev: *mut aeth_rs_record, summary_dev: *mut aeth_rs_summary) -> c_int;
    pub fn aeth_polar_rank(n: u32, order_out: *mut u32, count: usize) -> c_int;
    pub fn aeth_polar_mask(n: u32, k: u32, mask_out: *mut u8, count: usize) -> c_int;
    pub fn aeth_polar_create(ctx: *mut aeth_ctx, n: u32, mask: *const u8, out: *mut *mut aeth_polar) -> c_int;
    pub fn aeth_polar_destroy(polar: *mut aeth_polar) -> c_int;
    pub fn aeth_polar_n(polar: *const aeth_polar) -> usize;
    pub fn aeth_polar_k(polar: *const aeth_polar) -> usize;
    pub fn aeth_polar_lanes(polar: *const aeth_polar) -> u32;
    pub fn aeth_polar_group(polar: *const aeth_polar) -> u32;
    pub fn aeth_polar_lds_bytes(polar: *const aeth_polar) -> usize;
    pub fn aeth_polar_encode(polar: *mut aeth_polar, bits_dev: *const u8, nbits: usize, coded_dev: *mut u8, ncoded: usize) -> c_int;
    pub fn aeth_polar_decode(polar: *mut aeth_polar, soft_dev: *const i8, nsoft: usize, flip_dev: *const u32, flags: u32, bits_dev: *mut u8,
                             nbits: usize, rec_dev: *mut aeth_polar_record) -> c_int;
    pub fn aeth_polar_list_create(ctx: *mut aeth_ctx, n: u32, mask: *const u8, l: u32, out: *mut *mut aeth_polar_list) -> c_int;
    pub fn aeth_polar_list_destroy(list: *mut aeth_polar_list) -> c_int;
    pub fn aeth_polar_list_n(list: *const aeth_polar_list) -> usize;
    pub fn aeth_polar_list_k(list: *const aeth_polar_list) -> usize;
    pub fn aeth_polar_list_paths(list: *const aeth_polar_list) -> u32;
    pub fn aeth_polar_list_lanes(list: *const aeth_polar_list) -> u32;
    pub fn aeth_polar_list_group(list: *const aeth_polar_list) -> u32;
    pub fn aeth_polar_list_lds_bytes(list: *const aeth_polar_list) -> usize;
    pub fn aeth_polar_list_decode(list: *mut aeth_polar_list, soft_dev: *const i8, nsoft: usize, flags: u32, bits_dev: *mut u8, nbits: usize,
                                  rec_dev: *mut aeth_polar_list_record) -> c_int;
    pub fn aeth_polar_list_pick(ctx: *mut aeth_ctx, rows_dev: *const u8, row_bytes: usize, f: usize, l: u32, diff_dev: *const u64,
                                out_dev: *mut u8, which_dev: *mut u32) -> c_int;
    pub fn aeth_turbo_named(name: *const c_char, code_out: *mut aeth_turbo_code) -> c_int;
    pub fn aeth_turbo_qpp(k: u32, f1: u32, f2: u32, pi_out: *mut u32, count: usize) -> c_int;
    pub fn aeth_turbo_create(ctx: *mut aeth_ctx, code: *const aeth_turbo_code, k: u32, pi_host: *const u32, window: u32, warmup: u32,
                             out: *mut *mut aeth_turbo) -> c_int;
    pub fn aeth_turbo_destroy(turbo: *mut aeth_turbo) -> c_int;
    pub fn aeth_turbo_k(turbo: *const aeth_turbo) -> usize;
    pub fn aeth_turbo_n(turbo: *const aeth_turbo) -> usize;
    pub fn aeth_turbo_states(turbo: *const aeth_turbo) -> u32;
    pub fn aeth_turbo_window(turbo: *const aeth_turbo) -> u32;
    pub fn aeth_turbo_warmup(turbo: *const aeth_turbo) -> u32;
    pub fn aeth_turbo_windows(turbo: *const aeth_turbo) -> u32;
    pub fn aeth_turbo_group(turbo: *const aeth_turbo) -> u32;
    pub fn aeth_turbo_lds_bytes(turbo: *const aeth_turbo) -> usize;
    pub fn aeth_turbo_encode(turbo: *mut aeth_turbo, bits_dev: *const u8, nbits: usize, coded_dev: *mut u8, ncoded: usize) -> c_int;
    pub fn aeth_turbo_decode(turbo: *mut aeth_turbo, soft_dev: *const i8, nsoft: usize, max_iter: u32, flags: u32, bits_dev: *mut u8,
                             nbits: usize, rec_dev: *mut aeth_turbo_record) -> c_int;
    pub fn aeth_pool_create(ctx: *mut aeth_ctx, elem_bytes: usize, initial_len: usize, flags: c_int, out: *mut *mut aeth_pool) -> c_int;
    pub fn aeth_pool_destroy(pool: *mut aeth_pool) -> c_int;
    pub fn aeth_pool_take(pool: *mut aeth_pool, buf: *mut *mut c_void) -> c_int;
    pub fn aeth_pool_take_or_make(pool: *mut aeth_pool, buf: *mut *mut c_void) -> c_int;
    pub fn aeth_pool_give_back(pool: *mut aeth_pool, buf: *mut c_void) -> c_int;
    pub fn aeth_pool_len(pool: *mut aeth_pool) -> usize;
    pub fn aeth_pool_cap(pool: *mut aeth_pool) -> usize;
    pub fn aeth_pool_elem_bytes(pool: *const aeth_pool) -> usize;
    pub fn aeth_host_register(ctx: *mut aeth_ctx, ptr: *mut c_void, bytes: usize) -> c_int;
    pub fn aeth_host_unregister(ctx: *mut aeth_ctx, ptr: *mut c_void) -> c_int;
    pub fn aeth_host_is_pinned(ptr: *const c_void, bytes: usize) -> c_int;
    pub fn aeth_vec_fft(ctx: *mut aeth_ctx, x: *mut cf32, n: usize, sign: c_int, kind: c_int, x_scale: c_float) -> c_int;
    pub fn aeth_host_vec_fft(ctx: *mut aeth_ctx, x: *mut cf32, n: usize, sign: c_int, kind: c_int, x_scale: c_float) -> c_int;
    pub fn aeth_vec_chain(ctx: *mut aeth_ctx, self_: *mut cf32, n: usize, steps: *const aeth_vec_step, n_steps: usize) -> c_int;
    pub fn aeth_stream_out_count(ctx: *mut aeth_ctx, op: *const aeth_stream_op, n_in: usize) -> usize;
    pub fn aeth_stream_host(ctx: *mut aeth_ctx, op: *const aeth_stream_op, inp: *const c_void, n_in: usize, out: *mut c_void,
                            n_out: usize, chunk: usize, stats: *mut aeth_pipe_stats) -> c_int;
    pub fn aeth_stream_host_util(ctx: *mut aeth_ctx, op: *const aeth_stream_op, inp: *const c_void, n_in: usize, out: *mut c_void,
                                 n_out: usize, chunk: usize, util: *mut aeth_pipe_util) -> c_int;
    pub fn aeth_stream_chain_out_count(ctx: *mut aeth_ctx, ops: *const aeth_stream_op, n_ops: usize, n_in: usize) -> usize;
    pub fn aeth_stream_host_chain(ctx: *mut aeth_ctx, ops: *const aeth_stream_op, n_ops: usize, inp: *const c_void, n_in: usize,
                                  out: *mut c_void, n_out: usize, chunk: usize, stats: *mut aeth_pipe_stats, util: *mut aeth_pipe_util) -> c_int;
    pub fn aeth_ctx_trim(ctx: *mut aeth_ctx) -> c_int;
    pub fn aeth_test_fail_staging_after(n: c_int);
    pub fn aeth_fir_stream_host(fir: *mut aeth_fir, inp: *const cf32, n: usize, out: *mut cf32, chunk: usize,
                                stats: *mut aeth_pipe_stats) -> c_int;
    pub fn aeth_fir_stream_host_util(fir: *mut aeth_fir, inp: *const cf32, n: usize, out: *mut cf32, chunk: usize,
                                     util: *mut aeth_pipe_util) -> c_int;
    pub fn aeth_stream_file(ctx: *mut aeth_ctx, op: *const aeth_stream_op, in_path: *const c_char, out_path: *const c_char, chunk: usize,
                            stats: *mut aeth_pipe_stats) -> c_int;
    pub fn aeth_fir_stream_file(fir: *mut aeth_fir, in_path: *const c_char, out_path: *const c_char, chunk: usize,
                                stats: *mut aeth_pipe_stats) -> c_int;
    pub fn aeth_file_count_structs(path: *const c_char, elem_size: usize, count: *mut usize) -> c_int;
    pub fn aeth_file_read(path: *const c_char, first_elem: usize, dst: *mut c_void, n: usize, elem_size: usize) -> c_int;
    pub fn aeth_file_write(path: *const c_char, src: *const c_void, n: usize, elem_size: usize, append: c_int) -> c_int;

    pub fn aeth_interpolate(ctx: *mut aeth_ctx, src: *const cf32, n_src: usize, dst: *mut cf32, cap: usize,
                            n_between: usize, compat_im: c_int, n_written: *mut usize) -> c_int;
    pub fn aeth_interpolate_frames(ctx: *mut aeth_ctx, src: *const cf32, frame_len: usize, batch: usize, dst: *mut cf32,
                                   cap: usize, n_between: usize, compat_im: c_int, n_written: *mut usize) -> c_int;
    pub fn aeth_downsample(ctx: *mut aeth_ctx, src: *const c_void, n_src: usize, dst: *mut c_void, n_dst: usize,
                           elem_size: usize) -> c_int;

    pub fn aeth_host_interpolate(ctx: *mut aeth_ctx, src: *const cf32, n_src: usize, dst: *mut cf32, cap: usize,
                                 n_between: usize, compat_im: c_int, n_written: *mut usize) -> c_int;
    pub fn aeth_modulate(ctx: *mut aeth_ctx, bits: *const u8, nbits: usize, bits_per_symbol: c_int,
                         table: *const cf32, out: *mut cf32, n_out: usize) -> c_int;
    pub fn aeth_modulate_awgn(ctx: *mut aeth_ctx, bits: *const u8, nbits: usize, bps: c_int, table: *const cf32, out: *mut cf32,
                              n_out: usize, power: c_float, seed: u64, offset: u64) -> c_int;
    pub fn aeth_demod_naive(ctx: *mut aeth_ctx, sym: *const cf32, nsym: usize, bits_per_symbol: c_int,
                            table: *const cf32, bits_out: *mut u8, nbits_out: usize, compat: c_int) -> c_int;
    pub fn aeth_demod_soft(ctx: *mut aeth_ctx, sym: *const cf32, nsym: usize, bits_per_symbol: c_int, table: *const cf32,
                           scale: c_float, out: *mut i8, nout: usize) -> c_int;
    pub fn aeth_awgn_apply(ctx: *mut aeth_ctx, signal: *mut cf32, n: usize, power: c_float, seed: u64, offset: u64) -> c_int;
    pub fn aeth_awgn_fill(ctx: *mut aeth_ctx, target: *mut cf32, n: usize, power: c_float, seed: u64, offset: u64) -> c_int;
    pub fn aeth_rng_philox4x32_10(ctx: *mut aeth_ctx, ctr_key: *const u32, n: usize, out: *mut u32) -> c_int;
    pub fn aeth_rng_philox4x32(ctx: *mut aeth_ctx, ctr_key: *const u32, n: usize, rounds: c_int, out: *mut u32) -> c_int;
    pub fn aeth_rng_normal_pairs(ctx: *mut aeth_ctx, ab: *const u32, n: usize, out: *mut aeth_cf32) -> c_int;
    pub fn aeth_host_downsample(ctx: *mut aeth_ctx, src: *const c_void, n_src: usize, dst: *mut c_void,
                                n_dst: usize, elem_size: usize) -> c_int;
    pub fn aeth_downsample_release(ctx: *mut aeth_ctx, src: *const c_void, n_src: usize, dst: *mut c_void, n_dst: usize,
                                   elem_size: usize, step_by: c_int) -> c_int;
    pub fn aeth_host_downsample_release(ctx: *mut aeth_ctx, src: *const c_void, n_src: usize, dst: *mut c_void,
                                        n_dst: usize, elem_size: usize, step_by: c_int) -> c_int;
}

/// Error convention: the reference panics (assert_eq!); the C ABI returns a code and a
/// thread-local message that carries the reference's panic text verbatim.
pub fn check(rc: c_int) {
    if rc != AETH_OK {
        let msg = unsafe { std::ffi::CStr::from_ptr(aeth_last_error()) }.to_string_lossy().into_owned();
        panic!("{}", msg);
    }
}
