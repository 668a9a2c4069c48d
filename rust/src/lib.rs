//! aether_hip -- MI355X backend behind aether_primitives' own traits.
//!
//! * `HipFft` implements `aether_primitives::fft::Fft` (src/fft.rs:48-77), so it plugs
//!   into `vec_rfft` / `vec_rifft` (generic over `impl Fft`, src/vecops.rs:83,88) exactly
//!   where `Cfft` does: `data.vec_rfft(&mut hip_fft, Scale::SN)`.
//! * `DeviceVec` keeps samples in HBM and offers the `VecOps` method set with the same
//!   names and chaining (`&mut self -> &mut Self`), one kernel launch per call.
//! * `sampling::{interpolate, downsample}` have the reference's signatures.
//!
//! Not compiled in this pipeline (no Rust toolchain): see Cargo.toml.
pub mod ffi;

use aether_primitives::cf32;
use aether_primitives::fft::{Fft, Scale};
use ffi::*;
use std::marker::PhantomData;
use std::os::raw::{c_int, c_void};
use std::ptr;

fn scale_args(s: Scale) -> (i32, f32) {
    match s {
        Scale::None => (AETH_SCALE_NONE, 0.0),
        Scale::SN => (AETH_SCALE_SN, 0.0),
        Scale::N => (AETH_SCALE_N, 0.0),
        Scale::X(x) => (AETH_SCALE_X, x),
    }
}

/// One device + one HIP stream.  `Send` (may move between pipeline threads like a
/// pooled `Cfft`, src/pool.rs:69-71), not `Sync` (every method takes `&mut self`).
///
/// Device objects (`DeviceVec`, plans) borrow the context SHARED, so several can live at once; the
/// context itself is `!Sync` (raw pointer), which keeps all of them on one thread at a time as the
/// C side requires.
pub struct Context { h: *mut aeth_ctx }
unsafe impl Send for Context {}
impl Context {
    pub fn new(device: i32) -> Context {
        let mut h = ptr::null_mut();
        check(unsafe { aeth_ctx_create(device, &mut h) });
        Context { h }
    }
    pub fn sync(&self) { check(unsafe { aeth_ctx_sync(self.h) }) }
    /// Consecutive independent `Fir::filter` launches alternate between two HIP queues.
    pub fn set_overlap(&self, enable: bool) { check(unsafe { aeth_ctx_set_overlap(self.h, enable as c_int) }) }
}
impl Drop for Context { fn drop(&mut self) { unsafe { aeth_ctx_destroy(self.h); } } }

/// Replaces `Cfft` (src/fft.rs:134-235).  Borrows its `Context` for `'c`: the plan's Drop (and every call)
/// goes through the context's stream, so the context must outlive it -- the borrow checker enforces what the
/// C side requires.  Not `Send`: the plan shares the context's one stream and staging buffers with every other
/// object of that context, so it stays on the context's thread (the reference's `Cfft` is `Send` because it owns
/// everything it touches; a whole `Context` with its plans can still move as one unit).
pub struct HipFft<'c> { h: *mut aeth_fft, _ctx: PhantomData<&'c Context> }
impl<'c> HipFft<'c> {
    /// `Cfft::with_len` (src/fft.rs:147)
    pub fn with_len(ctx: &'c Context, len: usize) -> HipFft<'c> {
        let mut h = ptr::null_mut();
        check(unsafe { aeth_fft_create(ctx.h, len, 1, &mut h) });
        HipFft { h, _ctx: PhantomData }
    }
    fn host(&mut self, input: *const cf32, n_in: usize, output: *mut cf32, n_out: usize, sign: i32, s: Scale) {
        let (k, x) = scale_args(s);
        check(unsafe { aeth_fft_exec_host(self.h, input, n_in, output, n_out, sign, k, x) });
    }
    /// per frame: `vec_rfft(self, s)`, `vec_mirror()` if asked for, then the level of every bin: `waterfall` / `spectrum`
    /// of src/util/plot.rs:46-68, :109-130 in one call; `frames` stays as it was
    pub fn levels<'v>(&mut self, frames: &DeviceVec<'v>, s: Scale, mirror: bool, kind: Level) -> DeviceF32<'v> {
        let (k, x) = scale_args(s);
        let batch = if self.len() > 0 { frames.n / self.len() } else { 0 };
        let out = DeviceF32::new(frames.ctx, frames.n);
        check(unsafe { aeth_fft_exec_levels(self.h, frames.p, frames.n, batch, AETH_SIGN_REF_FWD, k, x, mirror as i32, kind as i32, out.p, out.n) });
        out
    }
    fn tmp(&mut self, input: &[cf32], sign: i32, s: Scale) -> &[cf32] {
        let (k, x) = scale_args(s);
        let mut view: *const cf32 = ptr::null();
        check(unsafe { aeth_fft_exec_tmp_host(self.h, input.as_ptr(), input.len(), sign, k, x, &mut view) });
        // borrow tied to &mut self: valid until the next call on this plan (src/fft.rs:68,73)
        unsafe { std::slice::from_raw_parts(view, self.len()) }
    }
}
impl<'c> Drop for HipFft<'c> { fn drop(&mut self) { unsafe { aeth_fft_destroy(self.h); } } }

impl<'c> Fft for HipFft<'c> {
    fn fwd(&mut self, input: &[cf32], output: &mut [cf32], s: Scale) {
        self.host(input.as_ptr(), input.len(), output.as_mut_ptr(), output.len(), AETH_SIGN_REF_FWD, s)
    }
    fn bwd(&mut self, input: &[cf32], output: &mut [cf32], s: Scale) {
        self.host(input.as_ptr(), input.len(), output.as_mut_ptr(), output.len(), AETH_SIGN_REF_BWD, s)
    }
    fn ifwd(&mut self, input: &mut [cf32], s: Scale) {
        let (p, n) = (input.as_mut_ptr(), input.len());
        self.host(p as *const cf32, n, p, n, AETH_SIGN_REF_FWD, s)     // in == out: in place on the C side
    }
    fn ibwd(&mut self, input: &mut [cf32], s: Scale) {
        let (p, n) = (input.as_mut_ptr(), input.len());
        self.host(p as *const cf32, n, p, n, AETH_SIGN_REF_BWD, s)
    }
    fn tfwd(&mut self, input: &[cf32], s: Scale) -> &[cf32] { self.tmp(input, AETH_SIGN_REF_FWD, s) }
    fn tbwd(&mut self, input: &[cf32], s: Scale) -> &[cf32] { self.tmp(input, AETH_SIGN_REF_BWD, s) }
    fn len(&self) -> usize { unsafe { aeth_fft_len(self.h) } }
}

/// level kinds (AETH_LEVEL_*): `norm()`, the reference's `DB::from(norm).db()` (10 * log10 of the amplitude: its
/// quirk), the power in dB
#[derive(Clone, Copy)]
pub enum Level { Norm = 0, Db = 1, PowerDb = 2 }
/// the reference's open item "VecStats" (README.md:90-91)
pub type VecStats = aeth_vec_stats_t;

/// Device-resident `[f32]`: the levels of a vector or of a batch of spectra.
pub struct DeviceF32<'c> { ctx: &'c Context, p: *mut f32, n: usize }
impl<'c> DeviceF32<'c> {
    pub fn new(ctx: &'c Context, n: usize) -> DeviceF32<'c> {
        let mut p: *mut c_void = ptr::null_mut();
        check(unsafe { aeth_dev_alloc(ctx.h, n.max(1) * 4, &mut p) });
        DeviceF32 { ctx, p: p as *mut f32, n }
    }
    pub fn len(&self) -> usize { self.n }
    pub fn to_vec(&self) -> Vec<f32> {
        let mut v = vec![0f32; self.n];
        check(unsafe { aeth_download(self.ctx.h, v.as_mut_ptr() as *mut c_void, self.p as *const c_void, self.n * 4) });
        v
    }
}
impl<'c> Drop for DeviceF32<'c> { fn drop(&mut self) { unsafe { aeth_dev_free(self.ctx.h, self.p as *mut c_void); } } }

/// Device-resident `[f64]`: the sum and max planes of averaged spectra (aeth_vec_frame_sums, aeth_chan_exec_sums).
pub struct DeviceF64<'c> { ctx: &'c Context, p: *mut f64, n: usize }
impl<'c> DeviceF64<'c> {
    pub fn new(ctx: &'c Context, n: usize) -> DeviceF64<'c> {
        let mut p: *mut c_void = ptr::null_mut();
        check(unsafe { aeth_dev_alloc(ctx.h, n.max(1) * 8, &mut p) });
        DeviceF64 { ctx, p: p as *mut f64, n }
    }
    pub fn len(&self) -> usize { self.n }
    pub fn to_vec(&self) -> Vec<f64> {
        let mut v = vec![0f64; self.n];
        check(unsafe { aeth_download(self.ctx.h, v.as_mut_ptr() as *mut c_void, self.p as *const c_void, self.n * 8) });
        v
    }
    /// what a plot draws of the plane: the level of q / count (the frames of a row for a sum plane, 1 for a max plane)
    pub fn sum_levels(&self, count: f64, kind: Level) -> DeviceF32<'c> {
        let out = DeviceF32::new(self.ctx, self.n);
        check(unsafe { aeth_vec_sum_levels(self.ctx.h, self.p, self.n, count, kind as i32, out.p) });
        out
    }
}
impl<'c> Drop for DeviceF64<'c> { fn drop(&mut self) { unsafe { aeth_dev_free(self.ctx.h, self.p as *mut c_void); } } }

/// Device-resident `[cf32]` with the `VecOps` method set (src/vecops.rs:39-89).
pub struct DeviceVec<'c> { ctx: &'c Context, p: *mut cf32, n: usize }
impl<'c> DeviceVec<'c> {
    pub fn from_slice(ctx: &'c Context, host: &[cf32]) -> DeviceVec<'c> {
        let mut p: *mut c_void = ptr::null_mut();
        check(unsafe { aeth_dev_alloc(ctx.h, host.len() * 8, &mut p) });
        check(unsafe { aeth_upload(ctx.h, p, host.as_ptr() as *const c_void, host.len() * 8) });
        DeviceVec { ctx, p: p as *mut cf32, n: host.len() }
    }
    pub fn to_vec(&mut self) -> Vec<cf32> {
        let mut v = vec![cf32::default(); self.n];
        check(unsafe { aeth_download(self.ctx.h, v.as_mut_ptr() as *mut c_void, self.p as *const c_void, self.n * 8) });
        v
    }
    pub fn len(&self) -> usize { self.n }
    /// one read-only pass: min / max by norm with their (lowest) indices, mean, power; waits for the 64-byte record
    pub fn stats(&self) -> VecStats {
        let mut st = VecStats::default();
        check(unsafe { aeth_vec_stats(self.ctx.h, self.p, self.n, &mut st) });
        st
    }
    /// the level of every sample (src/util/plot.rs:65,127); `self` is not modified
    pub fn levels(&self, kind: Level) -> DeviceF32<'c> {
        let out = DeviceF32::new(self.ctx, self.n);
        check(unsafe { aeth_vec_levels(self.ctx.h, self.p, self.n, kind as i32, out.p, out.n) });
        out
    }
    /// `self` as frames of `len` samples: per-column sums and maxima of q over rows of `block` frames (0: one row), added
    /// in chunks of `chunk` frames (aeth_vec_frame_sums); a plane that is None is not computed
    pub fn frame_sums(&self, len: usize, block: usize, chunk: usize, sum: Option<&mut DeviceF64>, max: Option<&mut DeviceF64>) {
        let n_out = sum.as_ref().map(|v| v.n).or(max.as_ref().map(|v| v.n)).unwrap_or(0);
        check(unsafe { aeth_vec_frame_sums(self.ctx.h, self.p, self.n, len, block, chunk, sum.map_or(ptr::null_mut(), |v| v.p),
                                           max.map_or(ptr::null_mut(), |v| v.p), n_out) });
    }
    pub fn vec_scale(&mut self, s: f32) -> &mut Self { check(unsafe { aeth_vec_scale(self.ctx.h, self.p, self.n, s) }); self }
    pub fn vec_mul(&mut self, o: &DeviceVec) -> &mut Self { check(unsafe { aeth_vec_mul(self.ctx.h, self.p, self.n, o.p, o.n) }); self }
    pub fn vec_div(&mut self, o: &DeviceVec) -> &mut Self { check(unsafe { aeth_vec_div(self.ctx.h, self.p, self.n, o.p, o.n) }); self }
    pub fn vec_conj(&mut self) -> &mut Self { check(unsafe { aeth_vec_conj(self.ctx.h, self.p, self.n) }); self }
    pub fn vec_mirror(&mut self) -> &mut Self { check(unsafe { aeth_vec_mirror(self.ctx.h, self.p, self.n) }); self }
    pub fn vec_clone(&mut self, o: &DeviceVec) -> &mut Self { check(unsafe { aeth_vec_clone(self.ctx.h, self.p, self.n, o.p, o.n) }); self }
    pub fn vec_zero(&mut self) -> &mut Self { check(unsafe { aeth_vec_zero(self.ctx.h, self.p, self.n) }); self }
    pub fn vec_add(&mut self, o: &DeviceVec) -> &mut Self { check(unsafe { aeth_vec_add(self.ctx.h, self.p, self.n, o.p, o.n) }); self }
    pub fn vec_sub(&mut self, o: &DeviceVec) -> &mut Self { check(unsafe { aeth_vec_sub(self.ctx.h, self.p, self.n, o.p, o.n) }); self }
    /// closures cannot cross the FFI: D2H, apply in order, H2D (slow by design)
    pub fn vec_mutate(&mut self, f: impl FnMut(&mut cf32)) -> &mut Self {
        let mut v = self.to_vec();
        v.iter_mut().for_each(f);
        check(unsafe { aeth_upload(self.ctx.h, self.p as *mut c_void, v.as_ptr() as *const c_void, self.n * 8) });
        self
    }
    /// the chained element-wise methods as ONE pass over memory (`aeth_vec_chain`; bit-identical to the separate calls):
    /// `v.fused().vec_add(&a).vec_mul(&b).vec_conj().run();` -- the operands are borrowed until `run`, so the borrow
    /// checker rules out an operand that aliases `self` exactly as it does for the separate calls
    pub fn fused<'v>(&'v mut self) -> Chain<'v, 'c> { Chain { v: self, steps: Vec::new() } }
    /// device frames through a plan: `len()` may be a multiple of `fft.len()` (a batch)
    pub fn vec_rfft(&mut self, fft: &mut HipFft, s: Scale) -> &mut Self { self.exec(fft, AETH_SIGN_REF_FWD, s) }
    pub fn vec_rifft(&mut self, fft: &mut HipFft, s: Scale) -> &mut Self { self.exec(fft, AETH_SIGN_REF_BWD, s) }
    fn exec(&mut self, fft: &mut HipFft, sign: i32, s: Scale) -> &mut Self {
        let (k, x) = scale_args(s);
        let batch = if fft.len() > 0 { self.n / fft.len() } else { 0 };
        check(unsafe { aeth_fft_exec(fft.h, self.p, self.n, self.p, batch, sign, k, x) });
        self
    }
}
impl<'c> Drop for DeviceVec<'c> { fn drop(&mut self) { unsafe { aeth_dev_free(self.ctx.h, self.p as *mut c_void); } } }

/// links recorded by `DeviceVec::fused()`
pub struct Chain<'v, 'c> { v: &'v mut DeviceVec<'c>, steps: Vec<aeth_vec_step> }
impl<'v, 'c> Chain<'v, 'c> {
    fn un(mut self, op: c_int, scale: f32) -> Self { self.steps.push(aeth_vec_step { op, other_dev: ptr::null(), n_other: 0, scale }); self }
    fn bin(mut self, op: c_int, o: &'v DeviceVec) -> Self { self.steps.push(aeth_vec_step { op, other_dev: o.p, n_other: o.n, scale: 0.0 }); self }
    pub fn vec_scale(self, s: f32) -> Self { self.un(AETH_VEC_SCALE, s) }
    pub fn vec_conj(self) -> Self { self.un(AETH_VEC_CONJ, 0.0) }
    pub fn vec_zero(self) -> Self { self.un(AETH_VEC_ZERO, 0.0) }
    pub fn vec_mul(self, o: &'v DeviceVec) -> Self { self.bin(AETH_VEC_MUL, o) }
    pub fn vec_div(self, o: &'v DeviceVec) -> Self { self.bin(AETH_VEC_DIV, o) }
    pub fn vec_add(self, o: &'v DeviceVec) -> Self { self.bin(AETH_VEC_ADD, o) }
    pub fn vec_sub(self, o: &'v DeviceVec) -> Self { self.bin(AETH_VEC_SUB, o) }
    pub fn vec_clone(self, o: &'v DeviceVec) -> Self { self.bin(AETH_VEC_CLONE, o) }
    pub fn run(self) { check(unsafe { aeth_vec_chain(self.v.ctx.h, self.v.p, self.v.n, self.steps.as_ptr(), self.steps.len()) }); }
}

pub mod sampling {
    use super::*;
    /// `sampling::interpolate` (src/sampling.rs:7-24): APPENDS to `dst`.
    pub fn interpolate(ctx: &Context, src: &[cf32], dst: &mut Vec<cf32>, n_between: usize) {
        assert!(!src.is_empty());                              // the reference unwrap()s src.last()
        let add = src.len() + (src.len() - 1) * n_between;
        dst.reserve(add);
        let mut written = 0usize;
        let tail = unsafe { dst.as_mut_ptr().add(dst.len()) };
        check(unsafe { aeth_host_interpolate(ctx.h, src.as_ptr(), src.len(), tail, add, n_between, 1, &mut written) });
        unsafe { dst.set_len(dst.len() + written) };
    }
    /// `sampling::downsample<T: Copy>` (src/sampling.rs:28-42)
    /// The reference's divisibility check is a `debug_assert_eq!` (:32-36): a debug build of this crate binds the
    /// checked entry point, a release build the one that floors the ratio, exactly as the reference itself behaves
    /// under `cargo test` and `cargo bench` (benches/benches.rs:113,130: 8096 -> 512).
    pub fn downsample<T: Copy>(ctx: &Context, src: &[T], dst: &mut [T]) {
        let (s, d, e) = (src.as_ptr() as *const c_void, dst.as_mut_ptr() as *mut c_void, std::mem::size_of::<T>());
        if cfg!(debug_assertions) { check(unsafe { aeth_host_downsample(ctx.h, s, src.len(), d, dst.len(), e) }); }
        else { check(unsafe { aeth_host_downsample_release(ctx.h, s, src.len(), d, dst.len(), e, 0) }); }
    }
    /// `sampling::downsample_sb<T: Copy>` (src/sampling.rs:49-62): the step_by variant
    pub fn downsample_sb<T: Copy>(ctx: &Context, src: &[T], dst: &mut [T]) {
        let (s, d, e) = (src.as_ptr() as *const c_void, dst.as_mut_ptr() as *mut c_void, std::mem::size_of::<T>());
        if cfg!(debug_assertions) { check(unsafe { aeth_host_downsample(ctx.h, s, src.len(), d, dst.len(), e) }); }
        else { check(unsafe { aeth_host_downsample_release(ctx.h, s, src.len(), d, dst.len(), e, 1) }); }
    }
}

/// Overlap-save FIR behind `fir::Fir`'s constructor shape (src/fir.rs:3-22 stores taps and a scratch but has
/// no filter method; this one filters).
/// Like `HipFft`, borrows its `Context` (Drop goes through the context) and stays on the context's thread.
pub struct Fir<'c> { h: *mut aeth_fir, _ctx: PhantomData<&'c Context> }
impl<'c> Fir<'c> {
    pub fn new(ctx: &'c Context, taps: &[cf32], fft_len: usize) -> Fir<'c> {
        let mut h = ptr::null_mut();
        check(unsafe { aeth_fir_create(ctx.h, taps.as_ptr(), taps.len(), fft_len, &mut h) });
        Fir { h, _ctx: PhantomData }
    }
    /// device-resident stream: y[n] = sum_k taps[k] x[n-k], zero initial state
    pub fn filter(&mut self, x: &DeviceVec, y: &mut DeviceVec) {
        assert_eq!(x.n, y.n, "Vectors must have same length");
        check(unsafe { aeth_fir_exec(self.h, ptr::null(), x.p, x.n, y.p) });
    }
    /// host-resident stream through the three-stage H2D | kernel | D2H pipeline (src/pipeline.rs counterpart)
    pub fn filter_stream(&mut self, x: &[cf32], y: &mut [cf32]) -> aeth_pipe_stats {
        assert_eq!(x.len(), y.len(), "Vectors must have same length");
        let mut st = aeth_pipe_stats::default();
        check(unsafe { aeth_fir_stream_host(self.h, x.as_ptr(), x.len(), y.as_mut_ptr(), 0, &mut st) });
        st
    }
    /// the same run, printing the reference pipeline's per-stage report (src/pipeline.rs:101-108) for the device stages
    /// and, when the slices had to be staged through the context's pinned pool, the two host stages
    pub fn filter_stream_report(&mut self, x: &[cf32], y: &mut [cf32]) -> aeth_pipe_util {
        assert_eq!(x.len(), y.len(), "Vectors must have same length");
        let mut u = aeth_pipe_util::default();
        check(unsafe { aeth_fir_stream_host_util(self.h, x.as_ptr(), x.len(), y.as_mut_ptr(), 0, &mut u) });
        for (name, active) in [("copy-in", u.active_copy_in), ("upload", u.active_upload), ("kernel", u.active_kernel),
                               ("download", u.active_download), ("copy-out", u.active_copy_out)].iter() {
            if name.starts_with("copy") && *active == 0.0 { continue; }
            println!("Stage: {:15} : Processed {} in {:3.3}s ({:9.2}/s); Utilisation: {:3.2}%",
                     name, u.chunks as u64, u.seconds, u.chunks / u.seconds, active / u.seconds * 100.0);
        }
        u
    }
}
impl<'c> Drop for Fir<'c> { fn drop(&mut self) { unsafe { aeth_fir_destroy(self.h); } } }

/// Polyphase analysis filter bank (no body in the reference: `waterfall`, src/util/plot.rs:46-68, frames with
/// chunks_mut(fft_len)): weight `proto.len()` = P * channels samples, fold them modulo `channels`, transform, advance by
/// `hop`.  `stream_phase`: bin phases refer to the first sample ever fed (pass the global number of a call's first frame).
pub struct Channelizer<'c> { h: *mut aeth_chan, _ctx: PhantomData<&'c Context> }
impl<'c> Channelizer<'c> {
    pub fn new(ctx: &'c Context, proto: &[f32], channels: usize, hop: usize, stream_phase: bool) -> Channelizer<'c> {
        let mut h = ptr::null_mut();
        let phase = if stream_phase { AETH_CHAN_PHASE_STREAM } else { AETH_CHAN_PHASE_FRAME };
        check(unsafe { aeth_chan_create(ctx.h, proto.as_ptr(), proto.len(), channels, hop, phase, 0, &mut h) });
        Channelizer { h, _ctx: PhantomData }
    }
    /// RECT / HANN / HAMMING / SINC_HAMMING taps (AETH_CHAN_PROTO_*), computed on the host
    pub fn prototype(kind: i32, channels: usize, taps_per_channel: usize) -> Vec<f32> {
        let mut w = vec![0f32; channels * taps_per_channel];
        check(unsafe { aeth_chan_prototype(kind, channels, taps_per_channel, w.as_mut_ptr()) });
        w
    }
    pub fn channels(&self) -> usize { unsafe { aeth_chan_channels(self.h) } }
    pub fn hop(&self) -> usize { unsafe { aeth_chan_hop(self.h) } }
    pub fn frames(&self, n: usize) -> usize { n / self.hop() }
    /// the folded frames alone; `hist`: the ntaps - hop samples in front of x (None: zeros)
    pub fn fold(&mut self, x: &DeviceVec, hist: Option<&DeviceVec>, first_frame: u64, out: &mut DeviceVec) {
        check(unsafe { aeth_chan_fold(self.h, hist.map_or(ptr::null(), |h| h.p as *const cf32), x.p, x.n, first_frame, out.p, out.n) });
    }
    /// fold, then `fwd` with Scale `s` on every frame
    pub fn exec(&mut self, x: &DeviceVec, hist: Option<&DeviceVec>, first_frame: u64, s: Scale, out: &mut DeviceVec) {
        let (kind, xs) = scale_args(s);
        check(unsafe { aeth_chan_exec(self.h, hist.map_or(ptr::null(), |h| h.p as *const cf32), x.p, x.n, first_frame,
                                      AETH_SIGN_REF_FWD, kind, xs, out.p, out.n) });
    }
    /// frames per chunk of `sums` (the launch geometry) and whether it takes the one-kernel route
    pub fn sums_chunk(&self) -> usize { unsafe { aeth_chan_sums_chunk(self.h) } }
    pub fn sums_fused(&self) -> bool { unsafe { aeth_chan_sums_fused(self.h) != 0 } }
    /// averaged spectra: per-bin sums and maxima of q over rows of `block` frames (0: one row); a plane that is None is not
    /// computed; `general`: never the one-kernel route
    pub fn sums(&mut self, x: &DeviceVec, hist: Option<&DeviceVec>, first_frame: u64, s: Scale, mirror: bool, block: usize, general: bool,
                sum: Option<&mut DeviceF64>, max: Option<&mut DeviceF64>) {
        let (kind, xs) = scale_args(s);
        let n_out = sum.as_ref().map(|v| v.n).or(max.as_ref().map(|v| v.n)).unwrap_or(0);
        check(unsafe { aeth_chan_exec_sums(self.h, hist.map_or(ptr::null(), |h| h.p as *const cf32), x.p, x.n, first_frame, AETH_SIGN_REF_FWD,
                                           kind, xs, mirror as i32, block, if general { AETH_SUMS_GENERAL } else { 0 },
                                           sum.map_or(ptr::null_mut(), |v| v.p), max.map_or(ptr::null_mut(), |v| v.p), n_out) });
    }
}
impl<'c> Drop for Channelizer<'c> { fn drop(&mut self) { unsafe { aeth_chan_destroy(self.h); } } }

/// Polyphase synthesis filter bank (no body in the reference: src/util/plot.rs:46-68 only takes a stream apart), the
/// transpose of `Channelizer`: every frame's `channels` time samples are extended periodically to `proto.len()`, weighted
/// and overlap-added at `hop`.  The output is the reconstruction delayed by `proto.len() - hop` samples.
pub struct Synthesizer<'c> { h: *mut aeth_synth, _ctx: PhantomData<&'c Context> }
impl<'c> Synthesizer<'c> {
    pub fn new(ctx: &'c Context, proto: &[f32], channels: usize, hop: usize, stream_phase: bool) -> Synthesizer<'c> {
        let mut h = ptr::null_mut();
        let phase = if stream_phase { AETH_CHAN_PHASE_STREAM } else { AETH_CHAN_PHASE_FRAME };
        check(unsafe { aeth_synth_create(ctx.h, proto.as_ptr(), proto.len(), channels, hop, phase, 0, &mut h) });
        Synthesizer { h, _ctx: PhantomData }
    }
    /// the synthesis window that inverts a windowed, overlapped transform of `w.len()` points at `hop`
    pub fn dual_window(w: &[f32], hop: usize) -> Vec<f32> {
        let mut g = vec![0f32; w.len()];
        check(unsafe { aeth_synth_dual_window(w.as_ptr(), w.len(), hop, g.as_mut_ptr()) });
        g
    }
    pub fn channels(&self) -> usize { unsafe { aeth_synth_channels(self.h) } }
    pub fn hop(&self) -> usize { unsafe { aeth_synth_hop(self.h) } }
    /// frames in front of a call's first that reach into its output
    pub fn history(&self) -> usize { unsafe { aeth_synth_history(self.h) } }
    pub fn samples(&self, n_in: usize) -> usize { n_in / self.channels() * self.hop() }
    /// the overlap-add alone; `hist`: the history() frames in front of `frames` (None: zeros)
    pub fn unfold(&mut self, frames: &DeviceVec, hist: Option<&DeviceVec>, first_frame: u64, out: &mut DeviceVec) {
        check(unsafe { aeth_synth_unfold(self.h, hist.map_or(ptr::null(), |h| h.p as *const cf32), frames.p, frames.n, first_frame,
                                         out.p, out.n) });
    }
    /// `bwd` with Scale `s` on every frame of `spec` (and of `hist`: both hold spectra), then the overlap-add
    pub fn exec(&mut self, spec: &DeviceVec, hist: Option<&DeviceVec>, first_frame: u64, s: Scale, out: &mut DeviceVec) {
        let (kind, xs) = scale_args(s);
        check(unsafe { aeth_synth_exec(self.h, hist.map_or(ptr::null(), |h| h.p as *const cf32), spec.p, spec.n, first_frame,
                                       AETH_SIGN_REF_BWD, kind, xs, out.p, out.n) });
    }
}
impl<'c> Drop for Synthesizer<'c> { fn drop(&mut self) { unsafe { aeth_synth_destroy(self.h); } } }

/// Polyphase rational resampler (no body in the reference: src/sampling.rs:7-62 has only linear interpolation and sample
/// picking): upsample by `up`, filter with the real taps, keep every `down`-th sample, in one pass.  A call over
/// n = B * down samples makes B * up outputs; the previous `history()` input samples make chunks concatenate exactly.
pub struct Resampler<'c> { h: *mut aeth_resamp, _ctx: PhantomData<&'c Context> }
impl<'c> Resampler<'c> {
    pub fn new(ctx: &'c Context, taps: &[f32], up: usize, down: usize) -> Resampler<'c> {
        let mut h = ptr::null_mut();
        check(unsafe { aeth_resamp_create(ctx.h, taps.as_ptr(), taps.len(), up, down, &mut h) });
        Resampler { h, _ctx: PhantomData }
    }
    /// `up * taps_per_phase` taps of the low-pass at 1 / (2 max(up, down)) cycles per upsampled sample, summing to `up`
    pub fn prototype(up: usize, down: usize, taps_per_phase: usize) -> Vec<f32> {
        let mut g = vec![0f32; up * taps_per_phase];
        check(unsafe { aeth_resamp_prototype(up, down, taps_per_phase, g.as_mut_ptr()) });
        g
    }
    pub fn up(&self) -> usize { unsafe { aeth_resamp_up(self.h) } }
    pub fn down(&self) -> usize { unsafe { aeth_resamp_down(self.h) } }
    pub fn ntaps(&self) -> usize { unsafe { aeth_resamp_ntaps(self.h) } }
    /// input samples in front of a call's first that reach into its output: taps per phase - 1
    pub fn history(&self) -> usize { unsafe { aeth_resamp_history(self.h) } }
    pub fn tile(&self) -> usize { unsafe { aeth_resamp_tile(self.h) } }
    pub fn route(&self) -> String { unsafe { std::ffi::CStr::from_ptr(aeth_resamp_route(self.h)) }.to_string_lossy().into_owned() }
    pub fn out_count(&self, n_in: usize) -> usize { unsafe { aeth_resamp_out_count(self.h, n_in) } }
    /// `hist`: the history() samples in front of `x` (None: zeros)
    pub fn exec(&mut self, x: &DeviceVec, hist: Option<&DeviceVec>, out: &mut DeviceVec) {
        check(unsafe { aeth_resamp_exec(self.h, hist.map_or(ptr::null(), |h| h.p as *const cf32), x.p, x.n, out.p, out.n) });
    }
}
impl<'c> Drop for Resampler<'c> { fn drop(&mut self) { unsafe { aeth_resamp_destroy(self.h); } } }

/// Arbitrary-ratio resampler (no body in the reference: src/sampling.rs:7-62 has only linear interpolation and sample
/// picking): 2^log2_phases phases whose taps are interpolated linearly between neighbours, behind an unsigned Q32.32 time
/// word.  Output m of a call stands at phase + m * step input samples; `advance` gives a call's output count and the next
/// call's phase, and the previous `history()` input samples make chunks concatenate exactly.
pub struct ArbResampler<'c> { h: *mut aeth_arb, _ctx: PhantomData<&'c Context> }
impl<'c> ArbResampler<'c> {
    pub fn new(ctx: &'c Context, taps: &[f32], log2_phases: usize) -> ArbResampler<'c> {
        let mut h = ptr::null_mut();
        check(unsafe { aeth_arb_create(ctx.h, taps.as_ptr(), taps.len(), log2_phases, &mut h) });
        ArbResampler { h, _ctx: PhantomData }
    }
    /// the Q32.32 word of `ratio` input samples per output sample, truncated
    pub fn step_word(ratio: f64) -> u64 { (ratio * 4294967296.0) as u64 }
    /// (outputs of a call over n input samples from `phase`, the phase of the call behind it)
    pub fn advance(step: u64, phase: u64, n: usize) -> (usize, u64) {
        let (mut count, mut next) = (0usize, 0u64);
        check(unsafe { aeth_arb_advance(step, phase, n, &mut count, &mut next) });
        (count, next)
    }
    pub fn phases(&self) -> usize { unsafe { aeth_arb_phases(self.h) } }
    pub fn ntaps(&self) -> usize { unsafe { aeth_arb_ntaps(self.h) } }
    /// input samples in front of a call's first that reach into its output: taps per phase - 1
    pub fn history(&self) -> usize { unsafe { aeth_arb_history(self.h) } }
    pub fn tile(&self, step: u64) -> usize { unsafe { aeth_arb_tile(self.h, step) } }
    pub fn route(&self, step: u64) -> String { unsafe { std::ffi::CStr::from_ptr(aeth_arb_route(self.h, step)) }.to_string_lossy().into_owned() }
    /// `hist`: the history() samples in front of `x` (None: zeros); `out` holds advance(step, phase, x.n).0 samples
    pub fn exec(&mut self, x: &DeviceVec, step: u64, phase: u64, hist: Option<&DeviceVec>, out: &mut DeviceVec) {
        check(unsafe { aeth_arb_exec(self.h, hist.map_or(ptr::null(), |h| h.p as *const cf32), x.p, x.n, step, phase, out.p, out.n) });
    }
}
impl<'c> Drop for ArbResampler<'c> { fn drop(&mut self) { unsafe { aeth_arb_destroy(self.h); } } }

/// Numerically controlled oscillator (no body in the reference: it has no frequency shift, tone or chirp).  Three 64-bit
/// words, fractions of a turn scaled by 2^64: w(n) = phase + n * step + n (n - 1) / 2 * rate modulo 2^64, exact at every
/// stream position.  `mix` and `tone` advance `position` by the samples they handled: chunks concatenate bit for bit.
pub struct Nco<'c> { ctx: &'c Context, pub words: aeth_nco_words, pub position: u64 }
impl<'c> Nco<'c> {
    /// `freq` in cycles per sample, `phase` in cycles, `rate` in cycles per sample per sample
    pub fn new(ctx: &'c Context, freq: f64, phase: f64, rate: f64, position: u64) -> Nco<'c> {
        Nco { ctx, words: aeth_nco_words { phase: Nco::word(phase), step: Nco::word(freq), rate: Nco::word(rate) }, position }
    }
    pub fn from_words(ctx: &'c Context, words: aeth_nco_words, position: u64) -> Nco<'c> { Nco { ctx, words, position } }
    pub fn word(cycles: f64) -> u64 { unsafe { aeth_nco_word(cycles) } }
    pub fn word_at(words: &aeth_nco_words, n: u64) -> u64 { unsafe { aeth_nco_word_at(words, n) } }
    pub fn phasor(word: u64) -> cf32 {
        let mut out = cf32::new(0.0, 0.0);
        check(unsafe { aeth_nco_phasor(word, &mut out) });
        out
    }
    pub fn seek(&mut self, position: u64) { self.position = position; }
    pub fn mix(&mut self, x: &DeviceVec, out: &mut DeviceVec) {
        assert_eq!(x.n, out.n, "Nco::mix: the output's length is not the input's");
        check(unsafe { aeth_nco_mix(self.ctx.h, &self.words, self.position, x.p, out.p, x.n) });
        self.position += x.n as u64;
    }
    pub fn mix_in_place(&mut self, x: &mut DeviceVec) {
        check(unsafe { aeth_nco_mix(self.ctx.h, &self.words, self.position, x.p, x.p, x.n) });
        self.position += x.n as u64;
    }
    pub fn tone(&mut self, amp: f32, out: &mut DeviceVec) {
        check(unsafe { aeth_nco_tone(self.ctx.h, &self.words, self.position, amp, out.p, out.n) });
        self.position += out.n as u64;
    }
}

/// Synchronisation estimators (no body in the reference: it estimates no offset).  `line` sums a non-linearity of the
/// samples against the oscillator's phasor (kind 0, the square law, with step = word(-1 / sps): symbol timing; kind M in
/// 1, 2, 4, 8 without words: the M-th power carrier phase), `lag` sums pw_M(x[i]) * conj(pw_M(x[i - lag])) (carrier
/// frequency).  f64 sums in a fixed order: one record per `block` samples at `rec_dev` (device memory of
/// ceil(n / block) records, or None) and the total, for which the call waits.
pub struct Sync;
impl Sync {
    pub const SQUARE: i32 = 0;
    pub fn chunk() -> usize { unsafe { aeth_sync_chunk() } }
    pub fn line(ctx: &Context, kind: i32, words: Option<&aeth_nco_words>, position: u64, x: &DeviceVec, block: usize,
                rec_dev: Option<*mut aeth_sync_record>) -> aeth_sync_record {
        let mut total = aeth_sync_record::default();
        check(unsafe { aeth_sync_line(ctx.h, kind, words.map_or(ptr::null(), |w| w as *const aeth_nco_words), position, x.p, x.n, block,
                                      rec_dev.unwrap_or(ptr::null_mut()), &mut total) });
        total
    }
    /// `hist`: the `lag` samples in front of `x` (None: the terms i < lag do not exist)
    pub fn lag(ctx: &Context, power: i32, lag: usize, hist: Option<&DeviceVec>, x: &DeviceVec, block: usize,
               rec_dev: Option<*mut aeth_sync_record>) -> aeth_sync_record {
        let mut total = aeth_sync_record::default();
        check(unsafe { aeth_sync_lag(ctx.h, power, lag, hist.map_or(ptr::null(), |h| h.p as *const cf32), x.p, x.n, block,
                                     rec_dev.unwrap_or(ptr::null_mut()), &mut total) });
        total
    }
    /// atan2(im, re) / (2 pi)
    pub fn turns(r: &aeth_sync_record) -> f64 { unsafe { aeth_sync_turns(r) } }
    /// the oscillator step that removes the offset a lag sum of that power and lag has seen
    pub fn freq_step(r: &aeth_sync_record, power: i32, lag: usize) -> u64 { unsafe { aeth_sync_freq_step(r, power, lag) } }
    /// the Q32.32 phase of the first symbol instant, for a square-law line taken with step = word(-1 / sps)
    pub fn timing_phase(r: &aeth_sync_record, sps: f64) -> u64 { unsafe { aeth_sync_timing_phase(r, sps) } }
}

/// Moving-window detectors (no body in the reference): for every sample the sum of the last `window` lag terms
/// x[j] * conj(x[j - lag]) and powers, the timing metric |P|^2 / (R(i) R(i - lag)) (kind `AETH_MOV_LAG`) or the moving mean
/// power (`AETH_MOV_POWER`, lag 0).  `hist`: the `history()` samples in front of `x` (None: zeros).
pub struct Mov;
impl Mov {
    pub fn history(kind: i32, window: usize, lag: usize) -> usize { unsafe { aeth_mov_history(kind, window, lag) } }
    /// a stream cut at a multiple of this continues bit for bit
    pub fn grid(kind: i32, window: usize) -> usize { unsafe { aeth_mov_grid(kind, window) } }
    /// the planes that are given: P as cf32, R and the metric as f32, one value per sample; stream-ordered, no wait
    pub fn exec(ctx: &Context, kind: i32, window: usize, lag: usize, hist: Option<&DeviceVec>, x: &DeviceVec, p: Option<&mut DeviceVec>,
                r_dev: Option<*mut f32>, m_dev: Option<*mut f32>) {
        check(unsafe { aeth_mov_exec(ctx.h, kind, window, lag, hist.map_or(ptr::null(), |h| h.p as *const cf32), x.p, x.n,
                                     p.map_or(ptr::null_mut(), |v| v.p), r_dev.unwrap_or(ptr::null_mut()), m_dev.unwrap_or(ptr::null_mut())) });
    }
    /// one record per `block` samples at `peaks_dev` (device memory of ceil(n / block) records, or None) and the record
    /// over the whole call, for which the call waits
    pub fn search(ctx: &Context, kind: i32, window: usize, lag: usize, r_min: f64, threshold: f64, hist: Option<&DeviceVec>, x: &DeviceVec,
                  block: usize, peaks_dev: Option<*mut aeth_mov_peak>) -> aeth_mov_peak {
        let mut best = aeth_mov_peak::default();
        check(unsafe { aeth_mov_search(ctx.h, kind, window, lag, r_min, threshold, hist.map_or(ptr::null(), |h| h.p as *const cf32), x.p, x.n,
                                       block, peaks_dev.unwrap_or(ptr::null_mut()), &mut best) });
        best
    }
    /// the oscillator step that removes the offset the lag sum of the record has seen
    pub fn freq_step(p: &aeth_mov_peak, lag: usize) -> u64 { unsafe { aeth_mov_freq_step(p, lag) } }
}

/// Convolutional code (no body in the reference: it has no forward error correction): a rate 1/n code of constraint
/// length k = 3 .. 7, polynomials in the octal convention with the current bit at the MSB (K = 7: 0o171, 0o133).  Bits are
/// one byte each; soft values are i8, positive meaning bit 0 is likelier, 0 an erasure.  `decode` is a causal system with
/// a delay of `traceback()` steps: out[o] is the decision for step o - traceback().
pub struct ConvCode<'c> { h: *mut aeth_cc, _ctx: &'c Context }
impl<'c> ConvCode<'c> {
    /// output block `block`, warm-up `warmup` and traceback `traceback` in trellis steps (block + traceback <= 4096)
    pub fn new(ctx: &'c Context, k: u32, polys: &[u32], block: usize, warmup: usize, traceback: usize) -> ConvCode<'c> {
        assert!(polys.len() <= 4, "ConvCode::new: at most 4 polynomials");
        let mut code = aeth_cc_code { k, n: polys.len() as u32, poly: [0; 4] };
        code.poly[..polys.len()].copy_from_slice(polys);
        let mut h = ptr::null_mut();
        check(unsafe { aeth_cc_create(ctx.h, &code, block, warmup, traceback, &mut h) });
        ConvCode { h, _ctx: ctx }
    }
    pub fn k(&self) -> usize { unsafe { aeth_cc_k(self.h) } }
    pub fn n(&self) -> usize { unsafe { aeth_cc_n(self.h) } }
    pub fn block(&self) -> usize { unsafe { aeth_cc_block(self.h) } }
    pub fn warmup(&self) -> usize { unsafe { aeth_cc_warmup(self.h) } }
    pub fn traceback(&self) -> usize { unsafe { aeth_cc_traceback(self.h) } }
    /// warmup + traceback: the steps of soft values a continued `decode` wants in front
    pub fn history(&self) -> usize { unsafe { aeth_cc_history(self.h) } }
    /// `hist_dev`: the k - 1 bits before `bits_dev[0]` (None: zeros); `coded_dev` holds nbits * n bytes
    pub fn encode(&mut self, hist_dev: Option<*const u8>, bits_dev: *const u8, nbits: usize, coded_dev: *mut u8, ncoded: usize) {
        check(unsafe { aeth_cc_encode(self.h, hist_dev.unwrap_or(ptr::null()), bits_dev, nbits, coded_dev, ncoded) });
    }
    /// `hist_dev`: the history() * n soft values before `soft_dev[0]` (None: erasures); `bits_dev` holds nsoft / n bytes
    pub fn decode(&mut self, hist_dev: Option<*const i8>, soft_dev: *const i8, nsoft: usize, bits_dev: *mut u8, nbits: usize) {
        check(unsafe { aeth_cc_decode(self.h, hist_dev.unwrap_or(ptr::null()), soft_dev, nsoft, bits_dev, nbits) });
    }
}
impl<'c> Drop for ConvCode<'c> { fn drop(&mut self) { unsafe { aeth_cc_destroy(self.h); } } }

/// Rate matching (no body in the reference): a periodic byte map, out[q r_out + i] = in[q r_in + map[i]], or `fill` where
/// map[i] is -1.  Puncturing, depuncturing to erasures, block interleaving and any chain of them are this one gather.  The
/// table builders are host-only integer arithmetic and need no context.
pub struct Remap<'c> { h: *mut aeth_remap, map: Vec<i32>, r_in: usize, ctx: &'c Context }
impl<'c> Remap<'c> {
    pub fn new(ctx: &'c Context, map: &[i32], r_in: usize) -> Remap<'c> {
        let mut h = ptr::null_mut();
        check(unsafe { aeth_remap_create(ctx.h, map.as_ptr(), map.len(), r_in, &mut h) });
        Remap { h, map: map.to_vec(), r_in, ctx }
    }
    /// keep[i] & 1: coded bit i of a period of keep.len() is sent
    pub fn puncture(ctx: &'c Context, keep: &[u8]) -> Remap<'c> {
        let (mut map, mut r_out) = (vec![0i32; keep.len().max(1)], 0usize);
        check(unsafe { aeth_remap_puncture(keep.as_ptr(), keep.len(), map.as_mut_ptr(), map.len(), &mut r_out) });
        map.truncate(r_out);
        Remap::new(ctx, &map, keep.len())
    }
    /// written row by row, read column by column
    pub fn rows_cols(ctx: &'c Context, rows: usize, cols: usize) -> Remap<'c> {
        let mut map = vec![0i32; (rows * cols).clamp(1, 1 << 20)];
        check(unsafe { aeth_remap_rows_cols(rows, cols, map.as_mut_ptr()) });
        Remap::new(ctx, &map, rows * cols)
    }
    /// the interleaver of 802.11a 17.3.5.6 over n_cbps coded bits at n_bpsc bits per carrier
    pub fn bicm16(ctx: &'c Context, n_cbps: usize, n_bpsc: usize) -> Remap<'c> {
        let mut map = vec![0i32; n_cbps.clamp(1, 1 << 20)];
        check(unsafe { aeth_remap_bicm16(n_cbps, n_bpsc, map.as_mut_ptr()) });
        Remap::new(ctx, &map, n_cbps)
    }
    /// the depuncturer of a puncturer, the deinterleaver of an interleaver, the first copy of a repetition
    pub fn inverse(&self) -> Remap<'c> {
        let mut inv = vec![0i32; self.r_in];
        check(unsafe { aeth_remap_invert(self.map.as_ptr(), self.map.len(), self.r_in, inv.as_mut_ptr()) });
        Remap::new(self.ctx, &inv, self.map.len())
    }
    /// `other` applied to the output of this map, as one map
    pub fn then(&self, other: &Remap<'c>) -> Remap<'c> {
        let (mut map, mut r_out, mut r_in) = (vec![0i32; 1 << 20], 0usize, 0usize);
        check(unsafe { aeth_remap_compose(self.map.as_ptr(), self.map.len(), self.r_in, other.map.as_ptr(), other.map.len(), other.r_in,
                                          map.as_mut_ptr(), map.len(), &mut r_out, &mut r_in) });
        map.truncate(r_out);
        Remap::new(self.ctx, &map, r_in)
    }
    pub fn in_period(&self) -> usize { unsafe { aeth_remap_in_period(self.h) } }
    pub fn out_period(&self) -> usize { unsafe { aeth_remap_out_period(self.h) } }
    /// the input bytes a call that writes `n_out` bytes reads
    pub fn in_count(&self, n_out: usize) -> usize { unsafe { aeth_remap_in_count(self.h, n_out) } }
    /// AETH_REMAP_ROUTE_TILE or AETH_REMAP_ROUTE_GATHER
    pub fn route(&self) -> i32 { unsafe { aeth_remap_route(self.h) } }
    /// periods per tile on the tile route, 0 on the gather route
    pub fn tile(&self) -> usize { unsafe { aeth_remap_tile(self.h) } }
    /// device pointers to bytes of any meaning (u8 bits, i8 soft values); `fill` stands where the map holds -1
    pub fn exec(&mut self, in_dev: *const c_void, n_in: usize, out_dev: *mut c_void, n_out: usize, fill: u8) {
        check(unsafe { aeth_remap_exec(self.h, in_dev, n_in, out_dev, n_out, fill) });
    }
}
impl<'c> Drop for Remap<'c> { fn drop(&mut self) { unsafe { aeth_remap_destroy(self.h); } } }

/// Frame checks (no body in the reference): a CRC of width r <= 64 over contiguous frames of one length, bits one byte per
/// bit, check bits highest coefficient first.  `registers` is the streaming primitive (no xorout), `attach` appends the r
/// check bits, `check` forms diff = received ^ computed ^ mask per frame, strips the payload and folds {n_bad, first_bad}.
pub struct Crc<'c> { h: *mut aeth_crc, _ctx: &'c Context }
impl<'c> Crc<'c> {
    pub fn new(ctx: &'c Context, r: u32, poly: u64, init: u64, xorout: u64) -> Crc<'c> {
        let mut h = ptr::null_mut();
        check(unsafe { aeth_crc_create(ctx.h, r, poly, init, xorout, &mut h) });
        Crc { h, _ctx: ctx }
    }
    /// a catalogue name: "crc-24/lte-a", "crc-32", ...
    pub fn named(ctx: &'c Context, name: &str) -> Crc<'c> {
        let (mut r, mut poly, mut init, mut xorout) = (0u32, 0u64, 0u64, 0u64);
        let name = std::ffi::CString::new(name).expect("a CRC name holds no NUL");
        check(unsafe { aeth_crc_named(name.as_ptr(), &mut r, &mut poly, &mut init, &mut xorout) });
        Crc::new(ctx, r, poly, init, xorout)
    }
    pub fn width(&self) -> u32 { unsafe { aeth_crc_width(self.h) } }
    pub fn poly(&self) -> u64 { unsafe { aeth_crc_poly(self.h) } }
    pub fn init(&self) -> u64 { unsafe { aeth_crc_init(self.h) } }
    pub fn xorout(&self) -> u64 { unsafe { aeth_crc_xorout(self.h) } }
    /// the register (before xorout) any frame followed by its own check bits leaves
    pub fn residue(&self) -> u64 { unsafe { aeth_crc_residue(self.h) } }
    /// AETH_CRC_ROUTE_FRAMES or AETH_CRC_ROUTE_LONG
    pub fn route(&self, l: usize, f: usize) -> i32 { unsafe { aeth_crc_route(self.h, l, f) } }
    pub fn route_frame_bits(&self) -> usize { unsafe { aeth_crc_route_frame_bits(self.h) } }
    pub fn frames_per_workgroup(&self, frame_bytes: usize) -> usize { unsafe { aeth_crc_frames_per_workgroup(self.h, frame_bytes) } }
    /// `state_in_dev` may be null: every frame starts from init
    pub fn registers(&mut self, bits_dev: *const u8, l: usize, f: usize, state_in_dev: *const u64, state_out_dev: *mut u64) {
        check(unsafe { aeth_crc_exec(self.h, bits_dev, l, f, state_in_dev, state_out_dev) });
    }
    pub fn attach(&mut self, in_dev: *const u8, l: usize, f: usize, out_dev: *mut u8) {
        check(unsafe { aeth_crc_attach(self.h, in_dev, l, f, out_dev) });
    }
    /// any of the three outputs may be null, not all
    pub fn check(&mut self, in_dev: *const u8, l: usize, f: usize, mask: u64, diff_dev: *mut u64, payload_dev: *mut u8,
                 summary_dev: *mut aeth_crc_summary) {
        check(unsafe { aeth_crc_check(self.h, in_dev, l, f, mask, diff_dev, payload_dev, summary_dev) });
    }
    /// the definition on host memory, no context: the register of `bits` (one byte per bit) started from init
    pub fn host(r: u32, poly: u64, init: u64, xorout: u64, bits: &[u8]) -> u64 {
        let mut reg = 0u64;
        check(unsafe { aeth_crc_host(r, poly, init, xorout, bits.as_ptr(), bits.len(), &mut reg) });
        reg
    }
}
impl<'c> Drop for Crc<'c> { fn drop(&mut self) { unsafe { aeth_crc_destroy(self.h); } } }

/// one byte per bit -> ceil(nbits / 8) bytes; `order` is AETH_BITS_LSB_FIRST or AETH_BITS_MSB_FIRST
pub fn pack(ctx: &Context, bits_dev: *const u8, nbits: usize, order: i32, bytes_dev: *mut u8) {
    check(unsafe { aeth_bits_pack(ctx.h, bits_dev, nbits, order, bytes_dev, (nbits + 7) / 8) });
}
/// bytes -> `nbits` <= 8 nbytes bytes of 0 / 1
pub fn unpack(ctx: &Context, bytes_dev: *const u8, nbytes: usize, order: i32, bits_dev: *mut u8, nbits: usize) {
    check(unsafe { aeth_bits_unpack(ctx.h, bytes_dev, nbytes, order, bits_dev, nbits) });
}

/// OFDM symbols (no body in the reference: it has `Fft`, `vec_mul` and `chunks_mut(fft_len)` framing only): a transform
/// length, a cyclic prefix and a carrier list (`bins[k]`: the FFT bin of carrier k).  `demod` strips the prefix, transforms
/// with the sign of `Fft::fwd`, picks the carriers and multiplies by `eq[k]` in one kernel; `modulate` is the way back with
/// the sign of `Fft::bwd`; `estimate` sums the training symbols per carrier in f64.
pub struct Ofdm<'c> { h: *mut aeth_ofdm, _ctx: &'c Context }
impl<'c> Ofdm<'c> {
    /// `max_symbols`: the symbols of one call at most (0: no bound); `general`: never take the fused kernel
    pub fn new(ctx: &'c Context, n_fft: usize, cp: usize, bins: &[u32], max_symbols: usize, general: bool) -> Ofdm<'c> {
        let mut h = ptr::null_mut();
        check(unsafe { aeth_ofdm_create(ctx.h, n_fft, cp, bins.as_ptr(), bins.len(), max_symbols, if general { AETH_OFDM_GENERAL } else { 0 }, &mut h) });
        Ofdm { h, _ctx: ctx }
    }
    pub fn len(&self) -> usize { unsafe { aeth_ofdm_len(self.h) } }
    pub fn cp(&self) -> usize { unsafe { aeth_ofdm_cp(self.h) } }
    pub fn symbol(&self) -> usize { unsafe { aeth_ofdm_symbol(self.h) } }
    pub fn carriers(&self) -> usize { unsafe { aeth_ofdm_carriers(self.h) } }
    pub fn route(&self) -> String { unsafe { std::ffi::CStr::from_ptr(aeth_ofdm_route(self.h)) }.to_string_lossy().into_owned() }
    /// samples `demod` reads for `n_sym` symbols: (n_sym - 1) * symbol() + len()
    pub fn span(&self, n_sym: usize) -> usize { unsafe { aeth_ofdm_span(self.h, n_sym) } }
    /// `x` starts at the first window sample; `eq`: carriers() coefficients; `out` holds n_sym * carriers()
    pub fn demod(&mut self, x: &DeviceVec, n_sym: usize, eq: Option<&DeviceVec>, scale: Scale, out: &mut DeviceVec) {
        let (k, s) = scale_args(scale);
        check(unsafe { aeth_ofdm_demod(self.h, x.p, x.n, n_sym, eq.map_or(ptr::null(), |e| e.p as *const cf32), k, s, out.p, out.n) });
    }
    /// `carriers` holds n_sym * carriers(), `out` n_sym * symbol() samples
    pub fn modulate(&mut self, carriers: &DeviceVec, n_sym: usize, scale: Scale, out: &mut DeviceVec) {
        let (k, s) = scale_args(scale);
        check(unsafe { aeth_ofdm_mod(self.h, carriers.p, carriers.n, n_sym, k, s, out.p, out.n) });
    }
    /// `y`: n_sym received training symbols, `x_known`: one symbol or n_sym of them; `eq_kind`: AETH_OFDM_EQ_*; any output may be
    /// None, not all
    pub fn estimate(&mut self, y: &DeviceVec, x_known: &DeviceVec, n_sym: usize, nv: f32, eq_kind: i32, h: Option<&mut DeviceVec>,
                    eq: Option<&mut DeviceVec>, csi: Option<&mut DeviceF32>) {
        let x_sym = if self.carriers() > 0 { x_known.n / self.carriers() } else { 0 };
        check(unsafe { aeth_ofdm_estimate(self.h, y.p, x_known.p, n_sym, x_sym, nv, eq_kind, h.map_or(ptr::null_mut(), |v| v.p),
                                          eq.map_or(ptr::null_mut(), |v| v.p), csi.map_or(ptr::null_mut(), |v| v.p)) });
    }
}
impl<'c> Drop for Ofdm<'c> { fn drop(&mut self) { unsafe { aeth_ofdm_destroy(self.h); } } }

/// The device counterpart of `pipeline::new().add_stage(..)` (src/pipeline.rs:24-41, :123-137): five fixed stages --
/// copy-in | upload | compute | download | copy-out -- whose compute stage is one of the library's device ops (a closure
/// cannot cross the C ABI).  `run` takes host slices and returns what `aeth_stream_host` reports.
pub struct Stage<'c> { op: aeth_stream_op, ctx: &'c Context }
impl<'c> Stage<'c> {
    fn blank(ctx: &'c Context, kind: std::os::raw::c_int) -> Stage<'c> {
        Stage { ctx, op: aeth_stream_op { kind, fir: ptr::null_mut(), fft: ptr::null_mut(), sig_dev: ptr::null(), n_sig: 0, sign: 0,
                                          scale_kind_fwd: 0, x_fwd: 0.0, scale_kind_bwd: 0, x_bwd: 0.0, bits_per_symbol: 0,
                                          table_host: ptr::null(), compat: 0, n_between: 0, seed: 0, offset: 0 } }
    }
    pub fn fir(ctx: &'c Context, f: &Fir<'c>) -> Stage<'c> { let mut s = Stage::blank(ctx, AETH_STREAM_FIR); s.op.fir = f.h; s }
    /// `Fft::fwd` over `chunks_mut(fft_len)` (src/util/plot.rs:59-61)
    pub fn fft(ctx: &'c Context, f: &HipFft<'c>, scale: Scale) -> Stage<'c> {
        let (k, x) = scale_args(scale);
        let mut s = Stage::blank(ctx, AETH_STREAM_FFT); s.op.fft = f.h; s.op.sign = AETH_SIGN_REF_FWD; s.op.scale_kind_fwd = k; s.op.x_fwd = x; s
    }
    /// `vec_rfft -> vec_mul(&sig) -> vec_rifft` per frame (benches/benches.rs:410-416)
    pub fn mul_chain(ctx: &'c Context, f: &HipFft<'c>, sig: &DeviceVec, s_fwd: Scale, s_bwd: Scale) -> Stage<'c> {
        let (kf, xf) = scale_args(s_fwd); let (kb, xb) = scale_args(s_bwd);
        let mut s = Stage::blank(ctx, AETH_STREAM_FFT_MUL_IFFT); s.op.fft = f.h; s.op.sig_dev = sig.p; s.op.n_sig = sig.n;
        s.op.scale_kind_fwd = kf; s.op.x_fwd = xf; s.op.scale_kind_bwd = kb; s.op.x_bwd = xb; s
    }
    /// the chain, then `Modulation::demod_naive` (examples/modem.rs:28-31): `bits_per_symbol` bytes out per sample
    pub fn correlate_demod(ctx: &'c Context, f: &HipFft<'c>, sig: &DeviceVec, bits_per_symbol: usize) -> Stage<'c> {
        let mut s = Stage::blank(ctx, AETH_STREAM_FFT_MUL_IFFT_DEMOD); s.op.fft = f.h; s.op.sig_dev = sig.p; s.op.n_sig = sig.n;
        s.op.bits_per_symbol = bits_per_symbol as std::os::raw::c_int; s.op.compat = 1; s
    }
    /// the transform, then `sampling::interpolate` per frame (src/sampling.rs:7-24)
    pub fn fft_interpolate(ctx: &'c Context, f: &HipFft<'c>, n_between: usize, scale: Scale) -> Stage<'c> {
        let (k, x) = scale_args(scale);
        let mut s = Stage::blank(ctx, AETH_STREAM_FFT_INTERPOLATE); s.op.fft = f.h; s.op.sign = AETH_SIGN_REF_FWD;
        s.op.scale_kind_fwd = k; s.op.x_fwd = x; s.op.n_between = n_between; s.op.compat = 1; s
    }
    pub fn out_count(&self, n_in: usize) -> usize { unsafe { aeth_stream_out_count(self.ctx.h, &self.op, n_in) } }
    /// cf32 in, `T` out (`cf32`, or `u8` for the demodulating stage); `out.len()` must be `out_count(x.len())`
    pub fn run<T: Copy>(&self, x: &[cf32], out: &mut [T]) -> aeth_pipe_stats {
        assert_eq!(out.len(), self.out_count(x.len()), "Vectors must have same length");
        let mut st = aeth_pipe_stats::default();
        check(unsafe { aeth_stream_host(self.ctx.h, &self.op, x.as_ptr() as *const _, x.len(), out.as_mut_ptr() as *mut _, out.len(), 0, &mut st) });
        st
    }
}

/// Pinned host buffers behind the reference's `pool::Pool<T>` (src/pool.rs:43-221): `take`, `take_or_make`, `len`,
/// `cap`; an `Elem` derefs into `[cf32]` and goes back to the pool on drop.  Elements are page-locked once by the
/// library, so `Fir::filter_stream` copies from / to them directly (no staging, no registration of caller memory).
pub struct PinnedPool<'c> { h: *mut aeth_pool, n: usize, _ctx: PhantomData<&'c Context> }
pub struct PinnedElem<'p, 'c> { pool: &'p PinnedPool<'c>, p: *mut cf32 }
impl<'c> PinnedPool<'c> {
    /// `pool::make(initial_len, maker, resetter)` with maker = one pinned buffer of `n` samples
    pub fn make(ctx: &'c Context, n: usize, initial_len: usize, zero_on_return: bool) -> PinnedPool<'c> {
        let mut h = ptr::null_mut();
        check(unsafe { aeth_pool_create(ctx.h, n * std::mem::size_of::<cf32>(), initial_len,
                                        if zero_on_return { AETH_POOL_ZERO_ON_RETURN } else { 0 }, &mut h) });
        PinnedPool { h, n, _ctx: PhantomData }
    }
    pub fn take(&self) -> Option<PinnedElem<'_, 'c>> {
        let mut p = ptr::null_mut();
        check(unsafe { aeth_pool_take(self.h, &mut p) });
        if p.is_null() { None } else { Some(PinnedElem { pool: self, p: p as *mut cf32 }) }
    }
    pub fn take_or_make(&self) -> PinnedElem<'_, 'c> {
        let mut p = ptr::null_mut();
        check(unsafe { aeth_pool_take_or_make(self.h, &mut p) });
        PinnedElem { pool: self, p: p as *mut cf32 }
    }
    pub fn len(&self) -> usize { unsafe { aeth_pool_len(self.h) } }
    pub fn cap(&self) -> usize { unsafe { aeth_pool_cap(self.h) } }
}
impl<'c> Drop for PinnedPool<'c> { fn drop(&mut self) { unsafe { aeth_pool_destroy(self.h); } } }
impl<'p, 'c> Drop for PinnedElem<'p, 'c> { fn drop(&mut self) { unsafe { aeth_pool_give_back(self.pool.h, self.p as *mut c_void); } } }
impl<'p, 'c> std::ops::Deref for PinnedElem<'p, 'c> {
    type Target = [cf32];
    fn deref(&self) -> &[cf32] { unsafe { std::slice::from_raw_parts(self.p, self.pool.n) } }
}
impl<'p, 'c> std::ops::DerefMut for PinnedElem<'p, 'c> {
    fn deref_mut(&mut self) -> &mut [cf32] { unsafe { std::slice::from_raw_parts_mut(self.p, self.pool.n) } }
}

/// `modulation::Modulation` for the generic BPSK/QPSK tables (src/modulation.rs:5-149) on device buffers,
/// and `noise::Awgn::apply` (src/noise.rs:53-59).
pub mod modem {
    use super::*;
    /// `m.modulate(&bits)`: one u8 per bit in, `bits.len() / bits_per_symbol` symbols out
    pub fn modulate(ctx: &Context, bits_dev: *const u8, nbits: usize, bits_per_symbol: i32, out: &mut DeviceVec) {
        check(unsafe { aeth_modulate(ctx.h, bits_dev, nbits, bits_per_symbol, ptr::null(), out.p, out.n) });
    }
    /// `m.demod_naive(..)`; `compat` reproduces the reference's `idx & 1u8 << 1` output (src/modulation.rs:54)
    pub fn demod_naive(ctx: &Context, sym: &DeviceVec, bits_per_symbol: i32, bits_dev: *mut u8, nbits: usize, compat: bool) {
        check(unsafe { aeth_demod_naive(ctx.h, sym.p, sym.n, bits_per_symbol, ptr::null(), bits_dev, nbits, compat as i32) });
    }
    /// soft decisions for `ConvCode::decode` (no body in the reference): `bits_per_symbol` i8 values per symbol
    pub fn demod_soft(ctx: &Context, sym: &DeviceVec, bits_per_symbol: i32, scale: f32, out_dev: *mut i8, nout: usize) {
        check(unsafe { aeth_demod_soft(ctx.h, sym.p, sym.n, bits_per_symbol, ptr::null(), scale, out_dev, nout) });
    }
    /// `noise::new(power, seed).apply(&mut signal)` -- the double scaling of the reference is kept
    pub fn awgn_apply(ctx: &Context, signal: &mut DeviceVec, power: f32, seed: u64, offset: u64) {
        check(unsafe { aeth_awgn_apply(ctx.h, signal.p, signal.n, power, seed, offset) });
    }
}
