// aether_hip.hpp -- header-only C++17 host wrapper over the C ABI (aether_hip.h).
//
// The reference is Rust; its toolchain is absent from this pipeline, so the host
// side above the C ABI is mirrored here in C++ with the reference's own names,
// argument meaning and error behaviour:
//   aether::Scale            <-> enum Scale              (src/fft.rs:6-38)
//   aether::Fft / HipFft     <-> trait Fft / struct Cfft (src/fft.rs:48-77, :134-235)
//   aether::DeviceVec        <-> trait VecOps on [cf32]  (src/vecops.rs:39-89), device-resident
//   aether::HostVec          <-> the same on a host slice (one H2D + D2H per call)
//   aether::interpolate / downsample                     (src/sampling.rs:7-62)
//   aether::assert_evm                                   (src/lib.rs:26-49)
// The reference panics on misuse (assert_eq!); here the same conditions throw
// aether::Panic carrying the reference's message text.
#pragma once

#include <algorithm>
#include <cmath>
#include <complex>
#include <cstddef>
#include <cstdio>
#include <functional>
#include <stdexcept>
#include <string>
#include <vector>

#include "aether_hip.h"

namespace aether {

using cf32 = std::complex<float>;     // layout-compatible with aeth_cf32 / Complex<f32>
static_assert(sizeof(cf32) == sizeof(aeth_cf32), "cf32 layout");

struct Panic : std::runtime_error {
    int code;
    Panic(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

inline void check(int rc)
{
    if (rc != AETH_OK) throw Panic(rc, aeth_last_error());
}

inline aeth_cf32 *raw(cf32 *p) { return reinterpret_cast<aeth_cf32 *>(p); }
inline const aeth_cf32 *raw(const cf32 *p) { return reinterpret_cast<const aeth_cf32 *>(p); }

// ---- enum Scale (src/fft.rs:6-18) ------------------------------------------------
struct Scale {
    int kind;
    float x;
    static Scale None() { return {AETH_SCALE_NONE, 0.f}; }
    static Scale SN() { return {AETH_SCALE_SN, 0.f}; }
    static Scale N() { return {AETH_SCALE_N, 0.f}; }
    static Scale X(float v) { return {AETH_SCALE_X, v}; }
    float factor(size_t n) const { return aeth_scale_factor(kind, n, x); }
};

class Context {
public:
    explicit Context(int device = 0) { check(aeth_ctx_create(device, &h_)); }
    ~Context() { aeth_ctx_destroy(h_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    aeth_ctx *get() const { return h_; }
    void sync() const { check(aeth_ctx_sync(h_)); }
    // consecutive independent Fir::filter launches alternate between two HIP queues (include/aether_hip.h)
    void set_overlap(bool enable = true) const { check(aeth_ctx_set_overlap(h_, enable ? 1 : 0)); }

private:
    aeth_ctx *h_ = nullptr;
};

class HipFft;

// level kinds of DeviceVec::levels / HipFft::levels (AETH_LEVEL_*): norm(), the reference's DB::from(norm).db()
// (10 * log10 of the amplitude: its quirk), the power in dB
enum class Level : int { Norm = AETH_LEVEL_NORM, Db = AETH_LEVEL_DB, PowerDb = AETH_LEVEL_POWER_DB };
using VecStats = struct ::aeth_vec_stats;     // the record of aeth_vec_stats, field for field

// device-resident [f32]: the levels of a vector or of a batch of spectra
class DeviceF32 {
public:
    DeviceF32(Context &ctx, size_t n) : ctx_(&ctx), n_(n)
    {
        void *p = nullptr;
        check(aeth_dev_alloc(ctx.get(), (n ? n : 1) * sizeof(float), &p));
        p_ = static_cast<float *>(p);
    }
    ~DeviceF32() { if (p_) aeth_dev_free(ctx_->get(), p_); }
    DeviceF32(const DeviceF32 &) = delete;
    DeviceF32 &operator=(const DeviceF32 &) = delete;
    DeviceF32(DeviceF32 &&o) noexcept : ctx_(o.ctx_), p_(o.p_), n_(o.n_) { o.p_ = nullptr; }
    size_t len() const { return n_; }
    float *ptr() const { return p_; }
    std::vector<float> to_host() const
    {
        std::vector<float> h(n_);
        check(aeth_download(ctx_->get(), h.data(), p_, n_ * sizeof(float)));
        return h;
    }
private:
    Context *ctx_;
    float *p_ = nullptr;
    size_t n_ = 0;
};

// device-resident [f64]: the sum and max planes of averaged spectra (aeth_vec_frame_sums, aeth_chan_exec_sums)
class DeviceF64 {
public:
    DeviceF64(Context &ctx, size_t n) : ctx_(&ctx), n_(n)
    {
        void *p = nullptr;
        check(aeth_dev_alloc(ctx.get(), (n ? n : 1) * sizeof(double), &p));
        p_ = static_cast<double *>(p);
    }
    ~DeviceF64() { if (p_) aeth_dev_free(ctx_->get(), p_); }
    DeviceF64(const DeviceF64 &) = delete;
    DeviceF64 &operator=(const DeviceF64 &) = delete;
    DeviceF64(DeviceF64 &&o) noexcept : ctx_(o.ctx_), p_(o.p_), n_(o.n_) { o.p_ = nullptr; }
    size_t len() const { return n_; }
    double *ptr() const { return p_; }
    std::vector<double> to_host() const
    {
        std::vector<double> h(n_);
        check(aeth_download(ctx_->get(), h.data(), p_, n_ * sizeof(double)));
        return h;
    }
    // what a plot draws of the plane: the level of q / count (count: the frames of a row for a sum plane, 1 for a max plane)
    DeviceF32 sum_levels(double count, Level kind = Level::Norm) const
    {
        DeviceF32 out(*ctx_, n_);
        check(aeth_vec_sum_levels(ctx_->get(), p_, n_, count, static_cast<int>(kind), out.ptr()));
        return out;
    }
private:
    Context *ctx_;
    double *p_ = nullptr;
    size_t n_ = 0;
};

// ---- trait VecOps, device-resident receiver (src/vecops.rs:39-89) ------------------
class DeviceVec {
public:
    DeviceVec(Context &ctx, size_t n) : ctx_(&ctx), n_(n), own_(true)
    {
        void *p = nullptr;
        check(aeth_dev_alloc(ctx.get(), (n ? n : 1) * sizeof(aeth_cf32), &p));
        p_ = static_cast<aeth_cf32 *>(p);
    }
    DeviceVec(Context &ctx, const std::vector<cf32> &host) : DeviceVec(ctx, host.size())
    {
        check(aeth_upload(ctx.get(), p_, host.data(), host.size() * sizeof(cf32)));
    }
    // borrowed view `self[start..stop]`
    DeviceVec(DeviceVec &parent, size_t start, size_t stop)
        : ctx_(parent.ctx_), p_(parent.p_ + start), n_(stop - start), own_(false)
    {
        if (start > stop || stop > parent.n_) throw Panic(AETH_E_LEN, "slice index out of range");
    }
    ~DeviceVec() { if (own_ && p_) aeth_dev_free(ctx_->get(), p_); }
    DeviceVec(const DeviceVec &) = delete;
    DeviceVec &operator=(const DeviceVec &) = delete;
    DeviceVec(DeviceVec &&o) noexcept : ctx_(o.ctx_), p_(o.p_), n_(o.n_), own_(o.own_) { o.p_ = nullptr; o.own_ = false; }

    size_t len() const { return n_; }
    aeth_cf32 *ptr() const { return p_; }
    Context &ctx() const { return *ctx_; }
    std::vector<cf32> to_host() const
    {
        std::vector<cf32> h(n_);
        check(aeth_download(ctx_->get(), h.data(), p_, n_ * sizeof(cf32)));
        return h;
    }

    DeviceVec &vec_scale(float s) { check(aeth_vec_scale(c(), p_, n_, s)); return *this; }
    DeviceVec &vec_mul(const DeviceVec &o) { check(aeth_vec_mul(c(), p_, n_, o.p_, o.n_)); return *this; }
    DeviceVec &vec_div(const DeviceVec &o) { check(aeth_vec_div(c(), p_, n_, o.p_, o.n_)); return *this; }
    DeviceVec &vec_conj() { check(aeth_vec_conj(c(), p_, n_)); return *this; }
    DeviceVec &vec_mirror() { check(aeth_vec_mirror(c(), p_, n_)); return *this; }
    DeviceVec &vec_clone(const DeviceVec &o) { check(aeth_vec_clone(c(), p_, n_, o.p_, o.n_)); return *this; }
    DeviceVec &vec_zero() { check(aeth_vec_zero(c(), p_, n_)); return *this; }
    DeviceVec &vec_add(const DeviceVec &o) { check(aeth_vec_add(c(), p_, n_, o.p_, o.n_)); return *this; }
    DeviceVec &vec_sub(const DeviceVec &o) { check(aeth_vec_sub(c(), p_, n_, o.p_, o.n_)); return *this; }
    // closure per element, in order (src/vecops.rs:179-182): cannot cross the FFI, so
    // the data takes a round trip through the host -- slow by design.
    DeviceVec &vec_mutate(const std::function<void(cf32 &)> &f)
    {
        auto h = to_host();
        for (auto &z : h) f(z);
        check(aeth_upload(c(), p_, h.data(), n_ * sizeof(cf32)));
        return *this;
    }
    // the reference's open item "VecStats" (README.md:90-91): one read-only pass, waits for the 64-byte record
    VecStats stats() const { VecStats st{}; check(aeth_vec_stats(c(), p_, n_, &st)); return st; }
    // the level of every sample (util/plot.rs:65,127); *this is not modified
    DeviceF32 levels(Level kind = Level::Norm) const
    {
        DeviceF32 out(*ctx_, n_);
        check(aeth_vec_levels(c(), p_, n_, static_cast<int>(kind), out.ptr(), out.len()));
        return out;
    }
    // *this as frames of `len` samples: per-column sums and maxima of q over rows of `block` frames (0: one row), added
    // in chunks of `chunk` frames (aeth_vec_frame_sums); a null plane is not computed
    void frame_sums(size_t len, size_t block, size_t chunk, DeviceF64 *sum, DeviceF64 *max) const
    {
        const DeviceF64 *any = sum ? sum : max;
        check(aeth_vec_frame_sums(c(), p_, n_, len, block, chunk, sum ? sum->ptr() : nullptr, max ? max->ptr() : nullptr, any ? any->len() : 0));
    }
    inline DeviceVec &vec_fft(Scale s);                    // fresh plan (src/vecops.rs:185-189)
    inline DeviceVec &vec_ifft(Scale s);
    inline DeviceVec &vec_rfft(HipFft &fft, Scale s);      // reused plan (src/vecops.rs:198-207)
    inline DeviceVec &vec_rifft(HipFft &fft, Scale s);

    // A chain of the element-wise methods in ONE pass over memory (aeth_vec_chain): v.fused().vec_add(a).vec_mul(b).vec_conj().run()
    class Chain {
    public:
        explicit Chain(DeviceVec &v) : v_(v) {}
        Chain &vec_scale(float s) { steps_.push_back({AETH_VEC_SCALE, nullptr, 0, s}); return *this; }
        Chain &vec_mul(const DeviceVec &o) { return bin(AETH_VEC_MUL, o); }
        Chain &vec_div(const DeviceVec &o) { return bin(AETH_VEC_DIV, o); }
        Chain &vec_conj() { steps_.push_back({AETH_VEC_CONJ, nullptr, 0, 0.f}); return *this; }
        Chain &vec_add(const DeviceVec &o) { return bin(AETH_VEC_ADD, o); }
        Chain &vec_sub(const DeviceVec &o) { return bin(AETH_VEC_SUB, o); }
        Chain &vec_clone(const DeviceVec &o) { return bin(AETH_VEC_CLONE, o); }
        Chain &vec_zero() { steps_.push_back({AETH_VEC_ZERO, nullptr, 0, 0.f}); return *this; }
        DeviceVec &run() { check(aeth_vec_chain(v_.c(), v_.ptr(), v_.len(), steps_.data(), steps_.size())); steps_.clear(); return v_; }
    private:
        Chain &bin(int op, const DeviceVec &o) { steps_.push_back({op, o.ptr(), o.len(), 0.f}); return *this; }
        DeviceVec &v_;
        std::vector<aeth_vec_step> steps_;
    };
    Chain fused() { return Chain(*this); }
private:
    aeth_ctx *c() const { return ctx_->get(); }
    Context *ctx_;
    aeth_cf32 *p_ = nullptr;
    size_t n_ = 0;
    bool own_ = false;
};

// ---- trait Fft (src/fft.rs:48-77) ---------------------------------------------------
struct Fft {
    virtual ~Fft() = default;
    virtual void fwd(const cf32 *input, size_t n_in, cf32 *output, size_t n_out, Scale s) = 0;
    virtual void bwd(const cf32 *input, size_t n_in, cf32 *output, size_t n_out, Scale s) = 0;
    virtual void ifwd(cf32 *input, size_t n, Scale s) = 0;
    virtual void ibwd(cf32 *input, size_t n, Scale s) = 0;
    virtual const cf32 *tfwd(const cf32 *input, size_t n, Scale s) = 0;
    virtual const cf32 *tbwd(const cf32 *input, size_t n, Scale s) = 0;
    virtual size_t len() const = 0;
};

// `impl Fft for HipFft`: plugs in where the reference's Cfft does (src/fft.rs:134-235).
// The exponent sign is bound to the method names HERE and nowhere else.
class HipFft final : public Fft {
public:
    static constexpr int kFwdSign = AETH_SIGN_REF_FWD;     // Cfft plans fwd with inverse=true (src/fft.rs:148)
    static constexpr int kBwdSign = AETH_SIGN_REF_BWD;
    HipFft(Context &ctx, size_t len, size_t max_batch = 1) { check(aeth_fft_create(ctx.get(), len, max_batch, &h_)); }
    static HipFft with_len(Context &ctx, size_t len) { return HipFft(ctx, len); }      // Cfft::with_len
    ~HipFft() override { aeth_fft_destroy(h_); }
    HipFft(const HipFft &) = delete;
    HipFft(HipFft &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }

    // host slices: the literal trait methods
    void fwd(const cf32 *in, size_t n_in, cf32 *out, size_t n_out, Scale s) override { check(aeth_fft_exec_host(h_, raw(in), n_in, raw(out), n_out, kFwdSign, s.kind, s.x)); }
    void bwd(const cf32 *in, size_t n_in, cf32 *out, size_t n_out, Scale s) override { check(aeth_fft_exec_host(h_, raw(in), n_in, raw(out), n_out, kBwdSign, s.kind, s.x)); }
    void ifwd(cf32 *io, size_t n, Scale s) override { check(aeth_fft_exec_host(h_, raw(io), n, raw(io), n, kFwdSign, s.kind, s.x)); }
    void ibwd(cf32 *io, size_t n, Scale s) override { check(aeth_fft_exec_host(h_, raw(io), n, raw(io), n, kBwdSign, s.kind, s.x)); }
    const cf32 *tfwd(const cf32 *in, size_t n, Scale s) override { return tmp(in, n, kFwdSign, s); }
    const cf32 *tbwd(const cf32 *in, size_t n, Scale s) override { return tmp(in, n, kBwdSign, s); }
    size_t len() const override { return aeth_fft_len(h_); }

    // device-resident frames (len(v) = batch * len()), stream-ordered
    void fwd(const DeviceVec &in, DeviceVec &out, Scale s) { exec(in, out, kFwdSign, s); }
    void bwd(const DeviceVec &in, DeviceVec &out, Scale s) { exec(in, out, kBwdSign, s); }
    void ifwd(DeviceVec &io, Scale s) { exec(io, io, kFwdSign, s); }
    void ibwd(DeviceVec &io, Scale s) { exec(io, io, kBwdSign, s); }
    // frames.vec_rfft(s).vec_mul(sig).vec_rifft(s) fused (benches/benches.rs:410-416)
    void mul_chain(DeviceVec &frames, const DeviceVec &sig, Scale s_fwd, Scale s_bwd)
    {
        size_t n = len();
        check(aeth_fft_mul_ifft(h_, frames.ptr(), frames.len(), n ? frames.len() / n : 0, sig.ptr(), sig.len(),
                                s_fwd.kind, s_fwd.x, s_bwd.kind, s_bwd.x));
    }
    // per frame: vec_rfft(s), vec_mirror() if asked for, then the level of every bin -- `waterfall` / `spectrum` of
    // util/plot.rs:46-68, :109-130 in one call; `frames` stays as it was
    DeviceF32 levels(const DeviceVec &frames, Scale s, bool mirror = false, Level kind = Level::Norm)
    {
        size_t n = len();
        DeviceF32 out(frames.ctx(), frames.len());
        check(aeth_fft_exec_levels(h_, frames.ptr(), frames.len(), n ? frames.len() / n : 0, kFwdSign, s.kind, s.x,
                                   mirror ? 1 : 0, static_cast<int>(kind), out.ptr(), out.len()));
        return out;
    }
    aeth_fft *get() const { return h_; }

private:
    void exec(const DeviceVec &in, DeviceVec &out, int sign, Scale s)
    {
        if (out.len() != in.len()) throw Panic(AETH_E_LEN, "Output and FFT must be the same length");
        size_t n = len();
        check(aeth_fft_exec(h_, in.ptr(), in.len(), out.ptr(), n ? in.len() / n : 0, sign, s.kind, s.x));
    }
    const cf32 *tmp(const cf32 *in, size_t n, int sign, Scale s)
    {
        const aeth_cf32 *view = nullptr;
        check(aeth_fft_exec_tmp_host(h_, raw(in), n, sign, s.kind, s.x, &view));
        return reinterpret_cast<const cf32 *>(view);
    }
    aeth_fft *h_ = nullptr;
};

// the reference plans per call (vecops.rs:185-189); the context keeps the plans these calls built
inline DeviceVec &DeviceVec::vec_fft(Scale s) { check(aeth_vec_fft(c(), p_, n_, HipFft::kFwdSign, s.kind, s.x)); return *this; }
inline DeviceVec &DeviceVec::vec_ifft(Scale s) { check(aeth_vec_fft(c(), p_, n_, HipFft::kBwdSign, s.kind, s.x)); return *this; }
inline DeviceVec &DeviceVec::vec_rfft(HipFft &fft, Scale s) { fft.ifwd(*this, s); return *this; }
inline DeviceVec &DeviceVec::vec_rifft(HipFft &fft, Scale s) { fft.ibwd(*this, s); return *this; }

// ---- VecOps on a host slice: the literal drop-in receiver ----------------------------
class HostVec {
public:
    HostVec(Context &ctx, cf32 *data, size_t n) : ctx_(&ctx), p_(data), n_(n) {}
    HostVec(Context &ctx, std::vector<cf32> &v) : HostVec(ctx, v.data(), v.size()) {}
    VecStats stats() const { VecStats st{}; check(aeth_host_vec_stats(c(), raw(p_), n_, &st)); return st; }
    HostVec &vec_scale(float s) { check(aeth_host_vec_scale(c(), raw(p_), n_, s)); return *this; }
    HostVec &vec_mul(const std::vector<cf32> &o) { check(aeth_host_vec_mul(c(), raw(p_), n_, raw(o.data()), o.size())); return *this; }
    HostVec &vec_div(const std::vector<cf32> &o) { check(aeth_host_vec_div(c(), raw(p_), n_, raw(o.data()), o.size())); return *this; }
    HostVec &vec_conj() { check(aeth_host_vec_conj(c(), raw(p_), n_)); return *this; }
    HostVec &vec_mirror() { check(aeth_host_vec_mirror(c(), raw(p_), n_)); return *this; }
    HostVec &vec_clone(const std::vector<cf32> &o) { check(aeth_host_vec_clone(c(), raw(p_), n_, raw(o.data()), o.size())); return *this; }
    HostVec &vec_zero() { check(aeth_host_vec_zero(c(), raw(p_), n_)); return *this; }
    HostVec &vec_add(const std::vector<cf32> &o) { check(aeth_host_vec_add(c(), raw(p_), n_, raw(o.data()), o.size())); return *this; }
    HostVec &vec_sub(const std::vector<cf32> &o) { check(aeth_host_vec_sub(c(), raw(p_), n_, raw(o.data()), o.size())); return *this; }
    HostVec &vec_mutate(const std::function<void(cf32 &)> &f) { for (size_t i = 0; i < n_; i++) f(p_[i]); return *this; }
    HostVec &vec_fft(Scale s) { check(aeth_host_vec_fft(c(), raw(p_), n_, HipFft::kFwdSign, s.kind, s.x)); return *this; }
    HostVec &vec_ifft(Scale s) { check(aeth_host_vec_fft(c(), raw(p_), n_, HipFft::kBwdSign, s.kind, s.x)); return *this; }
    HostVec &vec_rfft(Fft &fft, Scale s) { fft.ifwd(p_, n_, s); return *this; }
    HostVec &vec_rifft(Fft &fft, Scale s) { fft.ibwd(p_, n_, s); return *this; }

private:
    aeth_ctx *c() const { return ctx_->get(); }
    Context *ctx_;
    cf32 *p_;
    size_t n_;
};

// ---- pinned host buffers: pool::Pool<T> / Elem<T> (src/pool.rs:43-221) ------------------------------
// Pool::make(ctx, n_samples, initial_len): elements are pinned buffers of n_samples cf32 each (the maker), optionally
// zeroed on return (the resetter).  take() is empty (null Elem) when the pool is; take_or_make() grows it.  An Elem
// derefs into its samples and returns itself to the pool when it goes out of scope (Elem::drop, :196-208).
class Pool {
public:
    class Elem {
    public:
        Elem() = default;
        Elem(aeth_pool *pool, cf32 *p, size_t n) : pool_(pool), p_(p), n_(n) {}
        Elem(Elem &&o) noexcept : pool_(o.pool_), p_(o.p_), n_(o.n_) { o.p_ = nullptr; }
        Elem &operator=(Elem &&o) noexcept { reset(); pool_ = o.pool_; p_ = o.p_; n_ = o.n_; o.p_ = nullptr; return *this; }
        Elem(const Elem &) = delete;
        Elem &operator=(const Elem &) = delete;
        ~Elem() { reset(); }
        explicit operator bool() const { return p_ != nullptr; }          // Option<Elem<T>>::is_some()
        cf32 *data() { return p_; }
        const cf32 *data() const { return p_; }
        size_t size() const { return n_; }
        cf32 &operator[](size_t i) { return p_[i]; }
        void reset() { if (p_) { aeth_pool_give_back(pool_, p_); p_ = nullptr; } }
    private:
        aeth_pool *pool_ = nullptr;
        cf32 *p_ = nullptr;
        size_t n_ = 0;
    };
    static Pool make(Context &ctx, size_t n_samples, size_t initial_len, bool zero_on_return = false)
    {
        Pool p; p.n_ = n_samples;
        check(aeth_pool_create(ctx.get(), n_samples * sizeof(cf32), initial_len, zero_on_return ? AETH_POOL_ZERO_ON_RETURN : 0, &p.h_));
        return p;
    }
    Pool(Pool &&o) noexcept : h_(o.h_), n_(o.n_) { o.h_ = nullptr; }
    Pool(const Pool &) = delete;
    Pool &operator=(const Pool &) = delete;
    ~Pool() { if (h_) aeth_pool_destroy(h_); }
    Elem take() { void *b = nullptr; check(aeth_pool_take(h_, &b)); return Elem(h_, static_cast<cf32 *>(b), b ? n_ : 0); }
    Elem take_or_make() { void *b = nullptr; check(aeth_pool_take_or_make(h_, &b)); return Elem(h_, static_cast<cf32 *>(b), n_); }
    size_t len() const { return aeth_pool_len(h_); }
    size_t cap() const { return aeth_pool_cap(h_); }
    bool is_empty() const { return len() == 0; }
private:
    Pool() = default;
    aeth_pool *h_ = nullptr;
    size_t n_ = 0;
};

// ---- FIR (src/fir.rs:3-22 has the struct, not the filter) ------------------------------
class Fir {
public:
    Fir(Context &ctx, const std::vector<cf32> &taps, size_t fft_len = 2048) { check(aeth_fir_create(ctx.get(), raw(taps.data()), taps.size(), fft_len, &h_)); }
    ~Fir() { aeth_fir_destroy(h_); }
    Fir(const Fir &) = delete;
    size_t hop() const { return aeth_fir_hop(h_); }
    void filter(const DeviceVec &x, DeviceVec &y, const DeviceVec *hist = nullptr)
    {
        if (y.len() != x.len()) throw Panic(AETH_E_LEN, "Vectors must have same length");
        check(aeth_fir_exec(h_, hist ? hist->ptr() : nullptr, x.ptr(), x.len(), y.ptr()));
    }
    void filter(const std::vector<cf32> &x, std::vector<cf32> &y)
    {
        y.resize(x.size());
        check(aeth_fir_exec_host(h_, nullptr, raw(x.data()), x.size(), raw(y.data())));
    }
    // host-resident stream through the upload | kernel | download pipeline (src/pipeline.rs counterpart); with report =
    // true the reference pipeline's per-stage lines (pipeline.rs:101-108) go to stdout
    aeth_pipe_util filter_stream(const std::vector<cf32> &x, std::vector<cf32> &y, size_t chunk = 0, bool report = false)
    {
        y.resize(x.size());
        aeth_pipe_util u{};
        check(aeth_fir_stream_host_util(h_, raw(x.data()), x.size(), raw(y.data()), chunk, &u));
        if (report) print_report(u);
        return u;
    }
    // the same on raw slices: memory inside a pinned Pool element (or a registered range) is copied from / to directly
    aeth_pipe_util filter_stream(const cf32 *x, size_t n, cf32 *y, size_t chunk = 0, bool report = false)
    {
        aeth_pipe_util u{};
        check(aeth_fir_stream_host_util(h_, raw(x), n, raw(y), chunk, &u));
        if (report) print_report(u);
        return u;
    }
    static void print_report(const aeth_pipe_util &u)
    {
        if (!(u.seconds > 0)) return;
        const char *names[5] = {"copy-in", "upload", "kernel", "download", "copy-out"};
        const double act[5] = {u.active_copy_in, u.active_upload, u.active_kernel, u.active_download, u.active_copy_out};
        for (int s = 0; s < 5; s++) {
            if ((s == 0 || s == 4) && act[s] == 0) continue;       // a side that was copied directly has no host stage
            std::printf("Stage: %-15s : Processed %llu in %3.3fs (%9.2f/s); Utilisation: %3.2f%%\n", names[s],
                        (unsigned long long)u.chunks, u.seconds, u.chunks / u.seconds, act[s] / u.seconds * 100.0);
        }
    }
    // the filter followed by sampling::downsample (sampling.rs:28-42) in one pass: y[i] = fir(x)[i * (x.len / y.len)]
    void filter_decim(const DeviceVec &x, DeviceVec &y, const DeviceVec *hist = nullptr)
    {
        check(aeth_fir_exec_decim(h_, hist ? hist->ptr() : nullptr, x.ptr(), x.len(), y.ptr(), y.len()));
    }

    aeth_fir *get() const { return h_; }

private:
    aeth_fir *h_ = nullptr;
};

// ---- streaming correlator (the reference's open item "Add Correlation by Freq. Domain Convolution", README.md:95) ----
// c[j] = sum_k conj(ref[M-1-k]) * x[j-k]: an occurrence of ref that starts at p peaks at j = p + M - 1
using CorrPeak = struct ::aeth_corr_peak;     // the record of aeth_corr_search, field for field
class Corr {
public:
    Corr(Context &ctx, const std::vector<cf32> &ref, size_t fft_len = 2048) { check(aeth_corr_create(ctx.get(), raw(ref.data()), ref.size(), fft_len, &h_)); }
    ~Corr() { aeth_corr_destroy(h_); }
    Corr(const Corr &) = delete;
    Corr &operator=(const Corr &) = delete;
    size_t nref() const { return aeth_corr_nref(h_); }
    size_t fft_len() const { return aeth_corr_fft_len(h_); }
    size_t hop() const { return aeth_corr_hop(h_); }
    size_t n_blocks(size_t n) const { return (n + hop() - 1) / hop(); }
    void correlate(const DeviceVec &x, DeviceVec &c, const DeviceVec *hist = nullptr)
    {
        if (c.len() != x.len()) throw Panic(AETH_E_LEN, "Vectors must have same length");
        check(aeth_corr_exec(h_, hist ? hist->ptr() : nullptr, x.ptr(), x.len(), c.ptr()));
    }
    // the level of every c[j] in one pass (c is never written)
    DeviceF32 levels(const DeviceVec &x, int kind = AETH_LEVEL_NORM, const DeviceVec *hist = nullptr)
    {
        DeviceF32 out(x.ctx(), x.len());
        check(aeth_corr_exec_levels(h_, hist ? hist->ptr() : nullptr, x.ptr(), x.len(), kind, out.ptr(), out.len()));
        return out;
    }
    // the best peak of the stream in one pass; `blocks` (optional) receives one record per hop() outputs
    CorrPeak search(const DeviceVec &x, std::vector<CorrPeak> *blocks = nullptr, const DeviceVec *hist = nullptr)
    {
        CorrPeak best{};
        const aeth_cf32 *hp = hist ? hist->ptr() : nullptr;
        if (!blocks) { check(aeth_corr_search(h_, hp, x.ptr(), x.len(), nullptr, 0, &best)); return best; }
        const size_t nb = n_blocks(x.len());
        void *dev = nullptr;
        check(aeth_dev_alloc(x.ctx().get(), (nb ? nb : 1) * sizeof(CorrPeak), &dev));
        int rc = aeth_corr_search(h_, hp, x.ptr(), x.len(), static_cast<CorrPeak *>(dev), nb, &best);
        blocks->resize(nb);
        if (rc == AETH_OK && nb) rc = aeth_download(x.ctx().get(), blocks->data(), dev, nb * sizeof(CorrPeak));
        aeth_dev_free(x.ctx().get(), dev);
        check(rc);
        return best;
    }
    aeth_corr *get() const { return h_; }

private:
    aeth_corr *h_ = nullptr;
};

// ---- polyphase analysis filter bank (no body in the reference: `waterfall`, src/util/plot.rs:46-68, frames with
// chunks_mut(fft_len)) ---------------------------------------------------------------------------------------------------
// Weight proto.size() = P * channels samples, fold them modulo `channels`, transform, advance by `hop`.
class Channelizer {
public:
    Channelizer(Context &ctx, const std::vector<float> &proto, size_t channels, size_t hop = 0, int phase = AETH_CHAN_PHASE_FRAME,
                size_t max_frames = 0)
    {
        check(aeth_chan_create(ctx.get(), proto.data(), proto.size(), channels, hop ? hop : channels, phase, max_frames, &h_));
    }
    ~Channelizer() { aeth_chan_destroy(h_); }
    Channelizer(const Channelizer &) = delete;
    Channelizer &operator=(const Channelizer &) = delete;
    // RECT / HANN / HAMMING / SINC_HAMMING (AETH_CHAN_PROTO_*), computed on the host
    static std::vector<float> prototype(int kind, size_t channels, size_t taps_per_channel)
    {
        std::vector<float> w(channels * taps_per_channel);
        check(aeth_chan_prototype(kind, channels, taps_per_channel, w.data()));
        return w;
    }
    size_t channels() const { return aeth_chan_channels(h_); }
    size_t ntaps() const { return aeth_chan_ntaps(h_); }
    size_t hop() const { return aeth_chan_hop(h_); }
    int phase() const { return aeth_chan_phase(h_); }
    size_t tile() const { return aeth_chan_tile(h_); }
    std::string route() const { return aeth_chan_route(h_); }
    size_t frames(size_t n) const { return n / hop(); }
    // `hist`: the ntaps - hop samples in front of x (null: zeros); first_frame: the global number of the call's first frame
    void fold(const DeviceVec &x, DeviceVec &out, const DeviceVec *hist = nullptr, uint64_t first_frame = 0)
    {
        check(aeth_chan_fold(h_, hist ? hist->ptr() : nullptr, x.ptr(), x.len(), first_frame, out.ptr(), out.len()));
    }
    void exec(const DeviceVec &x, DeviceVec &out, Scale s, const DeviceVec *hist = nullptr, uint64_t first_frame = 0,
              int sign = AETH_SIGN_REF_FWD)
    {
        check(aeth_chan_exec(h_, hist ? hist->ptr() : nullptr, x.ptr(), x.len(), first_frame, sign, s.kind, s.x, out.ptr(), out.len()));
    }
    DeviceF32 levels(const DeviceVec &x, Scale s, bool mirror = false, int kind = AETH_LEVEL_NORM, const DeviceVec *hist = nullptr,
                     uint64_t first_frame = 0, int sign = AETH_SIGN_REF_FWD)
    {
        DeviceF32 out(x.ctx(), frames(x.len()) * channels());
        check(aeth_chan_exec_levels(h_, hist ? hist->ptr() : nullptr, x.ptr(), x.len(), first_frame, sign, s.kind, s.x, mirror ? 1 : 0,
                                    kind, out.ptr(), out.len()));
        return out;
    }
    // averaged spectra: per-bin sums and maxima of q over rows of `block` frames (0: one row); a null plane is not computed
    size_t sums_chunk() const { return aeth_chan_sums_chunk(h_); }
    bool sums_fused() const { return aeth_chan_sums_fused(h_) != 0; }
    void sums(const DeviceVec &x, Scale s, DeviceF64 *sum, DeviceF64 *max, size_t block = 0, bool mirror = false, const DeviceVec *hist = nullptr,
              uint64_t first_frame = 0, int sign = AETH_SIGN_REF_FWD, bool general = false)
    {
        const DeviceF64 *any = sum ? sum : max;
        check(aeth_chan_exec_sums(h_, hist ? hist->ptr() : nullptr, x.ptr(), x.len(), first_frame, sign, s.kind, s.x, mirror ? 1 : 0, block,
                                  general ? AETH_SUMS_GENERAL : 0, sum ? sum->ptr() : nullptr, max ? max->ptr() : nullptr, any ? any->len() : 0));
    }
    aeth_chan *get() const { return h_; }

private:
    aeth_chan *h_ = nullptr;
};

// ---- polyphase synthesis filter bank (no body in the reference: src/util/plot.rs:46-68 only takes a stream apart) ------
// The transpose of Channelizer: every frame's `channels` time samples are extended periodically to proto.size(), weighted
// and overlap-added at `hop`; the output is the reconstruction delayed by proto.size() - hop samples.
class Synthesizer {
public:
    Synthesizer(Context &ctx, const std::vector<float> &proto, size_t channels, size_t hop = 0, int phase = AETH_CHAN_PHASE_FRAME,
                size_t max_frames = 0)
    {
        check(aeth_synth_create(ctx.get(), proto.data(), proto.size(), channels, hop ? hop : channels, phase, max_frames, &h_));
    }
    ~Synthesizer() { aeth_synth_destroy(h_); }
    Synthesizer(const Synthesizer &) = delete;
    Synthesizer &operator=(const Synthesizer &) = delete;
    // the synthesis window that inverts a windowed, overlapped transform of w.size() points at `hop`, computed on the host
    static std::vector<float> dual_window(const std::vector<float> &w, size_t hop)
    {
        std::vector<float> g(w.size());
        check(aeth_synth_dual_window(w.data(), w.size(), hop, g.data()));
        return g;
    }
    size_t channels() const { return aeth_synth_channels(h_); }
    size_t ntaps() const { return aeth_synth_ntaps(h_); }
    size_t hop() const { return aeth_synth_hop(h_); }
    int phase() const { return aeth_synth_phase(h_); }
    size_t tile() const { return aeth_synth_tile(h_); }
    size_t history() const { return aeth_synth_history(h_); }
    std::string route() const { return aeth_synth_route(h_); }
    size_t samples(size_t n_in) const { return n_in / channels() * hop(); }
    // `hist`: the history() frames in front of `frames` (null: zeros); first_frame: the global number of the call's first frame
    void unfold(const DeviceVec &frames, DeviceVec &out, const DeviceVec *hist = nullptr, uint64_t first_frame = 0)
    {
        check(aeth_synth_unfold(h_, hist ? hist->ptr() : nullptr, frames.ptr(), frames.len(), first_frame, out.ptr(), out.len()));
    }
    // `spec` and `hist` hold spectra: the transform of every frame, then the overlap-add
    void exec(const DeviceVec &spec, DeviceVec &out, Scale s, const DeviceVec *hist = nullptr, uint64_t first_frame = 0,
              int sign = AETH_SIGN_REF_BWD)
    {
        check(aeth_synth_exec(h_, hist ? hist->ptr() : nullptr, spec.ptr(), spec.len(), first_frame, sign, s.kind, s.x, out.ptr(),
                              out.len()));
    }
    aeth_synth *get() const { return h_; }

private:
    aeth_synth *h_ = nullptr;
};

// ---- polyphase rational resampler (no body in the reference: src/sampling.rs:7-62 interpolates linearly and picks) -----
// Upsample by `up`, filter with the real taps, keep every `down`-th sample, in one pass: a call over n = B * down samples
// makes B * up outputs; the previous history() input samples make the chunks of a stream concatenate exactly.
class Resampler {
public:
    Resampler(Context &ctx, const std::vector<float> &taps, size_t up, size_t down)
    {
        check(aeth_resamp_create(ctx.get(), taps.data(), taps.size(), up, down, &h_));
    }
    ~Resampler() { aeth_resamp_destroy(h_); }
    Resampler(const Resampler &) = delete;
    Resampler &operator=(const Resampler &) = delete;
    // up * taps_per_phase taps of the low-pass at 1 / (2 max(up, down)) cycles per upsampled sample, summing to `up`
    static std::vector<float> prototype(size_t up, size_t down, size_t taps_per_phase)
    {
        const size_t L = up * taps_per_phase;
        std::vector<float> g(L > 0 ? L : 1);
        check(aeth_resamp_prototype(up, down, taps_per_phase, g.data()));
        return g;
    }
    size_t up() const { return aeth_resamp_up(h_); }
    size_t down() const { return aeth_resamp_down(h_); }
    size_t ntaps() const { return aeth_resamp_ntaps(h_); }
    size_t history() const { return aeth_resamp_history(h_); }
    size_t tile() const { return aeth_resamp_tile(h_); }
    std::string route() const { return aeth_resamp_route(h_); }
    size_t out_count(size_t n_in) const { return aeth_resamp_out_count(h_, n_in); }
    // `hist`: the history() samples in front of `x` (null: zeros)
    void exec(const DeviceVec &x, DeviceVec &out, const DeviceVec *hist = nullptr)
    {
        check(aeth_resamp_exec(h_, hist ? hist->ptr() : nullptr, x.ptr(), x.len(), out.ptr(), out.len()));
    }
    aeth_resamp *get() const { return h_; }

private:
    aeth_resamp *h_ = nullptr;
};

// ---- arbitrary-ratio resampler (no body in the reference: src/sampling.rs:7-62 interpolates linearly and picks) -------
// A bank of 2^log2_phases phases whose taps are interpolated linearly between neighbours, behind an unsigned Q32.32 time
// word: output m of a call stands at phase + m * step input samples.  advance() gives a call's output count and the next
// call's phase; with the previous history() input samples the chunks of a stream concatenate exactly.
class ArbResampler {
public:
    ArbResampler(Context &ctx, const std::vector<float> &taps, size_t log2_phases)
    {
        check(aeth_arb_create(ctx.get(), taps.data(), taps.size(), log2_phases, &h_));
    }
    ~ArbResampler() { aeth_arb_destroy(h_); }
    ArbResampler(const ArbResampler &) = delete;
    ArbResampler &operator=(const ArbResampler &) = delete;
    // the Q32.32 word of `ratio` input samples per output sample, truncated
    static uint64_t step_word(double ratio) { return (uint64_t)(ratio * 4294967296.0); }
    // outputs of a call over n input samples from `phase`; *next_phase: the phase of the call behind it
    static size_t advance(uint64_t step, uint64_t phase, size_t n, uint64_t *next_phase)
    {
        size_t count = 0;
        check(aeth_arb_advance(step, phase, n, &count, next_phase));
        return count;
    }
    size_t phases() const { return aeth_arb_phases(h_); }
    size_t ntaps() const { return aeth_arb_ntaps(h_); }
    size_t history() const { return aeth_arb_history(h_); }
    size_t tile(uint64_t step) const { return aeth_arb_tile(h_, step); }
    std::string route(uint64_t step) const { return aeth_arb_route(h_, step); }
    // `hist`: the history() samples in front of `x` (null: zeros); out.len() must be advance(step, phase, x.len())
    void exec(const DeviceVec &x, uint64_t step, uint64_t phase, DeviceVec &out, const DeviceVec *hist = nullptr)
    {
        check(aeth_arb_exec(h_, hist ? hist->ptr() : nullptr, x.ptr(), x.len(), step, phase, out.ptr(), out.len()));
    }
    aeth_arb *get() const { return h_; }

private:
    aeth_arb *h_ = nullptr;
};

// ---- numerically controlled oscillator (no body in the reference: it has no frequency shift, tone or chirp) ----------
// Three 64-bit words, fractions of a turn scaled by 2^64: w(n) = phase + n * step + n (n - 1) / 2 * rate modulo 2^64, exact
// at every stream position.  mix multiplies by the phasor of w(position + i), tone writes amp times it; both advance
// `position` by the samples they handled, so the chunks of a stream concatenate bit for bit.
class Nco {
public:
    // freq in cycles per sample, phase in cycles, rate in cycles per sample per sample
    explicit Nco(Context &ctx, double freq = 0.0, double phase = 0.0, double rate = 0.0, uint64_t position = 0)
        : ctx_(ctx.get()), w_{aeth_nco_word(phase), aeth_nco_word(freq), aeth_nco_word(rate)}, position_(position) {}
    static Nco from_words(Context &ctx, uint64_t phase, uint64_t step, uint64_t rate, uint64_t position = 0)
    {
        Nco o(ctx);
        o.w_ = aeth_nco_words{phase, step, rate};
        o.position_ = position;
        return o;
    }
    static uint64_t word(double cycles) { return aeth_nco_word(cycles); }
    static uint64_t word_at(const aeth_nco_words &w, uint64_t n) { return aeth_nco_word_at(&w, n); }
    static aeth_cf32 phasor(uint64_t word)
    {
        aeth_cf32 out;
        check(aeth_nco_phasor(word, &out));
        return out;
    }
    const aeth_nco_words &words() const { return w_; }
    uint64_t position() const { return position_; }
    void seek(uint64_t position) { position_ = position; }
    // out may be x itself (in place)
    void mix(const DeviceVec &x, DeviceVec &out)
    {
        if (x.len() != out.len()) throw Panic(AETH_E_LEN, "Nco::mix: the output's length is not the input's");
        check(aeth_nco_mix(ctx_, &w_, position_, x.ptr(), out.ptr(), x.len()));
        position_ += x.len();
    }
    void mix(DeviceVec &x) { mix(x, x); }
    void tone(DeviceVec &out, float amp = 1.0f)
    {
        check(aeth_nco_tone(ctx_, &w_, position_, amp, out.ptr(), out.len()));
        position_ += out.len();
    }

private:
    aeth_ctx *ctx_;
    aeth_nco_words w_;
    uint64_t position_;
};

// ---- synchronisation estimators (no body in the reference: it estimates no offset) -----------------------------------
// line sums a non-linearity of the samples against the oscillator's phasor (AETH_SYNC_SQUARE with step =
// aeth_nco_word(-1 / sps): symbol timing; AETH_SYNC_POW<M> without words: the M-th power carrier phase), lag sums
// pw_M(x[i]) * conj(pw_M(x[i - lag])) (carrier frequency).  f64 sums in a fixed order: one record per `block` samples at
// rec_dev (device memory of ceil(n / block) records, or null) and the total, for which the call waits.
struct Sync {
    static size_t chunk() { return aeth_sync_chunk(); }
    static aeth_sync_record line(Context &ctx, int kind, const DeviceVec &x, const aeth_nco_words *words = nullptr,
                                 uint64_t position = 0, size_t block = 0, aeth_sync_record *rec_dev = nullptr)
    {
        aeth_sync_record total;
        check(aeth_sync_line(ctx.get(), kind, words, position, x.ptr(), x.len(), block, rec_dev, &total));
        return total;
    }
    // hist: the `lag` samples in front of x (null: the terms i < lag do not exist)
    static aeth_sync_record lag(Context &ctx, int power, size_t lag, const DeviceVec &x, const DeviceVec *hist = nullptr,
                                size_t block = 0, aeth_sync_record *rec_dev = nullptr)
    {
        aeth_sync_record total;
        check(aeth_sync_lag(ctx.get(), power, lag, hist ? hist->ptr() : nullptr, x.ptr(), x.len(), block, rec_dev, &total));
        return total;
    }
    static double turns(const aeth_sync_record &r) { return aeth_sync_turns(&r); }
    static uint64_t freq_step(const aeth_sync_record &r, int power, size_t lag) { return aeth_sync_freq_step(&r, power, lag); }
    static uint64_t timing_phase(const aeth_sync_record &r, double sps) { return aeth_sync_timing_phase(&r, sps); }
};

// ---- moving-window detectors (no body in the reference) --------------------------------------------------------------
// For every sample the sum of the last `window` lag terms x[j] * conj(x[j - lag]) (P) and powers (R), and the metric
// |P|^2 / (R(i) R(i - lag)) (AETH_MOV_LAG) or the moving mean power (AETH_MOV_POWER, lag 0).  exec writes the planes that
// are not null and does not wait; search keeps one record per `block` samples at peaks_dev (or null) and returns the
// record over the whole call, for which it waits.  hist: the history() samples in front of x (null: zeros).
struct Mov {
    static size_t history(int kind, size_t window, size_t lag) { return aeth_mov_history(kind, window, lag); }
    static size_t grid(int kind, size_t window) { return aeth_mov_grid(kind, window); }
    static void exec(Context &ctx, int kind, size_t window, size_t lag, const DeviceVec &x, aeth_cf32 *p_dev, float *r_dev, float *m_dev,
                     const DeviceVec *hist = nullptr)
    {
        check(aeth_mov_exec(ctx.get(), kind, window, lag, hist ? hist->ptr() : nullptr, x.ptr(), x.len(), p_dev, r_dev, m_dev));
    }
    static aeth_mov_peak search(Context &ctx, int kind, size_t window, size_t lag, double r_min, double threshold, const DeviceVec &x,
                                const DeviceVec *hist = nullptr, size_t block = 0, aeth_mov_peak *peaks_dev = nullptr)
    {
        aeth_mov_peak best;
        check(aeth_mov_search(ctx.get(), kind, window, lag, r_min, threshold, hist ? hist->ptr() : nullptr, x.ptr(), x.len(), block,
                              peaks_dev, &best));
        return best;
    }
    static uint64_t freq_step(const aeth_mov_peak &p, size_t lag) { return aeth_mov_freq_step(&p, lag); }
};

// ---- convolutional codes (no body in the reference: it has no forward error correction) ------------------------------
// A rate 1/n code of constraint length k = 3 .. 7, polynomials in the octal convention with the current bit at the MSB
// (K = 7: 0171, 0133).  Device pointers in and out; bits are one byte each, soft values int8_t (positive: bit 0 likelier,
// 0: erasure).  decode is a causal system with a delay of traceback() steps: out[o] is the decision for step o - traceback().
class ConvCode {
public:
    ConvCode(Context &ctx, uint32_t k, const std::vector<uint32_t> &polys, size_t block = 512, size_t warmup = 64, size_t traceback = 64)
    {
        if (polys.size() > 4) throw Panic(AETH_E_ARG, "ConvCode: at most 4 polynomials");
        aeth_cc_code code{k, (uint32_t)polys.size(), {0, 0, 0, 0}};
        for (size_t i = 0; i < polys.size(); i++) code.poly[i] = polys[i];
        check(aeth_cc_create(ctx.get(), &code, block, warmup, traceback, &h_));
    }
    ~ConvCode() { aeth_cc_destroy(h_); }
    ConvCode(const ConvCode &) = delete;
    ConvCode &operator=(const ConvCode &) = delete;
    size_t k() const { return aeth_cc_k(h_); }
    size_t n() const { return aeth_cc_n(h_); }
    size_t block() const { return aeth_cc_block(h_); }
    size_t warmup() const { return aeth_cc_warmup(h_); }
    size_t traceback() const { return aeth_cc_traceback(h_); }
    // warmup + traceback: the steps of soft values a continued decode wants in front
    size_t history() const { return aeth_cc_history(h_); }
    // `hist_dev`: the k - 1 bits before bits_dev[0] (null: zeros); coded_dev holds nbits * n bytes
    void encode(const uint8_t *bits_dev, size_t nbits, uint8_t *coded_dev, size_t ncoded, const uint8_t *hist_dev = nullptr)
    {
        check(aeth_cc_encode(h_, hist_dev, bits_dev, nbits, coded_dev, ncoded));
    }
    // `hist_dev`: the history() * n soft values before soft_dev[0] (null: erasures); bits_dev holds nsoft / n bytes
    void decode(const int8_t *soft_dev, size_t nsoft, uint8_t *bits_dev, size_t nbits, const int8_t *hist_dev = nullptr)
    {
        check(aeth_cc_decode(h_, hist_dev, soft_dev, nsoft, bits_dev, nbits));
    }
    aeth_cc *get() const { return h_; }

private:
    aeth_cc *h_ = nullptr;
};

// ---- rate matching (no body in the reference) --------------------------------------------------------------------------
// A periodic byte map: out[q r_out + i] = in[q r_in + map[i]], or `fill` where map[i] is -1.  Puncturing, depuncturing to
// erasures, block interleaving and any chain of them are this one gather.  The table builders are host-only integer
// arithmetic; device pointers in and out, bytes of any meaning (uint8_t bits, int8_t soft values).
class Remap {
public:
    Remap(Context &ctx, std::vector<int32_t> map, size_t r_in) : ctx_(&ctx), map_(std::move(map)), r_in_(r_in)
    {
        check(aeth_remap_create(ctx.get(), map_.data(), map_.size(), r_in_, &h_));
    }
    ~Remap() { aeth_remap_destroy(h_); }
    Remap(const Remap &) = delete;
    Remap &operator=(const Remap &) = delete;
    Remap(Remap &&o) noexcept : ctx_(o.ctx_), map_(std::move(o.map_)), r_in_(o.r_in_), h_(o.h_) { o.h_ = nullptr; }
    // keep[i] & 1: coded bit i of a period of keep.size() is sent
    static Remap puncture(Context &ctx, const std::vector<uint8_t> &keep)
    {
        std::vector<int32_t> map(keep.empty() ? 1 : keep.size());
        size_t r_out = 0;
        check(aeth_remap_puncture(keep.data(), keep.size(), map.data(), map.size(), &r_out));
        map.resize(r_out);
        return Remap(ctx, std::move(map), keep.size());
    }
    // written row by row, read column by column
    static Remap rows_cols(Context &ctx, size_t rows, size_t cols)
    {
        std::vector<int32_t> map(std::min<size_t>(std::max<size_t>(rows * cols, 1), (size_t)1 << 20));
        check(aeth_remap_rows_cols(rows, cols, map.data()));
        return Remap(ctx, std::move(map), rows * cols);
    }
    // the interleaver of 802.11a 17.3.5.6 over n_cbps coded bits at n_bpsc bits per carrier
    static Remap bicm16(Context &ctx, size_t n_cbps, size_t n_bpsc)
    {
        std::vector<int32_t> map(std::min<size_t>(std::max<size_t>(n_cbps, 1), (size_t)1 << 20));
        check(aeth_remap_bicm16(n_cbps, n_bpsc, map.data()));
        return Remap(ctx, std::move(map), n_cbps);
    }
    // the depuncturer of a puncturer, the deinterleaver of an interleaver, the first copy of a repetition
    Remap inverse() const
    {
        std::vector<int32_t> inv(r_in_);
        check(aeth_remap_invert(map_.data(), map_.size(), r_in_, inv.data()));
        return Remap(*ctx_, std::move(inv), map_.size());
    }
    // `other` applied to the output of this map, as one map
    Remap then(const Remap &other) const
    {
        std::vector<int32_t> map((size_t)1 << 20);
        size_t r_out = 0, r_in = 0;
        check(aeth_remap_compose(map_.data(), map_.size(), r_in_, other.map_.data(), other.map_.size(), other.r_in_, map.data(), map.size(),
                                 &r_out, &r_in));
        map.resize(r_out);
        return Remap(*ctx_, std::move(map), r_in);
    }
    size_t in_period() const { return aeth_remap_in_period(h_); }
    size_t out_period() const { return aeth_remap_out_period(h_); }
    // the input bytes a call that writes n_out bytes reads
    size_t in_count(size_t n_out) const { return aeth_remap_in_count(h_, n_out); }
    int route() const { return aeth_remap_route(h_); }          // AETH_REMAP_ROUTE_TILE or AETH_REMAP_ROUTE_GATHER
    size_t tile() const { return aeth_remap_tile(h_); }         // periods per tile; 0 on the gather route
    void exec(const void *in_dev, size_t n_in, void *out_dev, size_t n_out, uint8_t fill = 0)
    {
        check(aeth_remap_exec(h_, in_dev, n_in, out_dev, n_out, fill));
    }
    const std::vector<int32_t> &map() const { return map_; }
    aeth_remap *get() const { return h_; }

private:
    Context *ctx_;
    std::vector<int32_t> map_;
    size_t r_in_;
    aeth_remap *h_ = nullptr;
};

// ---- frame checks: CRC attach and check over bit frames, bit packing (no body in the reference) ----------------------
// A CRC of width r <= 64: poly holds the generator's low r coefficients, bits are one byte per bit, first bit first, and
// the check bits go out highest coefficient first.  Frames are contiguous and of one length.  registers is the streaming
// primitive (no xorout; a frame cut anywhere continues from the states of the call before), attach appends the r check
// bits, check forms diff = received ^ computed ^ mask per frame, strips the payload and folds {n_bad, first_bad}.  Device
// pointers in and out, ordered on the context's stream.
class Crc {
public:
    Crc(Context &ctx, uint32_t r, uint64_t poly, uint64_t init = 0, uint64_t xorout = 0)
    {
        check(aeth_crc_create(ctx.get(), r, poly, init, xorout, &h_));
    }
    // a catalogue name: "crc-24/lte-a", "crc-32", ... (aeth_crc_named)
    static Crc named(Context &ctx, const char *name)
    {
        uint32_t r = 0;
        uint64_t poly = 0, init = 0, xorout = 0;
        check(aeth_crc_named(name, &r, &poly, &init, &xorout));
        return Crc(ctx, r, poly, init, xorout);
    }
    ~Crc() { aeth_crc_destroy(h_); }
    Crc(const Crc &) = delete;
    Crc &operator=(const Crc &) = delete;
    Crc(Crc &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    uint32_t width() const { return aeth_crc_width(h_); }
    uint64_t poly() const { return aeth_crc_poly(h_); }
    uint64_t init() const { return aeth_crc_init(h_); }
    uint64_t xorout() const { return aeth_crc_xorout(h_); }
    // the register (before xorout) any frame followed by its own check bits leaves
    uint64_t residue() const { return aeth_crc_residue(h_); }
    int route(size_t L, size_t F = 1) const { return aeth_crc_route(h_, L, F); }       // AETH_CRC_ROUTE_FRAMES or AETH_CRC_ROUTE_LONG
    size_t route_frame_bits() const { return aeth_crc_route_frame_bits(h_); }
    size_t frames_per_workgroup(size_t frame_bytes) const { return aeth_crc_frames_per_workgroup(h_, frame_bytes); }
    // state_in_dev may be null: every frame starts from init
    void registers(const uint8_t *bits_dev, size_t L, size_t F, const uint64_t *state_in_dev, uint64_t *state_out_dev)
    {
        check(aeth_crc_exec(h_, bits_dev, L, F, state_in_dev, state_out_dev));
    }
    void attach(const uint8_t *in_dev, size_t L, size_t F, uint8_t *out_dev) { check(aeth_crc_attach(h_, in_dev, L, F, out_dev)); }
    // any of the three outputs may be null, not all
    void check_frames(const uint8_t *in_dev, size_t L, size_t F, uint64_t mask, uint64_t *diff_dev, uint8_t *payload_dev,
                      aeth_crc_summary *summary_dev)
    {
        check(aeth_crc_check(h_, in_dev, L, F, mask, diff_dev, payload_dev, summary_dev));
    }
    // the definition on host memory, no context: the register of L bits started from init
    static uint64_t host(uint32_t r, uint64_t poly, uint64_t init, uint64_t xorout, const uint8_t *bits, size_t L)
    {
        uint64_t reg = 0;
        check(aeth_crc_host(r, poly, init, xorout, bits, L, &reg));
        return reg;
    }
    aeth_crc *get() const { return h_; }

private:
    aeth_crc *h_ = nullptr;
};

// one byte per bit <-> eight bits per byte; order is AETH_BITS_LSB_FIRST or AETH_BITS_MSB_FIRST
inline void pack_bits(Context &ctx, const uint8_t *bits_dev, size_t nbits, int order, uint8_t *bytes_dev)
{
    check(aeth_bits_pack(ctx.get(), bits_dev, nbits, order, bytes_dev, (nbits + 7) / 8));
}
inline void unpack_bits(Context &ctx, const uint8_t *bytes_dev, size_t nbytes, int order, uint8_t *bits_dev, size_t nbits)
{
    check(aeth_bits_unpack(ctx.get(), bytes_dev, nbytes, order, bits_dev, nbits));
}

// ---- OFDM symbols (no body in the reference: it has Fft, vec_mul and chunks_mut(fft_len) framing only) ----------------
// A transform length, a cyclic prefix and a carrier list (bins[k]: the FFT bin of carrier k).  demod strips the prefix,
// transforms with the sign of Fft::fwd, picks the carriers and multiplies by eq[k] in one kernel; mod is the way back with
// the sign of Fft::bwd; estimate sums n_sym training symbols per carrier in f64 into the channel h, the equaliser's
// coefficients eq (AETH_OFDM_EQ_*) and csi = |h|^2.  Device pointers in and out, ordered on the context's stream.
class Ofdm {
public:
    Ofdm(Context &ctx, size_t n_fft, size_t cp, const std::vector<uint32_t> &bins, size_t max_symbols = 0, bool general = false)
    {
        check(aeth_ofdm_create(ctx.get(), n_fft, cp, bins.data(), bins.size(), max_symbols, general ? AETH_OFDM_GENERAL : 0, &h_));
    }
    ~Ofdm() { aeth_ofdm_destroy(h_); }
    Ofdm(const Ofdm &) = delete;
    Ofdm &operator=(const Ofdm &) = delete;
    size_t len() const { return aeth_ofdm_len(h_); }
    size_t cp() const { return aeth_ofdm_cp(h_); }
    size_t symbol() const { return aeth_ofdm_symbol(h_); }
    size_t carriers() const { return aeth_ofdm_carriers(h_); }
    std::string route() const { return aeth_ofdm_route(h_); }
    // samples demod reads for n_sym symbols: (n_sym - 1) * symbol() + len()
    size_t span(size_t n_sym) const { return aeth_ofdm_span(h_, n_sym); }
    // in_dev points at the first window sample; eq_dev: carriers() coefficients or null; out_dev holds n_sym * carriers()
    void demod(const aeth_cf32 *in_dev, size_t n_in, size_t n_sym, aeth_cf32 *out_dev, size_t n_out, const aeth_cf32 *eq_dev = nullptr,
               Scale s = Scale::None())
    {
        check(aeth_ofdm_demod(h_, in_dev, n_in, n_sym, eq_dev, s.kind, s.x, out_dev, n_out));
    }
    // car_dev holds n_sym * carriers() carriers, out_dev n_sym * symbol() samples
    void mod(const aeth_cf32 *car_dev, size_t n_car, size_t n_sym, aeth_cf32 *out_dev, size_t n_out, Scale s = Scale::None())
    {
        check(aeth_ofdm_mod(h_, car_dev, n_car, n_sym, s.kind, s.x, out_dev, n_out));
    }
    // x_sym: 1 (one known symbol, repeated) or n_sym; any of h_dev, eq_dev, csi_dev may be null, not all
    void estimate(const aeth_cf32 *y_dev, const aeth_cf32 *x_dev, size_t n_sym, size_t x_sym, aeth_cf32 *h_dev, aeth_cf32 *eq_dev,
                  float *csi_dev, int eq_kind = AETH_OFDM_EQ_ZF, float nv = 0.f)
    {
        check(aeth_ofdm_estimate(h_, y_dev, x_dev, n_sym, x_sym, nv, eq_kind, h_dev, eq_dev, csi_dev));
    }
    aeth_ofdm *get() const { return h_; }

private:
    aeth_ofdm *h_ = nullptr;
};

// ---- sequence::expand / sequence::generate for linear generators (src/sequence.rs:18-53) ----------------------------
// A register is the set of its delays: seq[n] = XOR seq[n - d]; 1 .. 4 registers XORed (Gold codes: two).  `init` holds
// one word per register, bit i = seq[i] (what expand() unpacks).  Device pointers in and out; bits are one byte each.
namespace sequence {
inline std::vector<uint8_t> expand(uint64_t seed, size_t len)                       // :18-21 (len > 64 panics there)
{
    if (len > 64) throw Panic(AETH_E_ARG, "attempt to shift right with overflow");
    std::vector<uint8_t> v(len);
    for (size_t i = 0; i < len; i++) v[i] = (uint8_t)((seed >> i) & 1u);
    return v;
}
// the 64 values at [skip, skip + 64) of one register, on the host
inline uint64_t window(const std::vector<uint32_t> &delays, uint64_t init, uint64_t skip)
{
    aeth_seq_reg r{delays.data(), delays.size()};
    uint64_t w = 0;
    check(aeth_seq_window(&r, init, skip, &w));
    return w;
}
}  // namespace sequence

class Sequence {
public:
    Sequence(Context &ctx, const std::vector<std::vector<uint32_t>> &regs) : ctx_(&ctx)
    {
        std::vector<aeth_seq_reg> r;
        for (const auto &d : regs) r.push_back(aeth_seq_reg{d.data(), d.size()});
        check(aeth_seq_create(ctx.get(), r.data(), r.size(), &h_));
    }
    ~Sequence() { aeth_seq_destroy(h_); }
    Sequence(const Sequence &) = delete;
    Sequence &operator=(const Sequence &) = delete;
    size_t nregs() const { return aeth_seq_nregs(h_); }
    size_t order(size_t reg = 0) const { return aeth_seq_order(h_, reg); }
    size_t chunk() const { return aeth_seq_chunk(h_); }
    // c[i], i in [skip, skip + n), one byte per bit
    void bits(const std::vector<uint64_t> &init, uint64_t skip, uint8_t *bits_dev, size_t n) { check(aeth_seq_bits(h_, words(init), skip, bits_dev, n)); }
    // sequence::generate's own shape (:47-53): a host vector comes back
    std::vector<uint8_t> generate(const std::vector<uint64_t> &init, size_t n, uint64_t skip = 0)
    {
        std::vector<uint8_t> v(n);
        check(aeth_host_seq_bits(h_, words(init), skip, v.data(), n));
        return v;
    }
    // out = (in & 1) ^ c; out == in runs in place
    void scramble(const std::vector<uint64_t> &init, uint64_t skip, const uint8_t *in_dev, uint8_t *out_dev, size_t n)
    {
        check(aeth_seq_scramble(h_, words(init), skip, in_dev, out_dev, n));
    }
    // out = c ? one : zero (defaults: GENERIC_BPSK_TABLE, src/modulation.rs:77)
    void chips(const std::vector<uint64_t> &init, uint64_t skip, DeviceVec &out, cf32 zero = {1.f, 1.f}, cf32 one = {-1.f, -1.f})
    {
        check(aeth_seq_chips(h_, words(init), skip, *raw(&zero), *raw(&one), out.ptr(), out.len()));
    }
    // out[i] = sym[i / sf], negated where c[i] == 1; sf == 1 with &out == &sym runs in place
    void spread(const std::vector<uint64_t> &init, uint64_t skip, const DeviceVec &sym, size_t sf, DeviceVec &out)
    {
        check(aeth_seq_spread(h_, words(init), skip, sym.ptr(), sym.len(), sf, out.ptr(), out.len()));
    }
    aeth_seq *get() const { return h_; }

private:
    const uint64_t *words(const std::vector<uint64_t> &init) const
    {
        if (init.size() != nregs()) throw Panic(AETH_E_LEN, "one init word per register");
        return init.data();
    }
    Context *ctx_;
    aeth_seq *h_ = nullptr;
};

// ---- pipeline (src/pipeline.rs:24-41 add_stage, :123-137 new, :89-114 the per-stage report) ------------------
// The reference chains closures over channels; the device pipeline has five fixed stages (copy-in | upload | compute |
// download | copy-out) and the compute stage is one of the library's ops:
//     auto y = pipeline::stage_fft(fft, Scale::SN()).run(ctx, x);            // Vec<cf32> -> Vec<cf32>
//     auto b = pipeline::stage_correlate_demod(fft, sig, 2).run_bits(ctx, x);  // Vec<cf32> -> Vec<u8>
namespace pipeline {
struct Stage {
    aeth_stream_op op{};
    size_t out_count(Context &ctx, size_t n_in) const { return aeth_stream_out_count(ctx.get(), &op, n_in); }
    // host slices; with report = true the reference's per-stage lines go to stdout
    aeth_pipe_util run(Context &ctx, const void *in, size_t n_in, void *out, size_t n_out, size_t chunk = 0, bool report = false) const
    {
        aeth_pipe_util u{};
        check(aeth_stream_host_util(ctx.get(), &op, in, n_in, out, n_out, chunk, &u));
        if (report) Fir::print_report(u);
        return u;
    }
    std::vector<cf32> run(Context &ctx, const std::vector<cf32> &x, size_t chunk = 0) const
    {
        std::vector<cf32> y(out_count(ctx, x.size()));
        run(ctx, x.data(), x.size(), y.data(), y.size(), chunk);
        return y;
    }
    std::vector<uint8_t> run_bits(Context &ctx, const std::vector<cf32> &x, size_t chunk = 0) const
    {
        std::vector<uint8_t> y(out_count(ctx, x.size()));
        run(ctx, x.data(), x.size(), y.data(), y.size(), chunk);
        return y;
    }
};
inline Stage stage_fir(const Fir &f) { Stage s; s.op.kind = AETH_STREAM_FIR; s.op.fir = f.get(); return s; }
inline Stage stage_fir_decim(const Fir &f, size_t dec) { Stage s; s.op.kind = AETH_STREAM_FIR_DECIM; s.op.fir = f.get(); s.op.n_between = dec; return s; }
inline Stage stage_fft(const HipFft &f, Scale sc, int sign = HipFft::kFwdSign)
{
    Stage s; s.op.kind = AETH_STREAM_FFT; s.op.fft = f.get(); s.op.sign = sign; s.op.scale_kind_fwd = sc.kind; s.op.x_fwd = sc.x; return s;
}
inline Stage stage_mul_chain(const HipFft &f, const DeviceVec &sig, Scale s_fwd, Scale s_bwd)
{
    Stage s; s.op.kind = AETH_STREAM_FFT_MUL_IFFT; s.op.fft = f.get(); s.op.sig_dev = sig.ptr(); s.op.n_sig = sig.len();
    s.op.scale_kind_fwd = s_fwd.kind; s.op.x_fwd = s_fwd.x; s.op.scale_kind_bwd = s_bwd.kind; s.op.x_bwd = s_bwd.x; return s;
}
inline Stage stage_correlate_demod(const HipFft &f, const DeviceVec &sig, int bits_per_symbol, bool compat = true)
{
    Stage s; s.op.kind = AETH_STREAM_FFT_MUL_IFFT_DEMOD; s.op.fft = f.get(); s.op.sig_dev = sig.ptr(); s.op.n_sig = sig.len();
    s.op.bits_per_symbol = bits_per_symbol; s.op.compat = compat ? 1 : 0; return s;
}
inline Stage stage_fft_interpolate(const HipFft &f, size_t n_between, Scale sc, bool compat_im = true)
{
    Stage s; s.op.kind = AETH_STREAM_FFT_INTERPOLATE; s.op.fft = f.get(); s.op.sign = HipFft::kFwdSign; s.op.scale_kind_fwd = sc.kind;
    s.op.x_fwd = sc.x; s.op.n_between = n_between; s.op.compat = compat_im ? 1 : 0; return s;
}
}  // namespace pipeline

// ---- sampling (src/sampling.rs) ---------------------------------------------------------
// appends to dst, as the reference does (sampling.rs:17,23)
inline void interpolate(Context &ctx, const std::vector<cf32> &src, std::vector<cf32> &dst, size_t n_between,
                        bool compat_im = true)
{
    if (src.empty()) throw Panic(AETH_E_LEN, "interpolate on an empty src (the reference panics: sampling.rs:23)");
    const size_t add = src.size() + (src.size() - 1) * n_between, old = dst.size();
    dst.resize(old + add);
    size_t written = 0;
    check(aeth_host_interpolate(ctx.get(), raw(src.data()), src.size(), raw(dst.data() + old), add, n_between,
                                compat_im ? 1 : 0, &written));
    dst.resize(old + written);
}

// The reference checks divisibility with a debug_assert_eq! (sampling.rs:32-36): AETHER_REF_RELEASE_BUILD selects the
// semantics of its release build (assert compiled out, ratio floors: what `cargo bench` runs, benches/benches.rs:113,130)
// the way NDEBUG-less / --release selects them for the crate itself; the default mirrors `cargo test` (debug).
#ifdef AETHER_REF_RELEASE_BUILD
constexpr bool kRefReleaseBuild = true;
#else
constexpr bool kRefReleaseBuild = false;
#endif
template <typename T>
inline void downsample(Context &ctx, const std::vector<T> &src, std::vector<T> &dst, bool release = kRefReleaseBuild)
{
    if (release) check(aeth_host_downsample_release(ctx.get(), src.data(), src.size(), dst.data(), dst.size(), sizeof(T), 0));
    else check(aeth_host_downsample(ctx.get(), src.data(), src.size(), dst.data(), dst.size(), sizeof(T)));
}
template <typename T>
inline void downsample_sb(Context &ctx, const std::vector<T> &src, std::vector<T> &dst, bool release = kRefReleaseBuild)
{
    if (release) check(aeth_host_downsample_release(ctx.get(), src.data(), src.size(), dst.data(), dst.size(), sizeof(T), 1));
    else check(aeth_host_downsample(ctx.get(), src.data(), src.size(), dst.data(), dst.size(), sizeof(T)));
}

// ---- assert_evm! (src/lib.rs:26-49), literal, plus a NaN reject ---------------------------
inline void assert_evm(const std::vector<cf32> &actual, const std::vector<cf32> &ref, double evm_limit_db = -80.0)
{
    if (actual.size() != ref.size()) throw Panic(AETH_E_LEN, "Input slices/vectors must be same length");
    if (!(evm_limit_db < 0.0)) throw Panic(AETH_E_ARG, "The EVM threshold must be negative");
    const float fac = (float)std::pow(10.0, evm_limit_db / 10.0);
    for (size_t i = 0; i < actual.size(); i++) {
        const float evm = std::abs(actual[i] - ref[i]);
        const float limit = std::abs(ref[i]) * fac;
        if (evm > limit || std::isnan(actual[i].real()) || std::isnan(actual[i].imag()))
            throw Panic(AETH_E_ARG, "EVM limit exceeded for element " + std::to_string(i));
    }
}

}  // namespace aether
