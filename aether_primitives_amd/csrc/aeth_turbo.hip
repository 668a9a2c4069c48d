// aeth_turbo.hip -- turbo codes: two recursive systematic encoders with their tails and a windowed max-log-MAP iterative
// decoder with early stop and a record per codeword (no body in the reference; definition in include/aether_hip.h,
// aeth_turbo_*).  Everything is integer and defined byte for byte; compiled with the EXACT flags like the other bit-exact
// kernels.
//
// Decoder.  A lane owns one window of a codeword and keeps all S state metrics in registers, S = 4, 8, 16 a template
// parameter: with a = u ^ fbp(s) the step is s' = (a << (nu - 1)) | (s >> 1) for every polynomial, so the branches are
// unrolled over (s, a) at compile time, the add-compare-select is VALU only with no cross-lane traffic, and the
// polynomials enter as two uniform masks that give a branch's value +-x +-p its signs (aeth_turbo_core.h).  A workgroup
// owns G codewords, G x windows lanes, and loops over the call's groups of G with the grid's stride.
//   - LDS, per codeword, for the whole call: the frame's N soft values as they came, the K systematic values in
//     interleaved order, and the a-priori arrays a1 and a2 as int16.  An entry is (scale(e) << 1) | h: a2[i] carries
//     h1[pi[i]] to the lane that compares it with h2, and a1 carries h2, which is the output.  Memory is read once and
//     written once per codeword.
//   - A half-iteration per lane: warm-up and window forward, alpha of each window step to the store; warm-up (or the
//     tail) and window backward, forming D, e and scale(e) on the fly and writing the other constituent's a-priori through
//     pi or its inverse.  One workgroup barrier between half-iterations.
//   - The alpha store is int32 in device memory the object owns, one slab per resident workgroup, [step][lane][state]:
//     a lane moves its S values of a step in 16-byte accesses and a wave's lanes cover consecutive lines.  (W S 4 bytes per lane do not fit the LDS beside the frame at
//     K = 6144, and W may be the whole frame)
//   - The exact start (alpha or beta = {0, NEG, ...}) is taken by the lanes whose warm-up is clipped at step 0 or at the
//     tail, the zero start by all others: a per-lane choice.  A codeword that stops early shares its workgroup with
//     codewords that go on: its lanes skip the passes and still arrive at every barrier.
//
// Encoder.  A lane runs one constituent of one codeword serially: lane 2 c of a call takes u[i] and writes the systematic
// and first parity planes, lane 2 c + 1 takes u[pi[i]].
#include "aeth_turbo_core.h"

#include <new>
#include <vector>

namespace {

namespace tc = aeth::turbo;

constexpr int kMaxBlock = 1024;
constexpr int kEncBlock = 64;
constexpr int32_t kNeg = -(1 << 28);

struct DecCall {
    const int8_t *soft;
    uint8_t *bits;
    aeth_turbo_record *rec;             // or null
    const uint16_t *pi;                 // [K], then [K] its inverse
    int32_t *store;                     // [gridDim.x] slabs of `slab` words
    uint64_t F, slab;
    uint32_t groups;                    // of G codewords
    uint32_t K, N, W, A, nwin, G, cwb;  // cwb: bytes of LDS per codeword
    uint32_t max_iter, early;
    tc::Trellis tr;
};

// A trellis in a kernel's registers.  Branch (s, a) -- a is the bit that enters the register -- goes to state
// (a << (nu - 1)) | (s >> 1) and carries g = (1 - 2u) x + (1 - 2z) p with u = a ^ fbp(s), z = (a & ffmsb) ^ ffp(s).  The
// signs are uniform values used as multipliers: g(s, 0) = su x + sz p, g(s, 1) = -su x + kq sz p, kq = -1 where ff has
// its top bit; su = -1 where bit s of fbm is set (a = 0 is then the branch of input 1), sz = -1 where bit s of ffm is.
template <int S> struct Trel {
    static constexpr int NU = S == 4 ? 2 : S == 8 ? 3 : 4;
    uint32_t fbm, ffm;
    int32_t kq;
    __device__ __forceinline__ explicit Trel(const tc::Trellis &t) : fbm(t.fbm), ffm(t.ffm), kq(1 - 2 * (int32_t)t.ffmsb) {}
    // Called once per trellis step: the masks are read afresh (to the compiler: from a vector register it cannot see
    // through), and a sign is made from its bit where it is used, by two scalar instructions.  Without it the 2 S signs
    // are hoisted out of the loops, S = 16 runs out of scalar registers and they are spilled.
    __device__ __forceinline__ void pin()
    {
        uint32_t f = fbm, z = ffm;
        asm volatile("" : "+v"(f), "+v"(z));
        fbm = __builtin_amdgcn_readfirstlane(f);
        ffm = __builtin_amdgcn_readfirstlane(z);
    }
    static __device__ __forceinline__ int32_t sign(uint32_t mask, int s) { return ((int32_t)(mask << (31 - s)) >> 31) | 1; }   // bit set: -1
    __device__ __forceinline__ int32_t su(int s) const { return sign(fbm, s); }
    static constexpr int next(int s, int a) { return (a << (NU - 1)) | (s >> 1); }
    // base0 + g(s, 0) and base1 + g(s, 1); |x| and |p| are far below 2^23
    __device__ __forceinline__ void both(int s, int32_t x, int32_t p, int32_t pk, int32_t base0, int32_t base1, int32_t &v0, int32_t &v1) const
    {
        const int32_t X = __mul24(x, sign(fbm, s)), sz = sign(ffm, s);
        v0 = __mul24(p, sz) + base0 + X;
        v1 = __mul24(pk, sz) + base1 - X;
    }
};

// m ? a : b bit by bit; m is all ones or zero
__device__ __forceinline__ int32_t pick(uint32_t m, int32_t a, int32_t b) { return (int32_t)((uint32_t)b ^ (((uint32_t)a ^ (uint32_t)b) & m)); }

template <int S> __device__ __forceinline__ void fwd_step(int32_t (&al)[S], int32_t x, int32_t p, Trel<S> &tr)
{
    tr.pin();
    const int32_t pk = __mul24(p, tr.kq);
    int32_t v0[S], v1[S];
#pragma unroll
    for (int s = 0; s < S; s++) tr.both(s, x, p, pk, al[s], al[s], v0[s], v1[s]);
#pragma unroll
    for (int n = 0; n < S / 2; n++) {                                     // the two branches into a state
        al[n] = max(v0[2 * n], v0[2 * n + 1]);
        al[n + S / 2] = max(v1[2 * n], v1[2 * n + 1]);
    }
}

// the alpha store of a workgroup: a uniform base and a byte offset below 2^32 per lane, four states per access
typedef int32_t Quad __attribute__((ext_vector_type(4)));
__device__ __forceinline__ Quad *store_at(int32_t *slab, uint32_t byte) { return reinterpret_cast<Quad *>(reinterpret_cast<char *>(slab) + byte); }

// one window of siso(x, p) for one constituent.  xs: the K systematic values in this constituent's order, ap: its a-priori
// entries, ps: its K parities, tail: its nu (x, z) pairs.  Window step t writes dst[tab[t]] = (scale(e) << 1) | h and
// returns the number of steps whose decision differs from bit 0 of ap[t] (meaningful in the second half only).  The
// lane's alpha_t[s] lies at slab[((t - w0) nl + lane) S + s]; `first` is the byte offset of its first value, `step` of a row.
template <int S>
__device__ __forceinline__ uint32_t window_pass(const DecCall &a, uint32_t w, const int8_t *xs, const int16_t *ap, const int8_t *ps,
                                                const int8_t *tail, const uint16_t *tab, int16_t *dst, int32_t *slab, uint32_t first,
                                                uint32_t step, Trel<S> &tr)
{
    typedef Trel<S> T;
    const uint32_t K = a.K, w0 = w * a.W, e = min(w0 + a.W, K);
    int32_t m[S];

    // forward: warm-up, then the window with alpha_t stored in front of step t
    uint32_t t = w0 <= a.A ? 0u : w0 - a.A;
    const int32_t rest = w0 <= a.A ? kNeg : 0;
#pragma unroll
    for (int s = 0; s < S; s++) m[s] = s ? rest : 0;
    uint32_t at = first;
#pragma nounroll
    for (; t < e; t++) {
        if (t >= w0) {
#pragma unroll
            for (int q = 0; q < S / 4; q++) store_at(slab, at)[q] = Quad{m[4 * q], m[4 * q + 1], m[4 * q + 2], m[4 * q + 3]};
            at += step;
        }
        if (t + 1 < e) fwd_step<S>(m, (int32_t)xs[t] + (ap[t] >> 1), ps[t], tr);
    }

    // backward: from the end of the tail or of the warm-up; a step inside the window also forms D, e and scale(e)
    const bool exact = e + a.A >= K;
    t = exact ? K + T::NU : e + a.A;
    const int32_t brest = exact ? kNeg : 0;
#pragma unroll
    for (int s = 0; s < S; s++) m[s] = s ? brest : 0;
    uint32_t differ = 0;
#pragma nounroll
    while (t > w0) {
        t--;
        int32_t old = 0, x, p;
        if (t >= K) {
            x = tail[2 * (t - K)];
            p = tail[2 * (t - K) + 1];
        } else {
            old = ap[t];
            x = (int32_t)xs[t] + (old >> 1);
            p = ps[t];
        }
        tr.pin();
        const int32_t pk = __mul24(p, tr.kq);
        int32_t b0[S], b1[S];
#pragma unroll
        for (int s = 0; s < S; s++) tr.both(s, x, p, pk, m[T::next(s, 0)], m[T::next(s, 1)], b0[s], b1[s]);
#pragma unroll
        for (int s = 0; s < S; s++) m[s] = max(b0[s], b1[s]);
        if (t < e) {
            at -= step;
            int32_t m0 = INT32_MIN, m1 = INT32_MIN;
#pragma unroll
            for (int q = 0; q < S / 4; q++) {
                const Quad v = store_at(slab, at)[q];
                const int32_t al[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int s = 4 * q + k;
                    const uint32_t swap = (uint32_t)(tr.su(s) >> 1);      // all ones where a = 0 is the branch of input 1
                    m0 = max(m0, al[k] + pick(swap, b1[s], b0[s]));
                    m1 = max(m1, al[k] + pick(swap, b0[s], b1[s]));
                }
            }
            const int32_t D = m0 - m1, ex = D - 2 * x;
            const int32_t mag = min((3 * abs(ex)) >> 3, 2047);
            const int32_t h = D < 0 ? 1 : 0;
            differ += (uint32_t)((old & 1) != h);
            dst[tab[t]] = (int16_t)(((ex < 0 ? -mag : mag) << 1) | h);
        }
    }
    return differ;
}

template <int S> __global__ __launch_bounds__(kMaxBlock) void turbo_decode_kernel(DecCall a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char turbo_lds[];
    constexpr uint32_t NU = Trel<S>::NU;
    const uint32_t tid = threadIdx.x, nl = a.G * a.nwin;
    const uint32_t g = tid / a.nwin, w = tid - g * a.nwin;               // the lane's codeword of the group and its window
    const uint32_t K = a.K, N = a.N;
    uint32_t *counts = reinterpret_cast<uint32_t *>(turbo_lds + (size_t)a.G * a.cwb);   // [G][2] disagreements, by iteration parity
    uint32_t *going = counts + 2 * a.G;                                   // [2] a codeword of the group goes on
    Trel<S> tr(a.tr);
    int32_t *slab = a.store + (size_t)blockIdx.x * a.slab;

    // the lane's codeword in LDS (lanes beyond G x windows own none)
    unsigned char *mine = turbo_lds + (size_t)(tid < nl ? g : 0) * a.cwb;
    const int8_t *soft = reinterpret_cast<const int8_t *>(mine);
    int8_t *s2 = reinterpret_cast<int8_t *>(mine + tc::pad4(N));
    int16_t *a1 = reinterpret_cast<int16_t *>(mine + tc::pad4(N) + tc::pad4(K)), *a2 = a1 + K;

    for (uint32_t grp = blockIdx.x; grp < a.groups; grp += gridDim.x) {
        const uint64_t cw0 = (uint64_t)grp * a.G;
        const uint32_t ncw = a.F - cw0 < a.G ? (uint32_t)(a.F - cw0) : a.G;
        for (uint32_t c = 0; c < ncw; c++) {                              // the frames as they came, a1 = 0
            unsigned char *cwl = turbo_lds + (size_t)c * a.cwb;
            const int8_t *src = a.soft + (cw0 + c) * N;
            for (uint32_t i = tid; i < N; i += blockDim.x) cwl[i] = (unsigned char)src[i];
            int16_t *z = reinterpret_cast<int16_t *>(cwl + tc::pad4(N) + tc::pad4(K));
            for (uint32_t i = tid; i < K; i += blockDim.x) z[i] = 0;
        }
        for (uint32_t i = tid; i < 2 * a.G + 2; i += blockDim.x) counts[i] = 0;
        __syncthreads();
        for (uint32_t c = 0; c < ncw; c++) {                              // the systematic values in interleaved order
            unsigned char *cwl = turbo_lds + (size_t)c * a.cwb;
            for (uint32_t i = tid; i < K; i += blockDim.x) cwl[tc::pad4(N) + i] = cwl[a.pi[i]];
        }
        __syncthreads();

        const bool real = tid < nl && g < ncw;
        bool live = real;
        uint32_t iters = 0, dis = 0;
        for (uint32_t it = 1; it <= a.max_iter; it++) {
            for (uint32_t half = 0; half < 2; half++) {
                if (live) {
                    const uint32_t d = window_pass<S>(a, w, half ? s2 : soft, half ? a2 : a1, soft + K + half * K, soft + 3 * K + half * 2 * NU,
                                                      a.pi + (half ? 0u : K), half ? a1 : a2, slab, 4 * S * tid, 4 * S * nl, tr);
                    if (half && d) atomicAdd(&counts[2 * g + (it & 1u)], d);
                }
                __syncthreads();
            }
            if (live) {
                iters = it;
                dis = counts[2 * g + (it & 1u)];
                if (w == 0) counts[2 * g + ((it + 1) & 1u)] = 0;          // read last before this iteration's first barrier
                if (a.early && dis == 0) live = false;
            }
            if (a.early) {                                                // uniform: the whole group may be done
                if (live) going[it & 1u] = 1;
                if (tid == 0) going[(it + 1) & 1u] = 0;
                __syncthreads();
                if (!going[it & 1u]) break;
            }
        }

        for (uint32_t c = 0; c < ncw; c++) {                              // h2 of the last iteration run is bit 0 of a1
            const int16_t *h = reinterpret_cast<const int16_t *>(turbo_lds + (size_t)c * a.cwb + tc::pad4(N) + tc::pad4(K));
            uint8_t *out = a.bits + (cw0 + c) * K;
            for (uint32_t i = tid; i < K; i += blockDim.x) out[i] = (uint8_t)(h[i] & 1);
        }
        if (a.rec && real && w == 0) a.rec[cw0 + g] = aeth_turbo_record{iters, dis};
        __syncthreads();                                                  // the next group overwrites the LDS
    }
}

struct EncCall {
    const uint8_t *in;
    uint8_t *out;
    const uint16_t *pi;
    uint64_t F;
    uint32_t K, N, nu;
    uint32_t fb, ff;                    // fb without its top bit; ff whole
};

__global__ __launch_bounds__(kEncBlock) void turbo_encode_kernel(EncCall a)
{
    const uint64_t id = (uint64_t)blockIdx.x * kEncBlock + threadIdx.x;
    const uint64_t cw = id >> 1;
    if (cw >= a.F) return;
    const uint32_t second = (uint32_t)id & 1u, K = a.K, nu = a.nu;
    const uint8_t *u = a.in + cw * K;
    uint8_t *out = a.out + cw * a.N;
    uint8_t *zs = out + (second ? 2 * K : K), *tail = out + 3 * K + (second ? 2 * nu : 0);
    uint32_t s = 0;
    for (uint32_t i = 0; i < K; i++) {
        const uint32_t b = u[second ? a.pi[i] : i] & 1u;
        const uint32_t reg = ((b ^ ((uint32_t)__popc(s & a.fb) & 1u)) << nu) | s;
        if (!second) out[i] = (uint8_t)b;
        zs[i] = (uint8_t)(__popc(reg & a.ff) & 1);
        s = reg >> 1;
    }
    for (uint32_t j = 0; j < nu; j++) {                                   // u_tail makes a = 0: reg = s
        tail[2 * j] = (uint8_t)(__popc(s & a.fb) & 1);
        tail[2 * j + 1] = (uint8_t)(__popc(s & a.ff) & 1);
        s >>= 1;
    }
}

}  // namespace

struct aeth_turbo {
    aeth_ctx *ctx;
    uint32_t K, N, k, S, W, A, nwin, G, cwb, slots;
    uint64_t slab;                      // int32 values of one workgroup's alpha store
    aeth_turbo_code code;
    uint16_t *perm_dev;                 // [K] pi, then [K] its inverse
    int32_t *store_dev;                 // [slots][slab]
};

extern "C" {

int aeth_turbo_named(const char *name, aeth_turbo_code *code_out)
{
    AETH_REQUIRE(name, AETH_E_ARG, "name is null");
    AETH_REQUIRE(code_out, AETH_E_ARG, "code_out is null");
    for (const tc::Named &n : tc::kNamed)
        if (!std::strcmp(name, n.name)) {
            *code_out = n.code;
            return AETH_OK;
        }
    return aeth::set_error(AETH_E_ARG, "no turbo code is named '%.32s' (lte, ccsds, k3)", name);
}

int aeth_turbo_qpp(uint32_t K, uint32_t f1, uint32_t f2, uint32_t *pi_out, size_t count)
{
    if (int rc = tc::check_bits(K)) return rc;
    AETH_REQUIRE(count >= K, AETH_E_LEN, "the interleaver of K = %u has %u entries, pi_out holds %zu", K, K, count);
    AETH_REQUIRE(pi_out, AETH_E_ARG, "pi_out is null");
    std::vector<uint32_t> pi;
    tc::qpp(K, f1, f2, pi);
    if (int rc = tc::check_permutation(pi.data(), K)) return rc;
    std::copy(pi.begin(), pi.end(), pi_out);
    return AETH_OK;
}

int aeth_turbo_create(aeth_ctx *ctx, const aeth_turbo_code *code, uint32_t K, const uint32_t *pi_host, uint32_t window, uint32_t warmup,
                      aeth_turbo **out)
{
    AETH_REQUIRE(out, AETH_E_ARG, "out is null");
    *out = nullptr;
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    int rc = tc::check_code(code);
    if (rc) return rc;
    if ((rc = tc::check_bits(K))) return rc;
    AETH_REQUIRE(window >= 1, AETH_E_ARG, "window = 0");
    AETH_REQUIRE(warmup <= tc::kMaxWarm, AETH_E_ARG, "warmup = %u above %u", warmup, tc::kMaxWarm);
    AETH_REQUIRE(pi_host, AETH_E_ARG, "pi is null");
    if ((rc = tc::check_permutation(pi_host, K))) return rc;
    const uint32_t nwin = tc::windows_of(K, window);
    AETH_REQUIRE(nwin <= tc::kMaxWindows, AETH_E_UNSUPPORTED, "K = %u in windows of %u steps are %u windows: more than %u", K, window, nwin,
                 tc::kMaxWindows);
    aeth_turbo *t = new (std::nothrow) aeth_turbo{};
    AETH_REQUIRE(t, AETH_E_NOMEM, "out of host memory");
    const uint32_t nu = code->k - 1;
    t->ctx = ctx;
    t->code = *code;
    t->K = K; t->N = tc::frame_of(K, nu); t->k = code->k; t->S = 1u << nu;
    t->W = window; t->A = warmup; t->nwin = nwin;
    t->G = tc::group_of(K, nu, nwin);
    t->cwb = tc::lds_per_codeword(K, nu);
    t->slab = tc::store_words(K, window, t->S, t->G, nwin);
    // as many slabs as workgroups can be resident, within the budget; a call with more groups loops
    const uint64_t by_budget = std::max<uint64_t>(1, tc::kStoreBudget / (t->slab * sizeof(int32_t)));
    t->slots = (uint32_t)std::min<uint64_t>(by_budget, 8ull * (uint64_t)std::max(ctx->num_cus, 1));
    std::vector<uint16_t> perm(2 * (size_t)K);
    for (uint32_t i = 0; i < K; i++) {
        perm[i] = (uint16_t)pi_host[i];
        perm[K + pi_host[i]] = (uint16_t)i;
    }
    rc = aeth::upload_table(ctx, perm.data(), perm.size() * sizeof(uint16_t), &t->perm_dev, "aeth_turbo_create: interleaver");
    if (!rc) {
        aeth::DeviceGuard dg(ctx->device);
        const hipError_t e = hipMalloc((void **)&t->store_dev, (size_t)t->slots * t->slab * sizeof(int32_t));
        if (e != hipSuccess) {
            t->store_dev = nullptr;
            rc = aeth::hip_fail(e, "aeth_turbo_create: alpha store");
        }
    }
    if (rc) {
        (void)aeth::release_tables(ctx, {t->store_dev, t->perm_dev});
        delete t;
        return rc;
    }
    *out = t;
    return AETH_OK;
}

int aeth_turbo_destroy(aeth_turbo *t)
{
    if (!t) return AETH_OK;
    const hipError_t freed = aeth::release_tables(t->ctx, {t->store_dev, t->perm_dev});
    delete t;
    return freed == hipSuccess ? AETH_OK : aeth::hip_fail(freed, "hipFree");
}

size_t aeth_turbo_k(const aeth_turbo *t) { return t ? t->K : 0; }
size_t aeth_turbo_n(const aeth_turbo *t) { return t ? t->N : 0; }
uint32_t aeth_turbo_states(const aeth_turbo *t) { return t ? t->S : 0; }
uint32_t aeth_turbo_window(const aeth_turbo *t) { return t ? t->W : 0; }
uint32_t aeth_turbo_warmup(const aeth_turbo *t) { return t ? t->A : 0; }
uint32_t aeth_turbo_windows(const aeth_turbo *t) { return t ? t->nwin : 0; }
uint32_t aeth_turbo_group(const aeth_turbo *t) { return t ? t->G : 0; }
size_t aeth_turbo_lds_bytes(const aeth_turbo *t) { return t ? tc::lds_bytes(t->K, t->k - 1, t->G) : 0; }

int aeth_turbo_encode(aeth_turbo *t, const uint8_t *bits_dev, size_t nbits, uint8_t *coded_dev, size_t ncoded)
{
    AETH_REQUIRE(t, AETH_E_ARG, "turbo is null");
    size_t F;
    if (int rc = aeth::check_codewords(false, nbits, t->K, ncoded, t->N, &F)) return rc;
    if (F == 0) return AETH_OK;
    AETH_REQUIRE(bits_dev && coded_dev, AETH_E_ARG, "null pointer");
    if (int rc = aeth::check_disjoint({{bits_dev, nbits}}, {{coded_dev, ncoded}})) return rc;
    const uint64_t wgs = (aeth::mul_sat(F, 2) + kEncBlock - 1) / kEncBlock;
    if (int rc = aeth::check_grid(wgs, F, "codewords")) return rc;
    aeth::DeviceGuard dg(t->ctx->device);
    hipStream_t st = aeth::ctx_stream(t->ctx);
    const uint32_t nu = t->k - 1;
    EncCall a{bits_dev, coded_dev, t->perm_dev, (uint64_t)F, t->K, t->N, nu, t->code.fb & (t->S - 1), t->code.ff};
    hipLaunchKernelGGL(turbo_encode_kernel, dim3((unsigned)wgs), dim3(kEncBlock), 0, st, a);
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

int aeth_turbo_decode(aeth_turbo *t, const int8_t *soft_dev, size_t nsoft, uint32_t max_iter, uint32_t flags, uint8_t *bits_dev, size_t nbits,
                      aeth_turbo_record *rec_dev)
{
    AETH_REQUIRE(t, AETH_E_ARG, "turbo is null");
    AETH_REQUIRE(max_iter >= 1 && max_iter <= tc::kMaxIter, AETH_E_ARG, "max_iter %u outside 1 .. %u", max_iter, tc::kMaxIter);
    if (int rc = aeth::check_flags(flags, AETH_TURBO_EARLY)) return rc;
    size_t F;
    if (int rc = aeth::check_codewords(true, nsoft, t->N, nbits, t->K, &F)) return rc;
    if (F == 0) return AETH_OK;
    AETH_REQUIRE(soft_dev && bits_dev, AETH_E_ARG, "null pointer");
    AETH_REQUIRE(aeth::aligned4(rec_dev), AETH_E_ALIGN, "rec_dev not 4-byte aligned");
    if (int rc = aeth::check_disjoint({{soft_dev, nsoft}}, {{bits_dev, nbits}, {rec_dev, F * sizeof(aeth_turbo_record)}})) return rc;
    const uint64_t groups = (F + t->G - 1) / t->G;
    if (int rc = aeth::check_grid(groups, F, "codewords")) return rc;
    aeth::DeviceGuard dg(t->ctx->device);
    hipStream_t st = aeth::ctx_stream(t->ctx);
    DecCall a{};
    a.soft = soft_dev; a.bits = bits_dev; a.rec = rec_dev;
    a.pi = t->perm_dev;
    a.store = t->store_dev;
    a.F = F; a.slab = t->slab; a.groups = (uint32_t)groups;
    a.K = t->K; a.N = t->N; a.W = t->W; a.A = t->A; a.nwin = t->nwin; a.G = t->G; a.cwb = t->cwb;
    a.max_iter = max_iter; a.early = (flags & AETH_TURBO_EARLY) ? 1 : 0;
    a.tr = tc::trellis_of(t->code);
    const size_t lds = tc::lds_bytes(t->K, t->k - 1, t->G);
    const unsigned wgs = (unsigned)std::min<uint64_t>(groups, t->slots);
    const unsigned block = (t->G * t->nwin + 63u) & ~63u;
#define AETH_TURBO_LAUNCH(S_)                                                                                                                  \
    do {                                                                                                                                       \
        if (lds > 48 * 1024)                                                                                                                   \
            AETH_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(turbo_decode_kernel<S_>), hipFuncAttributeMaxDynamicSharedMemorySize, \
                                         (int)lds));                                                                                           \
        hipLaunchKernelGGL(turbo_decode_kernel<S_>, dim3(wgs), dim3(block), lds, st, a);                                                       \
    } while (0)
    switch (t->S) {
    case 4: AETH_TURBO_LAUNCH(4); break;
    case 8: AETH_TURBO_LAUNCH(8); break;
    default: AETH_TURBO_LAUNCH(16); break;
    }
#undef AETH_TURBO_LAUNCH
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

}  // extern "C"
