// aeth_cc.hip -- convolutional codes: encoder and a soft-decision Viterbi decoder on the device
// (no body in the reference; definition in include/aether_hip.h, aeth_cc_*).  All integer, so the output is defined
// bit for bit; compiled with the EXACT flags like the other bit-exact kernels.
//
// The decoder is the library's one kernel bound by instruction issue, not by HBM: it moves n + 1 bytes per information
// bit.  A wave owns 64 / S output blocks (S = 2^(k-1) states, one state per lane, the blocks of a wave side by side in
// groups of S lanes).  A trellis step is one cross-lane read of the partner's metric (DPP or a row swap: see acs_step),
// two 4 x int8 dot products of the step's packed soft values with the lane's +-1 patterns (v_dot4_i32_i8, the metric as
// the accumulator), a compare and two selects.  The soft values come a round (a whole number of groups, at most S steps)
// ahead: lane j of a group of lanes loads step t0 + j, every step then takes its dword from that lane.  What the traceback needs goes to LDS once per row of
// about 32 steps (see acs_step); a workgroup is ONE wave, so its LDS belongs to it and the barriers between the forward
// pass, the traceback and the output stores order one wave only.  Lane 0 of a group traces its block back, K - 1 steps
// per LDS read, and leaves the emitted bits packed in the rows it has finished with; all lanes then store the bytes.
// The last, shorter block of a call (N % D steps) has a window of its own length and runs as a second launch.
#include "aeth_internal.h"

#include <new>

namespace {

constexpr int kWave = 64;
constexpr int kBlock = 256;                        // encoder
constexpr uint32_t kMaxSpan = 4096;                // D + T, and A

struct CcCode { uint32_t k, n, poly[4]; };

struct DecodeCall {
    const int8_t *hist;        // (A + T) * n values before step 0, or null: erasures
    const int8_t *soft;
    uint8_t *out;
    CcCode code;
    uint64_t b0, nb;           // first output block of this launch and their number
    uint32_t D, A, T, dlen;    // block stride; warm-up, traceback; outputs per block in this launch (D, or N % D)
};

// the n soft values of one step as they come from memory: bytes 0 and 1 (the compiler makes one 16-bit load of them),
// byte 2, byte 3 (bytes past n re-read byte 0).  Nothing here looks at a loaded value, so all the loads of a round stay
// in flight until pack() wants them.
struct RawStep { unsigned lo, b2, b3; };

__device__ __forceinline__ RawStep load_step(const DecodeCall &a, int64_t s)
{
    if (s < 0 && !a.hist) return RawStep{0, 0, 0};
    const int64_t n = a.code.n;
    const uint8_t *p = reinterpret_cast<const uint8_t *>(s < 0 ? a.hist + (s + (int64_t)(a.A + a.T)) * n : a.soft + s * n);
    return RawStep{(unsigned)p[0] | ((unsigned)p[1] << 8), p[n > 2 ? 2 : 0], p[n > 3 ? 3 : 0]};
}

// packed little-endian into a dword, bytes n .. 3 zero
__device__ __forceinline__ int pack(const RawStep &r, unsigned n)
{
    return (int)(r.lo | (n > 2 ? r.b2 << 16 : 0u) | (n > 3 ? r.b3 << 24 : 0u));
}

// the lane's pattern for predecessor p: byte q = 1 - 2 c_q(u, p)
__device__ __forceinline__ int pattern(const CcCode &c, unsigned u, unsigned p)
{
    const unsigned reg = (u << (c.k - 1)) | p;
    unsigned v = 0;
    for (unsigned q = 0; q < 4; q++) {
        if (q >= c.n) break;
        v |= ((__popc(reg & c.poly[q]) & 1) ? 0xffu : 0x01u) << (8 * q);
    }
    return (int)v;
}

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// x of lane ^ (1 << R) without a trip through the LDS: DPP inside a row of 16 lanes, the gfx950 row swaps across rows
template <int R> __device__ __forceinline__ int partner(int x, unsigned lane)
{
    if constexpr (R == 0) return __builtin_amdgcn_mov_dpp(x, 0xB1, 0xf, 0xf, true);          // quad_perm:[1,0,3,2]
    else if constexpr (R == 1) return __builtin_amdgcn_mov_dpp(x, 0x4E, 0xf, 0xf, true);     // quad_perm:[2,3,0,1]
    else if constexpr (R == 2)                                                                 // i ^ 7, then ^ 3
        return __builtin_amdgcn_mov_dpp(__builtin_amdgcn_mov_dpp(x, 0x141, 0xf, 0xf, true), 0x1B, 0xf, 0xf, true);   // row_half_mirror, quad_perm:[3,2,1,0]
    else if constexpr (R == 3) return __builtin_amdgcn_mov_dpp(x, 0x128, 0xf, 0xf, true);     // row_ror:8
    else if constexpr (R == 4) {
        // odd rows of the first operand <-> even rows of the second: {r0, r0, r2, r2} and {r1, r1, r3, r3}
        const u32x2 r = __builtin_amdgcn_permlane16_swap((unsigned)x, (unsigned)x, false, false);
        return (int)((lane & 16u) ? r[0] : r[1]);
    } else {
        // rows 2, 3 of the first operand <-> rows 0, 1 of the second: {lo, lo} and {hi, hi}
        const u32x2 r = __builtin_amdgcn_permlane32_swap((unsigned)x, (unsigned)x, false, false);
        return (int)((lane & 32u) ? r[0] : r[1]);
    }
}

// The forward pass keeps the metrics in a rotating lane layout so that a trellis step needs no LDS: in layout r bit i of
// a state sits at lane bit (r + i) mod (K - 1).  The predecessors 2x and 2x + 1 of the states x and x + S / 2 are then
// the lane pair that differs in bit r; the lane with bit r == b holds p_b, computes the state with u = b in place, and
// the layout becomes r + 1.  Step w of a window runs in layout w mod (K - 1) (all metrics start at 0, so the first layout
// is free to choose).
// A group is the K - 1 steps from layout 0 back to layout 0.  Each step rewrites only bit r of the survivor's lane, so at
// the end of a group the lane index IS the group's K - 1 input bits, in order.  Beside its metric a lane carries `anc`,
// the lane its survivor sat in when the group began (it travels with the survivor: one more exchange and select per
// step).  What is stored is anc, K - 1 bits per group and lane, 32 / (K - 1) groups to a dword: the traceback is one
// dependent LDS read per GROUP -- the bits are the lane, the next lane is anc -- and not one per step.
template <int K, int R>
__device__ __forceinline__ void acs_step(int &m, unsigned &anc, int v, const int (&pat_own)[K - 1], const int (&pat_par)[K - 1], unsigned lane)
{
    const int other = partner<R>(m, lane);
    const unsigned oanc = (unsigned)partner<R>((int)anc, lane);
    const int c_own = __builtin_amdgcn_sdot4(pat_own[R], v, m, false), c_par = __builtin_amdgcn_sdot4(pat_par[R], v, other, false);
    // p1 is taken only if cand_1 > cand_0: the lane with bit R clear owns p0 and keeps it on a tie (c_own + 1 > c_par),
    // the other owns p1 (c_own > c_par); as one integer compare, the metrics being far from overflow
    const bool own = c_own + (int)(~(lane >> R) & 1u) > c_par;
    m = own ? c_own : c_par;
    anc = own ? anc : oanc;
}

// the steps of one group in a straight line (no branch between them: a taken branch per step costs more than the step);
// FULL: all K - 1 of them, else the first `lim` (the end of a window)
template <int K, bool FULL>
__device__ __forceinline__ void acs_group(int &m, unsigned &anc, const int (&v)[K - 1], const int (&pat_own)[K - 1],
                                          const int (&pat_par)[K - 1], unsigned lane, unsigned lim)
{
    constexpr int NR = K - 1;
    if (FULL || lim > 0) acs_step<K, 0>(m, anc, v[0], pat_own, pat_par, lane);
    if (FULL || lim > 1) acs_step<K, 1>(m, anc, v[1], pat_own, pat_par, lane);
    if constexpr (NR > 2) { if (FULL || lim > 2) acs_step<K, 2>(m, anc, v[2], pat_own, pat_par, lane); }
    if constexpr (NR > 3) { if (FULL || lim > 3) acs_step<K, 3>(m, anc, v[3], pat_own, pat_par, lane); }
    if constexpr (NR > 4) { if (FULL || lim > 4) acs_step<K, 4>(m, anc, v[4], pat_own, pat_par, lane); }
    if constexpr (NR > 5) { if (FULL || lim > 5) acs_step<K, 5>(m, anc, v[5], pat_own, pat_par, lane); }
}

template <int K> __global__ __launch_bounds__(kWave) void cc_decode_kernel(DecodeCall a)
{
    constexpr int S = 1 << (K - 1);                 // states = lanes per block
    constexpr int G = kWave / S;                    // blocks per wave
    constexpr int NR = K - 1;                       // layouts = steps per group
    constexpr int GPD = 32 / NR;                    // groups per dword
    constexpr int RS = GPD * NR;                    // steps per LDS row
    extern __shared__ __attribute__((aligned(16))) uint32_t dec[];       // [ceil((W - q0) / RS)][64]

    const unsigned lane = threadIdx.x;
    const unsigned j = lane & (S - 1), gbase = lane & ~(unsigned)(S - 1);
    const uint64_t rel = (uint64_t)blockIdx.x * G + lane / S;            // the group's block within the launch
    const bool present = rel < a.nb;
    const uint64_t blk = a.b0 + rel;
    const int64_t s0 = (int64_t)(blk * a.D) - (int64_t)(a.T + a.A);      // the window's first step
    const unsigned W = a.A + a.T + a.dlen;
    const unsigned q0 = (a.A / NR) * NR;            // the first step whose group is stored: the groups inside the warm-up are not

    // the state lane j holds in layout r, and its patterns there: byte q = 1 - 2 c_q(u, p) with u = bit 0 of the state
    auto state_in = [&](unsigned r) { return ((j >> r) | (j << (NR - r))) & (unsigned)(S - 1); };
    int pat_own[NR], pat_par[NR];
#pragma unroll
    for (int r = 0; r < NR; r++) {
        const unsigned p = state_in((unsigned)r);
        pat_own[r] = pattern(a.code, p & 1u, p);
        pat_par[r] = pattern(a.code, p & 1u, p ^ 1u);
    }

    // a round is RL steps, a whole number of groups: lane j < RL of a group of lanes holds the soft values of step w0 + j
    constexpr unsigned RL = (unsigned)(S / NR) * NR, GR = RL / NR;
    auto fetch = [&](unsigned w) { return (present && j < RL && w < W) ? load_step(a, s0 + (int64_t)w) : RawStep{0, 0, 0}; };

    int m = 0;
    unsigned anc = j, packw = 0, tail = 0, gi = 0, row = 0;
    RawStep nxt = fetch(j);
    for (unsigned w0 = 0; w0 < W; w0 += RL) {
        asm volatile("" : "+v"(nxt.lo), "+v"(nxt.b2), "+v"(nxt.b3));     // this round's values have arrived ...
        const int cur = pack(nxt, a.code.n);
        nxt = fetch(w0 + RL + j);                                         // ... and the next round's loads fly under its steps
        const unsigned left = W - w0, ng = left >= RL ? GR : left / (unsigned)NR;
        auto bcast = [&](int (&v)[NR], unsigned i0) {                     // the NR soft dwords of a group: off the metrics' chain
#pragma unroll
            for (int t = 0; t < NR; t++) {
                if constexpr (S == kWave) v[t] = __builtin_amdgcn_readlane(cur, (int)(i0 + t));
                else v[t] = __builtin_amdgcn_ds_bpermute((int)(4 * (gbase + i0 + t)), cur);
            }
        };
        for (unsigned gg = 0; gg < ng; gg++) {
            int v[NR];
            bcast(v, gg * NR);
            acs_group<K, true>(m, anc, v, pat_own, pat_par, lane, NR);
            if (w0 + gg * NR >= q0) {                                     // the group is stored
                packw |= anc << (gi * NR);
                if (++gi == (unsigned)GPD) { dec[row * kWave + lane] = packw; packw = 0; gi = 0; row++; }
            }
            anc = j;
        }
        if (left < RL && left > ng * NR) {                                // the window ends inside a group
            int v[NR];
            tail = left - ng * NR;
            bcast(v, ng * NR);                                            // ng NR + NR <= RL: lanes past the window hold zeros
            acs_group<K, false>(m, anc, v, pat_own, pat_par, lane, tail);
            packw |= anc << (gi * NR);
            gi++;
        }
    }
    if (gi != 0) dec[row * kWave + lane] = packw;
    const unsigned r = tail;                                              // the window ends in layout W mod (K - 1)

    // the state with the largest metric, ties to the smallest state (the window ends in layout r = W mod (K - 1)); every
    // lane of a group ends with the same (metric, state, lane)
    int bm = m;
    unsigned bs = state_in(r), bl = j;
#pragma unroll
    for (int x = S / 2; x >= 1; x >>= 1) {
        const int om = __shfl_xor(bm, x, S);
        const unsigned os = (unsigned)__shfl_xor((int)bs, x, S), ol = (unsigned)__shfl_xor((int)bl, x, S);
        if (om > bm || (om == bm && os < bs)) { bm = om; bs = os; bl = ol; }
    }
    __syncthreads();

    if (j == 0 && present) {
        // group g holds steps q0 + g NR ..: bit t of the survivor's lane at its end is u of step q0 + g NR + t, i.e. bit
        // (g % GPD) NR + t of row g / GPD.  (The last group may be short: its upper bits belong to no step and are never read.)
        unsigned l = bl, acc = 0;
        for (int g = (int)((W - 1 - q0) / NR); g >= 0; g--) {
            const unsigned grow = (unsigned)g / GPD, sh = ((unsigned)g % GPD) * NR;
            const unsigned wd = dec[grow * kWave + gbase + l];
            acc |= l << sh;
            l = (wd >> sh) & (unsigned)(S - 1);
            if (sh == 0) { dec[grow * kWave + gbase] = acc; acc = 0; }    // row finished: nobody reads it again
        }
    }
    __syncthreads();

    // out[blk D + i] is the decision for window step A + i
    for (int g = 0; g < G; g++) {
        const uint64_t rb = (uint64_t)blockIdx.x * G + g;
        if (rb >= a.nb) break;
        uint8_t *o = a.out + (a.b0 + rb) * a.D;
        for (unsigned i = lane; i < a.dlen; i += kWave) {
            const unsigned q = a.A + i - q0;
            o[i] = (uint8_t)((dec[(q / RS) * kWave + g * S] >> (q % RS)) & 1u);
        }
    }
}

// one lane per input bit: k input bytes in, n coded bytes out
template <int N> __global__ __launch_bounds__(kBlock) void cc_encode_kernel(const uint8_t *hist, const uint8_t *bits, uint8_t *coded,
                                                                            size_t nbits, CcCode c)
{
    const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= nbits) return;
    unsigned reg = 0;
    for (unsigned i = 0; i < c.k; i++) {                                  // u[t - i] at bit k - 1 - i
        unsigned b = 0;
        if (t >= i) b = bits[t - i];
        else if (hist) b = hist[(c.k - 1) - (i - t)];
        reg |= (b & 1u) << (c.k - 1 - i);
    }
#pragma unroll
    for (int q = 0; q < N; q++) coded[t * N + q] = (uint8_t)(__popc(reg & c.poly[q]) & 1);
}

// the decoder's dynamic LDS: one dword per lane and row of (32 / (k - 1)) groups of k - 1 steps, from the group that holds step A
size_t dec_lds_bytes(uint32_t k, uint32_t A, uint32_t T, uint32_t dlen)
{
    const uint32_t nr = k - 1, rs = (32u / nr) * nr, q0 = (A / nr) * nr;
    return (size_t)((A + T + dlen - q0 + rs - 1) / rs) * kWave * sizeof(uint32_t);
}

}  // namespace

struct aeth_cc {
    aeth_ctx *ctx;
    CcCode code;
    uint32_t D, A, T;
};

namespace {

int launch_decode(aeth_cc *cc, DecodeCall &a)
{
    const unsigned G = kWave >> (cc->code.k - 1);
    const dim3 grid((unsigned)((a.nb + G - 1) / G)), block(kWave);
    const size_t lds = dec_lds_bytes(cc->code.k, a.A, a.T, a.dlen);
    hipStream_t st = aeth::ctx_stream(cc->ctx);
    switch (cc->code.k) {
    case 3: hipLaunchKernelGGL(cc_decode_kernel<3>, grid, block, lds, st, a); break;
    case 4: hipLaunchKernelGGL(cc_decode_kernel<4>, grid, block, lds, st, a); break;
    case 5: hipLaunchKernelGGL(cc_decode_kernel<5>, grid, block, lds, st, a); break;
    case 6: hipLaunchKernelGGL(cc_decode_kernel<6>, grid, block, lds, st, a); break;
    default: hipLaunchKernelGGL(cc_decode_kernel<7>, grid, block, lds, st, a); break;
    }
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

}  // namespace

extern "C" {

int aeth_cc_create(aeth_ctx *ctx, const aeth_cc_code *code, size_t block, size_t warmup, size_t traceback, aeth_cc **out)
{
    AETH_REQUIRE(out, AETH_E_ARG, "out is null");
    *out = nullptr;
    AETH_REQUIRE(ctx, AETH_E_ARG, "ctx is null");
    AETH_REQUIRE(code, AETH_E_ARG, "code is null");
    AETH_REQUIRE(code->k != 8 && code->k != 9, AETH_E_UNSUPPORTED,
                 "k %u: constraint lengths 3 .. 7 are built (one state per lane); 8 and 9 are not", code->k);
    AETH_REQUIRE(code->k >= 3 && code->k <= 7, AETH_E_ARG, "k %u outside 3 .. 7", code->k);
    AETH_REQUIRE(code->n >= 2 && code->n <= 4, AETH_E_ARG, "n %u outside 2 .. 4", code->n);
    for (uint32_t q = 0; q < code->n; q++)
        AETH_REQUIRE(code->poly[q] > 0 && code->poly[q] < (1u << code->k), AETH_E_ARG, "poly[%u] %u outside 1 .. 2^%u - 1", q,
                     code->poly[q], code->k);
    AETH_REQUIRE(block >= 1, AETH_E_ARG, "block %zu: at least 1", block);
    AETH_REQUIRE(block <= kMaxSpan && traceback <= kMaxSpan - block, AETH_E_ARG, "block %zu + traceback %zu = %zu: at most %u", block,
                 traceback, block + traceback, kMaxSpan);
    AETH_REQUIRE(warmup <= kMaxSpan, AETH_E_ARG, "warmup %zu: at most %u", warmup, kMaxSpan);
    aeth_cc *cc = new (std::nothrow) aeth_cc{};
    AETH_REQUIRE(cc, AETH_E_NOMEM, "out of host memory");
    cc->ctx = ctx;
    cc->code.k = code->k;
    cc->code.n = code->n;
    for (uint32_t q = 0; q < 4; q++) cc->code.poly[q] = q < code->n ? code->poly[q] : 0;
    cc->D = (uint32_t)block; cc->A = (uint32_t)warmup; cc->T = (uint32_t)traceback;
    *out = cc;
    return AETH_OK;
}

int aeth_cc_destroy(aeth_cc *cc)
{
    delete cc;
    return AETH_OK;
}

size_t aeth_cc_k(const aeth_cc *cc) { return cc ? cc->code.k : 0; }
size_t aeth_cc_n(const aeth_cc *cc) { return cc ? cc->code.n : 0; }
size_t aeth_cc_block(const aeth_cc *cc) { return cc ? cc->D : 0; }
size_t aeth_cc_warmup(const aeth_cc *cc) { return cc ? cc->A : 0; }
size_t aeth_cc_traceback(const aeth_cc *cc) { return cc ? cc->T : 0; }
size_t aeth_cc_history(const aeth_cc *cc) { return cc ? (size_t)cc->A + cc->T : 0; }

int aeth_cc_encode(aeth_cc *cc, const uint8_t *hist_bits_dev, const uint8_t *bits_dev, size_t nbits, uint8_t *coded_dev, size_t ncoded)
{
    AETH_REQUIRE(cc, AETH_E_ARG, "cc is null");
    const size_t n = cc->code.n;
    AETH_REQUIRE(nbits <= SIZE_MAX / n && ncoded == nbits * n, AETH_E_LEN, "output holds %zu coded bits, %zu bits x %zu give %zu", ncoded,
                 nbits, n, nbits <= SIZE_MAX / n ? nbits * n : (size_t)0);
    if (nbits == 0) return AETH_OK;
    AETH_REQUIRE(bits_dev && coded_dev, AETH_E_ARG, "null pointer");
    if (int rc = aeth::check_disjoint({{bits_dev, nbits}, {hist_bits_dev, cc->code.k - 1}}, {{coded_dev, ncoded}})) return rc;
    const size_t blocks = (nbits + kBlock - 1) / kBlock;
    AETH_REQUIRE(blocks < ((size_t)1 << 31), AETH_E_UNSUPPORTED, "%zu bits need 2^31 workgroups or more", nbits);
    aeth::DeviceGuard dg(cc->ctx->device);
    const dim3 grid((unsigned)blocks), block(kBlock);
    hipStream_t st = aeth::ctx_stream(cc->ctx);
    switch (n) {
    case 2: hipLaunchKernelGGL(cc_encode_kernel<2>, grid, block, 0, st, hist_bits_dev, bits_dev, coded_dev, nbits, cc->code); break;
    case 3: hipLaunchKernelGGL(cc_encode_kernel<3>, grid, block, 0, st, hist_bits_dev, bits_dev, coded_dev, nbits, cc->code); break;
    default: hipLaunchKernelGGL(cc_encode_kernel<4>, grid, block, 0, st, hist_bits_dev, bits_dev, coded_dev, nbits, cc->code); break;
    }
    AETH_HIP(hipGetLastError());
    return AETH_OK;
}

int aeth_cc_decode(aeth_cc *cc, const int8_t *hist_soft_dev, const int8_t *soft_dev, size_t nsoft, uint8_t *bits_dev, size_t nbits)
{
    AETH_REQUIRE(cc, AETH_E_ARG, "cc is null");
    const size_t n = cc->code.n;
    AETH_REQUIRE(nbits <= SIZE_MAX / n && nsoft == nbits * n, AETH_E_LEN, "input holds %zu soft values, %zu bits x %zu need %zu", nsoft,
                 nbits, n, nbits <= SIZE_MAX / n ? nbits * n : (size_t)0);
    if (nbits == 0) return AETH_OK;
    AETH_REQUIRE(soft_dev && bits_dev, AETH_E_ARG, "null pointer");
    const size_t nhist = ((size_t)cc->A + cc->T) * n;
    if (int rc = aeth::check_disjoint({{soft_dev, nsoft}, {hist_soft_dev, nhist}}, {{bits_dev, nbits}})) return rc;
    const size_t nfull = nbits / cc->D, tail = nbits % cc->D;
    const unsigned G = kWave >> (cc->code.k - 1);
    AETH_REQUIRE((nfull + G - 1) / G < ((size_t)1 << 31), AETH_E_UNSUPPORTED, "%zu bits in blocks of %u need 2^31 workgroups or more", nbits,
                 cc->D);
    aeth::DeviceGuard dg(cc->ctx->device);
    DecodeCall a{hist_soft_dev, soft_dev, bits_dev, cc->code, 0, nfull, cc->D, cc->A, cc->T, cc->D};
    if (nfull) { int rc = launch_decode(cc, a); if (rc) return rc; }
    if (tail) {
        a.b0 = nfull; a.nb = 1; a.dlen = (uint32_t)tail;
        int rc = launch_decode(cc, a); if (rc) return rc;
    }
    return AETH_OK;
}

}  // extern "C"
