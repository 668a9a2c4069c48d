// fir_lab.hip -- A/B bench of the fused FIR kernel (aeth_fir_kernel.h) on the C3 geometry: FFT-2048, 64 taps,
// 16 Mi samples per launch, buffers rotating over 1.5 GiB.  Rows = a kernel variant (base, prio, xor, xor+prio,
// xor+prio+spread, and the 256-lane two-block configuration "x2") x a launch mode (one queue, any-order, 2 / 3 / 4 / 6
// queues, two queues with the library's event protocol) x a grid.  Interleaved rounds in one process (cdna guide
// rule 24); every row's output is compared bit for bit with variant 0 and variant 0 with an f64 direct convolution
// on sampled outputs.  The rows of variants that left the kernel are on record in profiles/r0*_fir_lab_*.txt.
// The "pol:" rows are builds of the same template with another cache policy on the stream accesses (see LabPol below;
// profiles/fir_policy_lab.txt).
//
// build (from the repo root):
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -ffp-contract=fast -Iaether_primitives_amd/csrc tools/fir_lab.hip \
//         -o tools/bin/fir_lab -Laether_primitives_amd/lib -laether_hip -Wl,-rpath,'$ORIGIN/../../aether_primitives_amd/lib'
//   (-DLAB_COMBO=body,halo,store,rule,order[,mask] adds the cell "pol:combo", -DLAB_COMBO2=... "pol:combo2")
// run:  tools/bin/fir_lab [steps=300] [rounds=5] [name ...]      (no names: every variant; @2q / @1q: every policy
//       cell's two-queue / one-queue row)
#include "aeth_fft_plan.h"
#include "aeth_fir_kernel.h"

#include <hip/hip_ext.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

using namespace aeth::firk;
using C2048 = CfgFor<2048>::type;
using C2048x2 = Cfg<2048, 16, 16, 16, 8, 1, 256>;   // two blocks per 256-lane workgroup: one wave on every SIMD

// ---- cache-policy cells (profiles/fir_policy_lab.txt) -------------------------------------------------------------
// The kernel asks StreamPolicy<C> (aeth_fir_kernel.h) how a window slot is loaded, in which order a burst issues its
// slots and what the sample stores carry; the library's configurations take the primary template, the shipped rule.  A
// lab configuration is the same Cfg with a LabPolicy member, for which the specialisation below answers instead: body
// and halo load aux, sample store aux (1 = sc0, 2 = nt, 16 = sc1), the halo rule (slot-coarse: the first and the last
// slot; wave-exact: of those two slots only the wave whose 64 elements lie in the halo, wave 0 of slot 0 and the last
// wave of the last slot, chosen by a wave-uniform branch with one load on either side) and the burst order (0: slots
// 0 ... P-1; 1: the last slot first and slot 0 last; 2: slot 0 first and the last slot second).  The builds differ in
// nothing else, so every cell is timed beside the others in one process.
// RULE: 0 slot-coarse, 1 wave-exact, 2 the wave-exact branch with its sides swapped (the half of the slot that is NOT
// shared takes the halo policy: what the branch itself costs, and whether the gain is the shared half's at all).
// MASK: the slots that take the halo policy, bit m = slot m (default: the first and the last, where the halo of up to
// 129 taps lies) -- cells that give it to slots no other workgroup reads ask the same question from the other side, and
// the sweep over how many slots take it is what plain_slots() in aeth_fir_kernel.h was chosen from.
template <int BODY, int HALO, int STORE, int RULE, int ORDER, unsigned MASK = 0x8001u>
struct LabPol {
    static constexpr int body = BODY, halo = HALO, store = STORE, rule = RULE, order = ORDER;
    static constexpr unsigned mask = MASK;
};
template <class Pol> struct LabCfg : C2048 { using LabPolicy = Pol; };

namespace aeth {
namespace firk {
template <class C>
struct StreamPolicy<C, std::void_t<typename C::LabPolicy>> {
    using L = typename C::LabPolicy;
    static constexpr int store = L::store;
    static constexpr int slot(int i)
    {
        if (L::order == 1) return i == 0 ? C::P - 1 : i == C::P - 1 ? 0 : i;
        if (L::order == 2) return i == 0 ? 0 : i == 1 ? C::P - 1 : i - 1;
        return i;
    }
    template <bool NT, class RS>
    static __device__ __forceinline__ cf load(RS rs, int tid, int m)
    {
        const int off = (tid + m * C::T) * 8;
        if ((L::mask >> m) & 1) {
            if constexpr (NT && L::rule != 0 && C::T > 64) {
                if (m == 0 || m == C::P - 1) {
                    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
                    if ((wave != (m == 0 ? 0 : C::T / 64 - 1)) == (L::rule == 1))
                        return as_cf(__builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, L::body));
                }
            }
            return as_cf(__builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, NT ? L::halo : 0));
        }
        return as_cf(__builtin_amdgcn_raw_buffer_load_b64(rs, off, 0, NT ? L::body : 0));
    }
};
}  // namespace firk
}  // namespace aeth

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); exit(2); } } while (0)
#define AK(x) do { int r_ = (x); if (r_ != 0) { fprintf(stderr, "aeth error %d (%s) at %s:%d\n", r_, aeth_last_error(), __FILE__, __LINE__); exit(2); } } while (0)

static const size_t NS = (size_t)1 << 24;
static const int NBUF = 6;

struct Variant {
    const char *name;
    int var;          // kernel template VAR (1000: variant 0 of the 256-lane two-block configuration)
    int mode;         // 0 plain launch, 1 hipExtAnyOrderLaunch, 2 two streams alternating, 3 the same with the library's event protocol,
                      // 4 / 5 / 6: three / four / six streams round-robin (no events: the lab's buffers make the launches independent)
    int grid;         // 0 = default
    void (*pol)(const FmiArgs &, int, hipStream_t) = nullptr;     // a policy cell: its own build (var is what it was cut from)
};

template <class P, int VAR>
static void launch_pol(const FmiArgs &a, int grid, hipStream_t s)
{
    hipLaunchKernelGGL((fmi_kernel<LabCfg<P>, false, 1, true, false, VAR>), dim3(grid), dim3(C2048::WG), 0, s, a);
}

// One cell = two rows: the burst build on two queues with the chained grid (12/16 of the resident one, the library's
// steady state) and the spread build on one queue with the full grid (the build a lone launch takes).
#define POL_CELL(NAME, ...)                                                                                        \
    {NAME "/g768/2q", 2052, 2, 768, launch_pol<LabPol<__VA_ARGS__>, V_XOR | V_PRIO>},                                \
    {NAME "/spread/1q", 18436, 0, 0, launch_pol<LabPol<__VA_ARGS__>, V_SPREAD | V_XOR | V_PRIO>}

template <int VAR>
static void launch_var2(const FmiArgs &a, int grid, hipStream_t s)
{
    hipLaunchKernelGGL((fmi_kernel<C2048x2, false, 1, true, false, VAR>), dim3(grid), dim3(C2048x2::WG), 0, s, a);
}

template <int VAR>
static void launch_var(const FmiArgs &a, int grid, hipStream_t s, int any_order)
{
    if (any_order) {
        hipExtLaunchKernelGGL((fmi_kernel<C2048, false, 1, true, false, VAR>), dim3(grid), dim3(C2048::WG), 0, s, nullptr, nullptr,
                              hipExtAnyOrderLaunch, a);
    } else {
        hipLaunchKernelGGL((fmi_kernel<C2048, false, 1, true, false, VAR>), dim3(grid), dim3(C2048::WG), 0, s, a);
    }
}

static void launch(int var, const FmiArgs &a, int grid, hipStream_t s, int any_order)
{
    switch (var) {
    case 1000: launch_var2<0>(a, grid, s); break;
    case 0: launch_var<0>(a, grid, s, any_order); break;
    case 4: launch_var<V_PRIO>(a, grid, s, any_order); break;
    case 2048: launch_var<V_XOR>(a, grid, s, any_order); break;
    case 2052: launch_var<V_XOR | V_PRIO>(a, grid, s, any_order); break;
    case 18436: launch_var<V_SPREAD | V_XOR | V_PRIO>(a, grid, s, any_order); break;
    default: fprintf(stderr, "variant %d not instantiated\n", var); exit(2);
    }
}

int main(int argc, char **argv)
{
    int steps = argc > 1 ? atoi(argv[1]) : 300;
    int rounds = argc > 2 ? atoi(argv[2]) : 5;
    std::vector<Variant> all = {
        {"base", 0, 0, 0},
        {"prio", 4, 0, 0},
        {"base/anyorder", 0, 1, 0},
        {"base/2q", 0, 2, 0},
        {"base/g960", 0, 0, 960},
        {"base/g768", 0, 0, 768}, {"base/g512", 0, 0, 512}, {"base/g256", 0, 0, 256},
        {"x2", 1000, 0, 512},
        {"base/g1280", 0, 0, 1280}, {"base/g1536", 0, 0, 1536}, {"base/g2048", 0, 0, 2048}, {"base/g3072", 0, 0, 3072}, {"base/g4229", 0, 0, 4229}, {"base/g8457", 0, 0, 8457},
        {"base/g2048/2q", 0, 2, 2048}, {"base/g4229/2q", 0, 2, 4229},
        {"prio/2q+events", 4, 3, 0}, {"base/2q+events", 0, 3, 0},
        {"xor", 2048, 0, 0}, {"xor+prio", 2052, 0, 0}, {"xor+prio/2q", 2052, 2, 0},
        {"xor+prio+spread", 18436, 0, 0}, {"xor+prio+spread/2q", 18436, 2, 0}, {"xor+prio+spread/g768/2q", 18436, 2, 768},
        {"xor+prio/g768/3q", 2052, 4, 768}, {"xor+prio/g768/4q", 2052, 5, 768}, {"xor+prio/g768/6q", 2052, 6, 768},
        {"xor+prio/g640/3q", 2052, 4, 640}, {"xor+prio/g640/4q", 2052, 5, 640}, {"xor+prio/g512/3q", 2052, 4, 512}, {"xor+prio/g512/4q", 2052, 5, 512},
        {"xor+prio/g896/3q", 2052, 4, 896}, {"xor+prio/g1024/3q", 2052, 4, 0}, {"xor+prio/g1024/4q", 2052, 5, 0},
        {"xor+prio/g384/4q", 2052, 5, 384}, {"xor+prio/g384/6q", 2052, 6, 384}, {"xor+prio/g512/6q", 2052, 6, 512},
        {"xor+prio/g768/2q", 2052, 2, 768}, {"xor+prio/g896/2q", 2052, 2, 896}, {"xor+prio/g768", 2052, 0, 768},
        {"xor+prio/g704/2q", 2052, 2, 704}, {"xor+prio/g736/2q", 2052, 2, 736}, {"xor+prio/g800/2q", 2052, 2, 800},
        {"xor+prio/g832/2q", 2052, 2, 832}, {"xor+prio/g960/2q", 2052, 2, 960},
        // 8457 blocks = 11 x 768 + 9 -- grids that divide the stream into whole rounds (769: 11 rounds, 705: 12, 846: 10)
        {"xor+prio/g769/2q", 2052, 2, 769}, {"xor+prio/g705/2q", 2052, 2, 705}, {"xor+prio/g846/2q", 2052, 2, 846},
        {"prio/2q", 4, 2, 0},
        // policy cells, one factor at a time (body load, halo load, sample store, halo rule, order) from the point that was
        // shipped when profiles/fir_policy_lab.txt was taken, where this cell is called "pol:shipped": nt loads, plain
        // on slots 0 and 15, nt + sc1 stores
        POL_CELL("pol:plain-slots-0-15", 2, 0, 18, 0, 0),
        POL_CELL("pol:body0", 0, 0, 18, 0, 0), POL_CELL("pol:body16", 16, 0, 18, 0, 0), POL_CELL("pol:body18", 18, 0, 18, 0, 0),
        POL_CELL("pol:halo16", 2, 16, 18, 0, 0), POL_CELL("pol:halo1", 2, 1, 18, 0, 0),
        POL_CELL("pol:store2", 2, 0, 2, 0, 0), POL_CELL("pol:store0", 2, 0, 0, 0, 0), POL_CELL("pol:store16", 2, 0, 16, 0, 0),
        POL_CELL("pol:wave-exact", 2, 0, 18, 1, 0),
        POL_CELL("pol:order-15-first-0-last", 2, 0, 18, 0, 1), POL_CELL("pol:order-0-first-15-second", 2, 0, 18, 0, 2),
        // whose gain is the plain pair of slots?  The branch of the wave-exact rule with its sides swapped, and the halo
        // policy on other sets of slots: one of the two, two that nobody shares, four and eight of the sixteen
        POL_CELL("pol:wave-swapped", 2, 0, 18, 2, 0),
        POL_CELL("pol:plain-slot-0", 2, 0, 18, 0, 0, 0x0001u), POL_CELL("pol:plain-slot-15", 2, 0, 18, 0, 0, 0x8000u),
        POL_CELL("pol:plain-slots-7-8", 2, 0, 18, 0, 0, 0x0180u), POL_CELL("pol:plain-slots-0-1-14-15", 2, 0, 18, 0, 0, 0xC003u),
        POL_CELL("pol:plain-slots-0-4-8-12", 2, 0, 18, 0, 0, 0x1111u), POL_CELL("pol:plain-even-slots", 2, 0, 18, 0, 0, 0x5555u),
        // ... it is the share of plain loads, not the sharing: how many of the sixteen, and does their place matter
        POL_CELL("pol:plain-slots-0-8-15", 2, 0, 18, 0, 0, 0x8101u), POL_CELL("pol:plain-slots-0-1-15", 2, 0, 18, 0, 0, 0x8003u),
        POL_CELL("pol:plain-slots-0-5-10-15", 2, 0, 18, 0, 0, 0x8421u), POL_CELL("pol:plain-slots-0-7-8-15", 2, 0, 18, 0, 0, 0x8181u),
        POL_CELL("pol:plain-slots-0-3-6-9-12", 2, 0, 18, 0, 0, 0x1249u), POL_CELL("pol:plain-slots-0-1-2-14-15", 2, 0, 18, 0, 0, 0xC007u),
        POL_CELL("pol:plain-slots-0-3-6-9-12-15", 2, 0, 18, 0, 0, 0x9249u), POL_CELL("pol:plain-slots-0-1-2-13-14-15", 2, 0, 18, 0, 0, 0xE007u),
        // each factor's best together: the values come from the table above, -DLAB_COMBO=body,halo,store,rule,order
#ifdef LAB_COMBO
        POL_CELL("pol:combo", LAB_COMBO),
#endif
#ifdef LAB_COMBO2
        POL_CELL("pol:combo2", LAB_COMBO2),
#endif
    };
    std::vector<Variant> vs;
    if (argc > 3) {
        for (int i = 3; i < argc; i++) {
            bool found = false;
            // "@2q" / "@1q": every policy cell's two-queue / one-queue row, in the table's order
            if (!strcmp(argv[i], "@2q") || !strcmp(argv[i], "@1q")) {
                for (auto &v : all) if (v.pol && (v.mode == 2) == (argv[i][1] == '2')) { vs.push_back(v); found = true; }
                if (found) continue;
            }
            for (auto &v : all) if (!strcmp(v.name, argv[i])) { vs.push_back(v); found = true; }
            if (!found) { fprintf(stderr, "unknown variant %s\n", argv[i]); return 2; }
        }
    } else vs = all;

    aeth_ctx *ctx = nullptr;
    AK(aeth_ctx_create(0, &ctx));
    hipStream_t s0 = (hipStream_t)aeth_ctx_stream(ctx), s1, sx[6];
    CK(hipStreamCreateWithFlags(&s1, hipStreamNonBlocking));
    sx[0] = s0; sx[1] = s1;
    for (int i = 2; i < 6; i++) CK(hipStreamCreateWithFlags(&sx[i], hipStreamNonBlocking));

    // taps: 64-tap Hamming-windowed sinc, unit DC gain (bench.py lowpass_taps)
    const int NT_ = 64;
    std::vector<aeth_cf32> taps(NT_);
    {
        std::vector<double> t(NT_);
        double sum = 0;
        for (int k = 0; k < NT_; k++) {
            double m = k - (NT_ - 1) / 2.0;
            double sinc = std::sin(2 * M_PI * 0.25 * m) / (M_PI * m);
            double w = 0.54 - 0.46 * std::cos(2 * M_PI * k / (NT_ - 1));
            t[k] = sinc * w; sum += t[k];
        }
        for (int k = 0; k < NT_; k++) taps[k] = aeth_cf32{(float)(t[k] / sum), 0.f};
    }
    aeth_fir *fir = nullptr;
    AK(aeth_fir_create(ctx, taps.data(), NT_, 2048, &fir));

    // input: deterministic pseudo-random cf32 in [-1, 1)
    std::vector<aeth_cf32> x(NS);
    {
        uint64_t st = 0x9E3779B97F4A7C15ull;
        for (size_t i = 0; i < NS; i++) {
            st = st * 6364136223846793005ull + 1442695040888963407ull;
            uint32_t a = (uint32_t)(st >> 40), b = (uint32_t)(st >> 16) & 0xFFFFFF;
            x[i] = aeth_cf32{(float)a / 8388608.0f - 1.0f, (float)b / 8388608.0f - 1.0f};
        }
    }
    float2 *in[NBUF], *out[NBUF];
    for (int i = 0; i < NBUF; i++) {
        CK(hipMalloc((void **)&in[i], NS * 8));
        CK(hipMalloc((void **)&out[i], NS * 8));
        CK(hipMemcpy(in[i], x.data(), NS * 8, hipMemcpyHostToDevice));
        CK(hipMemset(out[i], 0xFF, NS * 8));
    }

    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int cap = prop.multiProcessorCount * 8 / (C2048::WG / 64);
    auto args_for = [&](int b) {
        FmiArgs a;
        a.in = (const cf *)in[b]; a.out = (cf *)out[b]; a.hist = nullptr; a.Hf = (const cf *)fir->Hf;
        a.twN = (const cf *)fir->fft->tw_dev; a.twL = (const cf *)fir->fft->tw_lane_dev;
        a.n = (long long)NS; a.hop = (int)fir->hop; a.ov = (int)(fir->fft_len - fir->hop); a.nhist = (int)(fir->ntaps - 1);
        a.nblocks = (long long)((NS + fir->hop - 1) / fir->hop);
        a.s_fwd = 1.0f; a.s_bwd = 1.0f; a.frame_n = 2048;
        return a;
    };
    hipEvent_t ev_pre[2];
    CK(hipEventCreateWithFlags(&ev_pre[0], hipEventDisableTiming)); CK(hipEventCreateWithFlags(&ev_pre[1], hipEventDisableTiming));
    CK(hipEventRecord(ev_pre[0], s0)); CK(hipEventRecord(ev_pre[1], s1));
    auto issue = [&](const Variant &v, int i) {
        const int grid = v.grid ? v.grid : cap;
        const int nq = v.mode == 4 ? 3 : v.mode == 5 ? 4 : v.mode == 6 ? 6 : (v.mode >= 2 ? 2 : 1);
        const int lane = i % nq;
        hipStream_t s = sx[lane];
        if (v.mode == 3) {       // aeth_runtime.hip: ctx_fir_lane -- wait for the other lane's history, record this lane's
            CK(hipStreamWaitEvent(s, ev_pre[1 - lane], 0));
            CK(hipEventRecord(ev_pre[lane], s));
        }
        if (v.pol) v.pol(args_for(i % NBUF), grid, s);
        else launch(v.var, args_for(i % NBUF), grid, s, v.mode == 1);
    };
    auto sync_all = [&] { for (int i = 0; i < 6; i++) CK(hipStreamSynchronize(sx[i])); };

    // correctness: variant 0 against an f64 direct convolution on sampled outputs, every variant against variant 0
    std::vector<aeth_cf32> ref(NS), got(NS);
    issue(all[0], 0); sync_all(); CK(hipGetLastError());
    CK(hipMemcpy(ref.data(), out[0], NS * 8, hipMemcpyDeviceToHost));
    {
        double e2 = 0, r2 = 0;
        auto check = [&](size_t n0) {
            double re = 0, im = 0;
            for (int k = 0; k < NT_; k++) {
                if (n0 < (size_t)k) break;
                re += (double)taps[k].re * x[n0 - k].re; im += (double)taps[k].re * x[n0 - k].im;
            }
            double dr = ref[n0].re - re, di = ref[n0].im - im;
            e2 += dr * dr + di * di; r2 += re * re + im * im;
        };
        for (size_t n0 = 0; n0 < 6000; n0++) check(n0);
        for (size_t n0 = NS - 6000; n0 < NS; n0++) check(n0);
        for (size_t j = 0; j < 200000; j++) check((j * 2654435761ull) % NS);
        printf("variant 0 vs f64 direct convolution: EVM %.1f dB\n", 10 * std::log10(e2 / r2));
    }
    for (auto &v : vs) {
        CK(hipMemset(out[0], 0xFF, NS * 8));
        issue(v, 0); sync_all(); CK(hipGetLastError());
        CK(hipMemcpy(got.data(), out[0], NS * 8, hipMemcpyDeviceToHost));
        size_t bad = 0;
        for (size_t i = 0; i < NS; i++) bad += memcmp(&got[i], &ref[i], 8) != 0;
        printf("%-24s output %s (%zu samples differ)\n", v.name, bad ? "DIFFERS" : "bit-identical", bad);
    }

    // settle: ~80 ms of launches (load-onset power transient)
    for (int i = 0; i < 1500; i++) issue(vs[0], i);
    sync_all();

    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<std::vector<double>> wall(vs.size()), evt(vs.size());
    for (int r = 0; r < rounds; r++) {
        for (size_t k = 0; k < vs.size(); k++) {
            for (int i = 0; i < 30; i++) issue(vs[k], i);
            sync_all();
            auto t0 = std::chrono::steady_clock::now();
            CK(hipEventRecord(e0, s0));
            for (int i = 0; i < steps; i++) issue(vs[k], i);
            CK(hipEventRecord(e1, s0));
            sync_all();
            auto t1 = std::chrono::steady_clock::now();
            float ms = 0; CK(hipEventElapsedTime(&ms, e0, e1));
            wall[k].push_back(std::chrono::duration<double>(t1 - t0).count() / steps * 1e6);
            evt[k].push_back(ms * 1e3 / steps);
        }
    }
    // "vs row 0": this row's median against the first row's, in per cent of the latter (negative = faster)
    printf("%-40s %10s %10s %10s %10s %10s %8s %9s\n", "variant", "wall med", "wall min", "wall max", "event med", "GS/s", "% 8TB/s", "vs row 0");
    auto med = [](std::vector<double> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
    const double wm0 = med(wall[0]);
    for (size_t k = 0; k < vs.size(); k++) {
        double wm = med(wall[k]), wmin = *std::min_element(wall[k].begin(), wall[k].end()), em = med(evt[k]);
        double wmax = *std::max_element(wall[k].begin(), wall[k].end());
        printf("%-40s %9.2fus %9.2fus %9.2fus %9.2fus %10.1f %8.2f %+8.2f%%\n", vs[k].name, wm, wmin, wmax, em, NS / wm / 1e3,
               16.0 * NS / wm / 8e6 * 100, (wm / wm0 - 1) * 100);
    }
    return 0;
}
