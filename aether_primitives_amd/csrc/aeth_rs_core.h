// aeth_rs_core.h -- the algebra of a Reed-Solomon code over GF(2^m), 3 <= m <= 8, in plain C++ (not installed): the
// field, the generator, the systematic encoder and the bounded-distance errors-and-erasures decoder of
// include/aether_hip.h (aeth_rs_*).  aeth_rs_host_encode / aeth_rs_host_decode run it on host memory, so the maths is
// testable without a device; aeth_rs.hip runs the two decoder stages below (solve, locate) in its kernel on LDS arrays.
//
// Positions.  Symbol j of a codeword is the coefficient of x^p, p = n - 1 - j.  beta = alpha^prim; the locator of
// position p is X = beta^p.  Syndromes S_i = r(beta^(fcr + i)) = sum_k (e_k X_k^fcr) X_k^i, i < r.
// Decoder.  Gamma = prod (1 - X x) over the erased positions; Berlekamp-Massey started from Gamma gives Lambda of formal
// length L; Omega = S Lambda mod x^r has degree below L.  A root X^-1 of Lambda carries the error value
//     e = Omega(X^-1) X^(1 - fcr) / Lambda'(X^-1).
// The word is inside the bound exactly when deg Lambda = L, 2 L - f <= r, Lambda has L roots among the n positions of
// the (shortened) code and no denominator vanishes; everything else is a failure.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define AETH_RS_HD __host__ __device__ __forceinline__
#else
#define AETH_RS_HD inline
#endif

namespace aeth {
namespace rs {

constexpr uint32_t kMaxRoots = 64;
constexpr uint32_t kMaxDepth = 64;

struct Code { uint32_t m, poly, fcr, prim, nroots, n; };          // aeth_rs_code

// antilog twice over (no reduction of a sum of two logs) and log; log[0] is never read
struct Field {
    uint32_t m, N0;
    uint8_t exp[512];
    uint8_t log[256];
};

// the tables as a decoder stage sees them: host memory or LDS
struct Tab {
    const uint8_t *exp, *log;
    uint32_t N0, fcr, prim, r, n;
};

AETH_RS_HD uint32_t mul(const Tab &t, uint32_t a, uint32_t b) { return a && b ? t.exp[(uint32_t)t.log[a] + t.log[b]] : 0u; }
AETH_RS_HD uint32_t inv(const Tab &t, uint32_t a) { return t.exp[t.N0 - t.log[a]]; }
// beta^e for any e >= 0
AETH_RS_HD uint32_t beta_pow(const Tab &t, uint64_t e) { return t.exp[(uint32_t)(((e % t.N0) * t.prim) % t.N0)]; }

// 0 when poly (with its x^m term) is primitive of degree m: fills the tables
inline bool build_field(uint32_t m, uint32_t poly, Field &f)
{
    f.m = m;
    f.N0 = (1u << m) - 1;
    std::memset(f.exp, 0, sizeof f.exp);
    std::memset(f.log, 0, sizeof f.log);
    uint32_t v = 1;
    for (uint32_t i = 0; i < f.N0; i++) {
        if (i && v == 1) return false;                                   // the order of x divides i < N0
        f.exp[i] = f.exp[i + f.N0] = (uint8_t)v;
        f.log[v] = (uint8_t)i;
        v <<= 1;
        if (v >> m) v ^= poly;
    }
    return v == 1;
}

inline uint32_t gcd(uint32_t a, uint32_t b) { while (b) { const uint32_t t = a % b; a = b; b = t; } return a; }

inline Tab tab_of(const Field &f, const Code &c) { return Tab{f.exp, f.log, f.N0, c.fcr, c.prim, c.nroots, c.n}; }

// g[i] is the coefficient of x^i, g[r] = 1
inline void generator(const Tab &t, uint8_t *g)
{
    std::memset(g, 0, t.r + 1);
    g[0] = 1;
    for (uint32_t j = 0; j < t.r; j++) {
        const uint32_t root = beta_pow(t, (uint64_t)t.fcr + j);
        for (uint32_t i = j + 1; i > 0; i--) g[i] = (uint8_t)(g[i - 1] ^ mul(t, g[i], root));
        g[0] = (uint8_t)mul(t, g[0], root);
    }
}

// one codeword: k data symbols at data[j * stride] (taken & N0) -> parity[q * stride], q < r: the remainder of
// d(x) x^r modulo g, highest coefficient first
inline void encode_word(const Tab &t, const uint8_t *g, const uint8_t *data, size_t stride, uint8_t *parity)
{
    uint8_t rem[kMaxRoots] = {0};
    const uint32_t k = t.n - t.r;
    for (uint32_t j = 0; j < k; j++) {
        const uint32_t fb = (data[j * stride] & t.N0) ^ rem[0];
        for (uint32_t q = 0; q + 1 < t.r; q++) rem[q] = (uint8_t)(rem[q + 1] ^ mul(t, fb, g[t.r - 1 - q]));
        rem[t.r - 1] = (uint8_t)mul(t, fb, g[0]);
    }
    for (uint32_t q = 0; q < t.r; q++) parity[q * stride] = rem[q];
}

// S[i] = r(beta^(fcr + i)) by Horner over the n symbols
inline void syndromes(const Tab &t, const uint8_t *word, size_t stride, uint8_t *S)
{
    for (uint32_t i = 0; i < t.r; i++) {
        const uint32_t root = beta_pow(t, (uint64_t)t.fcr + i);
        uint32_t s = 0;
        for (uint32_t j = 0; j < t.n; j++) s = mul(t, s, root) ^ (word[j * stride] & t.N0);
        S[i] = (uint8_t)s;
    }
}

// The work arrays of one codeword, r + 1 bytes each but `S`, `omega`, `era`, `rpos`, `rmag` (r): host stack or LDS.
struct Work {
    uint8_t *S, *lam, *b, *tmp, *omega;
    uint8_t *era;                       // the powers p of the erased positions, f of them, any order
    uint8_t *rpos, *rmag;               // the roots found by locate: symbol index j and error value
};

// Stage 1, serial: Gamma, Berlekamp-Massey, Omega.  f <= r.  Returns L, or ~0u when the word is outside the bound for
// sure (deg Lambda != L or 2 L - f > r).
AETH_RS_HD uint32_t solve(const Tab &t, const Work &w, uint32_t f)
{
    const uint32_t r = t.r;
    for (uint32_t i = 0; i <= r; i++) w.lam[i] = 0;
    w.lam[0] = 1;
    for (uint32_t e = 0; e < f; e++) {
        const uint32_t X = beta_pow(t, w.era[e]);
        for (uint32_t i = e + 1; i > 0; i--) w.lam[i] = (uint8_t)(w.lam[i] ^ mul(t, w.lam[i - 1], X));
    }
    for (uint32_t i = 0; i <= r; i++) w.b[i] = w.lam[i];
    uint32_t L = f;
    for (uint32_t k = f; k < r; k++) {
        uint32_t d = 0;
        for (uint32_t i = 0; i <= k; i++) d ^= mul(t, w.lam[i], w.S[k - i]);
        if (d == 0) {
            for (uint32_t i = r; i > 0; i--) w.b[i] = w.b[i - 1];
            w.b[0] = 0;
            continue;
        }
        w.tmp[0] = w.lam[0];
        for (uint32_t i = 1; i <= r; i++) w.tmp[i] = (uint8_t)(w.lam[i] ^ mul(t, d, w.b[i - 1]));
        if (2 * L <= k + f) {
            L = k + 1 + f - L;
            const uint32_t di = inv(t, d);
            for (uint32_t i = 0; i <= r; i++) w.b[i] = (uint8_t)mul(t, w.lam[i], di);
        } else {
            for (uint32_t i = r; i > 0; i--) w.b[i] = w.b[i - 1];
            w.b[0] = 0;
        }
        for (uint32_t i = 0; i <= r; i++) w.lam[i] = w.tmp[i];
    }
    uint32_t deg = 0;
    for (uint32_t i = 0; i <= r; i++)
        if (w.lam[i]) deg = i;
    if (deg != L || 2 * L > r + f) return ~0u;
    for (uint32_t i = 0; i < L; i++) {
        uint32_t o = 0;
        for (uint32_t j = 0; j <= i; j++) o ^= mul(t, w.S[i - j], w.lam[j]);
        w.omega[i] = (uint8_t)o;
    }
    return L;
}

// Stage 2, per position: is symbol j an error location of Lambda (length L)?  0: no; 1: yes, *mag is the error value
// (which may be 0 at an erased position); 2: yes, but the denominator vanishes.
AETH_RS_HD uint32_t locate(const Tab &t, const Work &w, uint32_t L, uint32_t j, uint32_t *mag)
{
    const uint32_t p = t.n - 1 - j;
    const uint32_t lx = (p * t.prim) % t.N0;                             // log of X
    const uint32_t xi = t.exp[t.N0 - lx];                                // X^-1 (exp[N0] = 1)
    uint32_t v = 0;
    for (uint32_t i = L + 1; i > 0; i--) v = mul(t, v, xi) ^ w.lam[i - 1];
    if (v) return 0;
    uint32_t num = 0;
    for (uint32_t i = L; i > 0; i--) num = mul(t, num, xi) ^ w.omega[i - 1];
    // Lambda'(x) = sum over odd i of lam[i] x^(i - 1): a polynomial in x^2
    const uint32_t xi2 = mul(t, xi, xi);
    uint32_t den = 0;
    for (uint32_t i = ((L - 1) | 1u); ; i -= 2) {                        // the highest odd index <= L (L >= 1 here)
        if (i <= L) den = mul(t, den, xi2) ^ w.lam[i];
        if (i == 1) break;
    }
    if (den == 0) return 2;
    // X^(1 - fcr): log = lx (1 - fcr) mod N0
    const uint32_t lf = (lx * ((t.N0 + 1 - t.fcr % t.N0) % t.N0)) % t.N0;
    *mag = mul(t, mul(t, num, t.exp[lf]), inv(t, den));
    return 1;
}

struct Record { uint32_t corrected, status; };                            // aeth_rs_record

// the definition on one codeword in host memory; out receives nb (n or k) symbols
inline Record decode_word(const Tab &t, const uint8_t *in, const uint8_t *era, size_t stride, uint8_t *out, size_t ostride, uint32_t nb)
{
    uint8_t S[kMaxRoots], lam[kMaxRoots + 1], b[kMaxRoots + 1], tmp[kMaxRoots + 1], omega[kMaxRoots], ep[kMaxRoots], rpos[kMaxRoots], rmag[kMaxRoots];
    const Work w{S, lam, b, tmp, omega, ep, rpos, rmag};
    for (uint32_t j = 0; j < nb; j++) out[j * ostride] = (uint8_t)(in[j * stride] & t.N0);
    uint32_t f = 0;
    if (era)
        for (uint32_t j = 0; j < t.n; j++)
            if (era[j * stride]) {
                if (f < t.r) ep[f] = (uint8_t)(t.n - 1 - j);
                f++;
            }
    if (f > t.r) return Record{0, 1};
    syndromes(t, in, stride, S);
    bool clean = f == 0;
    for (uint32_t i = 0; i < t.r; i++) clean = clean && S[i] == 0;
    if (clean) return Record{0, 0};
    const uint32_t L = solve(t, w, f);
    if (L == ~0u) return Record{0, 1};
    uint32_t found = 0;
    bool bad = false;
    for (uint32_t j = 0; j < t.n && L; j++) {
        uint32_t mag = 0;
        const uint32_t h = locate(t, w, L, j, &mag);
        if (h == 2) bad = true;
        if (h == 1 && found < t.r) { rpos[found] = (uint8_t)j; rmag[found] = (uint8_t)mag; }
        if (h) found++;
    }
    if (bad || found != L) return Record{0, 1};
    uint32_t corrected = 0;
    for (uint32_t e = 0; e < found; e++) {
        if (!rmag[e]) continue;
        corrected++;
        if (rpos[e] < nb) out[rpos[e] * ostride] ^= rmag[e];
    }
    return Record{corrected, 0};
}

struct Named { const char *name; Code c; };
inline const Named *named_table(size_t *n)
{
    static const Named t[] = {
        {"ccsds-255-223", {8, 0x187, 112, 11, 32, 255}},
        {"ccsds-255-239", {8, 0x187, 120, 11, 16, 255}},
        {"dvb-204-188", {8, 0x11d, 0, 1, 16, 204}},
        {"rs-15-11", {4, 0x13, 1, 1, 4, 15}},
    };
    *n = sizeof(t) / sizeof(t[0]);
    return t;
}
inline const Named *find_named(const char *name)
{
    size_t n;
    const Named *t = named_table(&n);
    for (size_t i = 0; i < n; i++)
        if (!std::strcmp(t[i].name, name)) return &t[i];
    return nullptr;
}

}  // namespace rs
}  // namespace aeth
