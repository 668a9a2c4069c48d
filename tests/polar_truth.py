"""The numpy restatement of aeth_polar_* (include/aether_hip.h): polarization weights, rank, mask, transform, encoder and
the successive-cancellation decoder with flips, records and both outputs.  Vectorised over codewords: a node visit is one
numpy operation on [F][m] arrays, 2 N - 1 visits per call, nothing pruned."""
import numpy as np

CODEWORD = 1
NONE = 0xFFFFFFFF
Q = (4294967296, 5107605667, 6074001000, 7223245206)             # round(2^(r/4) 2^32)
RECORD = np.dtype([("index", np.uint32, 4), ("abs", np.uint32, 4)])


def weights(n):
    """W(i) = sum_j bit_j(i) (Q[j mod 4] << (j div 4)) as Python integers"""
    return [sum(((i >> j) & 1) * (Q[j % 4] << (j // 4)) for j in range(n)) for i in range(1 << n)]


def rank(n):
    """positions, most reliable first: larger weight first, ties to the larger position"""
    w = weights(n)
    return np.array(sorted(range(1 << n), key=lambda i: (w[i], i), reverse=True), np.uint32)


def mask(n, K):
    m = np.zeros(1 << n, np.uint8)
    m[rank(n)[:K]] = 1
    return m


def random_mask(n, K, seed):
    m = np.zeros(1 << n, np.uint8)
    m[np.random.default_rng(seed).choice(1 << n, K, replace=False)] = 1
    return m


def transform(u):
    """[F][N] bits -> [F][N]: for s = 0 .. n - 1, x[i] ^= x[i + 2^s] where bit s of i is clear"""
    x = np.array(u, np.uint8) & 1
    F, N = x.shape
    s = 1
    while s < N:
        v = x.reshape(F, N // (2 * s), 2, s)
        v[:, :, 0, :] ^= v[:, :, 1, :]
        s *= 2
    return x


def encode(msk, bits):
    """F K bytes -> F N coded bits"""
    msk = np.asarray(msk, np.uint8)
    N, K = msk.size, int(msk.sum())
    F = bits.size // K
    u = np.zeros((F, N), np.uint8)
    u[:, np.flatnonzero(msk)] = np.asarray(bits, np.uint8).reshape(F, K) & 1
    return transform(u).ravel()


def f_of(a, b):
    return np.sign(a) * np.sign(b) * np.minimum(np.abs(a), np.abs(b))


def decode(msk, soft, flip=None, flags=0):
    """-> (bits: F K decisions, or F N re-encoded bits with CODEWORD, flat uint8; records [F] of RECORD)"""
    msk = np.asarray(msk, np.uint8)
    N = msk.size
    F = soft.size // N
    flip = np.full(F, NONE, np.uint64) if flip is None else np.asarray(flip).astype(np.uint64)
    u = np.zeros((F, N), np.uint8)
    mag = np.zeros((F, N), np.int64)

    def dec(L, base):
        m = L.shape[1]
        if m == 1:
            if msk[base]:
                u[:, base] = (L[:, 0] < 0) ^ (flip == base)
                mag[:, base] = np.abs(L[:, 0])
            return u[:, base:base + 1].copy()
        h = m // 2
        a, b = L[:, :h], L[:, h:]
        x1 = dec(f_of(a, b), base)
        x2 = dec(np.where(x1 == 0, b + a, b - a), base + h)
        return np.concatenate([x1 ^ x2, x2], axis=1)

    x = dec(np.asarray(soft, np.int8).reshape(F, N).astype(np.int32), 0)
    info = np.flatnonzero(msk)
    rec = np.zeros(F, RECORD)
    rec["index"], rec["abs"] = NONE, NONE
    keys = np.sort(mag[:, info] * 1024 + info[None, :], axis=1)[:, :4]          # (|L|, i) in lexicographic order
    rec["index"][:, :keys.shape[1]] = keys % 1024
    rec["abs"][:, :keys.shape[1]] = keys // 1024
    bits = x if flags & CODEWORD else u[:, info]
    return np.ascontiguousarray(bits).ravel(), rec


def soft_of_bits(coded, level=127):
    """the noise-free soft values of coded bits: +level for 0, -level for 1"""
    return (level - 2 * level * (np.asarray(coded, np.int16) & 1)).astype(np.int8)


def noisy_soft(rng, coded, sigma, scale=32.0):
    """BPSK +-1 through AWGN of deviation sigma, scaled and clamped to int8"""
    y = 1.0 - 2.0 * (np.asarray(coded, np.float64) % 2) + sigma * rng.standard_normal(np.size(coded))
    return np.clip(np.rint(scale * y), -128, 127).astype(np.int8)


def test_codes():
    """{name: (n, mask)}: the codes of tests/test_gpu_polar.py"""
    codes = {f"{n}x{K}": (n, mask(n, K)) for n, K in ((3, 4), (3, 8), (5, 16), (9, 171), (10, 512), (10, 1023))}
    last = np.zeros(64, np.uint8)
    last[63] = 1
    codes["6x1"] = (6, last)
    codes["7x64r"] = (7, random_mask(7, 64, 764))
    return codes


test_codes.__test__ = False
