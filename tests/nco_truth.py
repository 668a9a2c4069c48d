"""numpy restatement of the oscillator's definition (include/aether_hip.h, aeth_nco_*): uint64 arrays with wrap-around
for the words, float32 array operations for the phasor (numpy rounds every product and every sum, as the definition does;
re and im are handled separately so that Inf, NaN and -0.0 behave as real multiplications), and a complex128 truth built
from Python integers."""
import numpy as np

f32 = np.float32
K = f32(2 * np.pi / 2 ** 32)                                       # 1.4629180792671596e-09 rounded to f32
S1, S2, S3 = f32(-1.6666654611e-1), f32(8.3321608736e-3), f32(-1.9515295891e-4)
C1, C2, C3 = f32(4.166664568298827e-2), f32(-1.388731625493765e-3), f32(2.443315711809948e-5)
MASK = (1 << 64) - 1


def words_at(words, n):
    """w(n) for a uint64 array n (or a Python integer) -> uint64 array"""
    phase, step, rate = (np.uint64(int(v) & MASK) for v in words)
    n = np.atleast_1d(np.asarray(n, dtype=np.uint64))
    one = np.uint64(1)
    with np.errstate(over="ignore"):
        tri = np.where((n & one) == 0, (n >> one) * (n - one), n * ((n - one) >> one))
        return phase + n * step + tri * rate


def positions(n0, n):
    """the stream positions n0 .. n0 + n - 1 as uint64 (n0 + n <= 2^64)"""
    assert 0 <= n0 and n0 + n <= 1 << 64
    return np.uint64(n0) + np.arange(n, dtype=np.uint64)


def phasor(w):
    """uint64 array of words -> (c, d) float32 arrays"""
    w = np.atleast_1d(np.asarray(w, dtype=np.uint64))
    t = (w >> np.uint64(32)).astype(np.uint32)
    k = ((t + np.uint32(0x20000000)) >> np.uint32(30)) & np.uint32(3)
    r = (t - (k << np.uint32(30))).view(np.int32)
    a = r.astype(f32) * K
    s = a * a
    ps = (S3 * s + S2) * s + S1
    sn = (a * s) * ps + a
    pc = (C3 * s + C2) * s + C1
    cs = (f32(1) - f32(0.5) * s) + (s * s) * pc
    for v in (a, s, ps, sn, pc, cs):
        assert v.dtype == f32
    c = np.where(k == 0, cs, np.where(k == 1, -sn, np.where(k == 2, -cs, sn)))
    d = np.where(k == 0, sn, np.where(k == 1, cs, np.where(k == 2, -sn, -cs)))
    return c, d


def mix(words, n0, x):
    x = np.asarray(x, np.complex64)
    c, d = phasor(words_at(words, positions(n0, x.size)))
    xr, xi = x.real.astype(f32), x.imag.astype(f32)
    out = np.empty(x.size, np.complex64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):          # Inf, NaN and denormals are data here
        out.real = xr * c - xi * d
        out.imag = xr * d + xi * c
    return out


def tone(words, n0, amp, n):
    c, d = phasor(words_at(words, positions(n0, n)))
    out = np.empty(n, np.complex64)
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        out.real = f32(amp) * c
        out.imag = f32(amp) * d
    return out


def word_int(words, n):
    """w(n) in Python integers"""
    phase, step, rate = (int(v) for v in words)
    n = int(n)
    return (phase + n * step + (n * (n - 1) // 2) * rate) & MASK


def phasor_f64(w):
    """exp(2 pi j w / 2^64) in complex128 from Python integers: the turn is reduced exactly before the division"""
    out = np.empty(len(w), np.complex128)
    for i, v in enumerate(w):
        v = int(v) & MASK
        q, r = divmod(v + (1 << 61), 1 << 62)                       # nearest quarter turn, r - 2^61 in [-2^61, 2^61)
        ang = 2 * np.pi * ((r - (1 << 61)) / 2.0 ** 64)
        out[i] = np.exp(1j * ang) * (1, 1j, -1, -1j)[q & 3]
    return out


def same_bits(got, want):
    """bit for bit, except that a NaN matches any NaN (the payload is not defined)"""
    g = np.ascontiguousarray(got, np.complex64).view(np.float32)
    w = np.ascontiguousarray(want, np.complex64).view(np.float32)
    if g.shape != w.shape:
        return False
    nan = np.isnan(w)
    return bool((np.isnan(g) == nan).all() and (g.view(np.uint32)[~nan] == w.view(np.uint32)[~nan]).all())
