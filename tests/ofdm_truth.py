"""numpy restatement of the OFDM calls (include/aether_hip.h, aeth_ofdm_*): `demod_truth` and `mod_truth` in complex128,
`estimate_truth` following the f64 definition step by step (its results are the expected BITS).

Signs.  The library binds `Fft::fwd` to the exponent +j and `Fft::bwd` to -j (csrc/aeth_fft_core.h: the reference plans
`fwd` with rustfft's inverse = true), demod transforms with `fwd` and mod with `bwd`.  So a carrier on bin b is the tone
exp(-2 pi i b n / N) in time, and a channel with taps h multiplies it by sum_t h[t] exp(+2 pi i b t / N): the transform of
the taps with demod's own sign, `channel_response` below.  A window taken `a` samples early multiplies by
exp(+2 pi i b a / N).  (The textbook form, mod = exp(+j) and demod = exp(-j), has both exponents negated.)"""
import numpy as np

ZF, MMSE, MATCHED = 0, 1, 2


def fwd(x):
    """Fft::fwd without a scale: X[k] = sum_n x[n] exp(+2 pi i k n / N), over the last axis"""
    x = np.asarray(x, np.complex128)
    return np.fft.ifft(x, axis=-1) * x.shape[-1]


def bwd(x):
    """Fft::bwd without a scale: exp(-2 pi i k n / N)"""
    return np.fft.fft(np.asarray(x, np.complex128), axis=-1)


def windows(x, n_fft, cp, n_sym):
    """the n_sym windows of demod: x[s L + e], e < N"""
    L = n_fft + cp
    x = np.asarray(x)
    return np.stack([x[s * L: s * L + n_fft] for s in range(n_sym)]) if n_sym else np.zeros((0, n_fft), x.dtype)


def demod_truth(x, n_fft, cp, bins, n_sym, eq=None, scale=1.0):
    """-> (n_sym, K) complex128"""
    y = fwd(windows(np.asarray(x, np.complex128), n_fft, cp, n_sym)) * scale
    y = y[:, np.asarray(bins, np.int64)]
    return y if eq is None else y * np.asarray(eq, np.complex128)[None, :]


def grid(car, n_fft, bins, n_sym):
    car = np.asarray(car).reshape(n_sym, len(bins))
    g = np.zeros((n_sym, n_fft), car.dtype)
    g[:, np.asarray(bins, np.int64)] = car
    return g


def add_prefix(t, cp):
    """(n_sym, N) time samples -> n_sym * (N + cp) samples, every symbol behind its last cp samples"""
    n = t.shape[1]
    return np.concatenate([t[:, n - cp:], t], axis=1).reshape(-1)


def mod_truth(car, n_fft, cp, bins, n_sym, scale=1.0):
    """-> n_sym * (n_fft + cp) complex128"""
    return add_prefix(bwd(grid(np.asarray(car, np.complex128), n_fft, bins, n_sym)) * scale, cp)


def channel_response(taps, n_fft):
    """what a channel with these taps multiplies bin b by: sum_t h[t] exp(+2 pi i b t / N)"""
    h = np.zeros(n_fft, np.complex128)
    h[:len(taps)] = taps
    return fwd(h)


def advance_ramp(n_fft, a):
    """what a window taken `a` samples early multiplies bin b by"""
    return np.exp(2j * np.pi * np.arange(n_fft) * a / n_fft)


def estimate_truth(y, x, n_sym, x_sym, K, nv=0.0, kind=ZF):
    """y: n_sym * K complex64, x: x_sym * K complex64 (x_sym 1 or n_sym) -> (h complex64[K], eq complex64[K], csi float32[K]),
    every step of the definition in the header on its own line"""
    y = np.asarray(y, np.complex64).reshape(n_sym, K)
    x = np.asarray(x, np.complex64).reshape(x_sym, K)
    assert x_sym in (1, n_sym)
    nr, ni, den = np.zeros(K, np.float64), np.zeros(K, np.float64), np.zeros(K, np.float64)
    with np.errstate(all="ignore"):
        for s in range(n_sym):
            xs = 0 if x_sym == 1 else s
            yr, yi = y[s].real.astype(np.float64), y[s].imag.astype(np.float64)
            xr, xi = x[xs].real.astype(np.float64), x[xs].imag.astype(np.float64)
            nr = nr + (yr * xr + yi * xi)           # the products are exact in f64: one rounding per sum
            ni = ni + (yi * xr - yr * xi)
            den = den + (xr * xr + xi * xi)
        live = den != 0.0
        safe = np.where(live, den, 1.0)
        hr = np.where(live, (nr / safe).astype(np.float32), np.float32(0)).astype(np.float32)
        hi = np.where(live, (ni / safe).astype(np.float32), np.float32(0)).astype(np.float32)
        hrd, hid = hr.astype(np.float64), hi.astype(np.float64)
        p = hrd * hrd + hid * hid
        csi = p.astype(np.float32)
        if kind == MATCHED:
            wr, wi = hr, (-hi).astype(np.float32)
        else:
            d = p + (np.float64(np.float32(nv)) if kind == MMSE else 0.0)
            ok = d != 0.0
            ds = np.where(ok, d, 1.0)
            wr = np.where(ok, (hrd / ds).astype(np.float32), np.float32(0)).astype(np.float32)
            wi = np.where(ok, ((-hid) / ds).astype(np.float32), np.float32(0)).astype(np.float32)
    h = np.empty(K, np.complex64); h.real, h.imag = hr, hi
    w = np.empty(K, np.complex64); w.real, w.imag = wr, wi
    return h, w, csi
