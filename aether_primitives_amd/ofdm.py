"""OFDM symbols on the device (include/aether_hip.h, aeth_ofdm_*): the framing and the one-tap equaliser of an OFDM link.

The reference has `Fft`, `vec_mul` and `chunks_mut(fft_len)` framing only.  An `Ofdm` is a transform length, a cyclic
prefix and a carrier list (`bins[k]`: the FFT bin of carrier k, in the caller's order).  `demod` strips the prefix,
transforms (sign of `Fft::fwd`), picks the carriers and multiplies by a per-carrier coefficient in one kernel; `mod`
places carriers on a zero grid, transforms back (sign of `Fft::bwd`) and writes the symbol behind its prefix;
`estimate` sums training symbols per carrier in f64 and hands out the channel, the equaliser's coefficients and |H|^2.
Everything stays on the device and is ordered on the context's stream."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .context import DeviceF32, DeviceVec
from .fft import Scale

GENERAL = 1
EQ_KINDS = {"zf": 0, "mmse": 1, "matched": 2}


def _vec(ctx, x):
    return x if isinstance(x, DeviceVec) else ctx.vec(x)


class Ofdm:
    """Ofdm(ctx, n_fft, cp, bins, max_symbols=0, general=False).  `max_symbols` bounds the symbols of one call (0: no
    bound; the general route's scratch then grows on demand); `general=True` never takes the fused kernel."""

    def __init__(self, ctx, n_fft, cp, bins, max_symbols=0, general=False):
        self.ctx = ctx
        self._lib = _lib.load()
        b = np.ascontiguousarray(np.asarray(bins, dtype=np.int64).reshape(-1))
        if b.size and (b.min() < 0 or b.max() > 0xFFFFFFFF):
            raise _lib.AetherError(_lib.E_ARG, f"bin {int(b.min() if b.min() < 0 else b.max())} is not a 32-bit unsigned number")
        b = b.astype(np.uint32)
        self.h = C.c_void_p()
        check(self._lib.aeth_ofdm_create(ctx.h, int(n_fft), int(cp), b.ctypes.data_as(C.c_void_p), b.size, int(max_symbols),
                                         GENERAL if general else 0, C.byref(self.h)))
        self.bins = b

    # ---- read-outs ----
    @property
    def len(self):
        return int(self._lib.aeth_ofdm_len(self.h))

    @property
    def cp(self):
        return int(self._lib.aeth_ofdm_cp(self.h))

    @property
    def symbol(self):
        """n_fft + cp"""
        return int(self._lib.aeth_ofdm_symbol(self.h))

    @property
    def carriers(self):
        return int(self._lib.aeth_ofdm_carriers(self.h))

    @property
    def route(self):
        """"fused", or "general: " and the inner plan's route"""
        return self._lib.aeth_ofdm_route(self.h).decode()

    def span(self, n_sym):
        """samples `demod` reads for n_sym symbols: (n_sym - 1) * symbol + len"""
        return int(self._lib.aeth_ofdm_span(self.h, int(n_sym)))

    # ---- calls ----
    def demod(self, x, n_sym, eq=None, scale=Scale.NONE, out=None):
        """x[s * symbol + e], e < len, is the window of symbol s (point x at the first window sample) -> DeviceVec of
        n_sym * carriers: the carriers of every symbol, times eq[k] when given"""
        x = _vec(self.ctx, x)
        if eq is not None:
            eq = _vec(self.ctx, eq)
            if eq.n != self.carriers:
                raise _lib.LengthMismatch(_lib.E_LEN, f"eq holds {eq.n} coefficients, {self.carriers} carriers")
        if out is None:
            out = DeviceVec(self.ctx, int(n_sym) * self.carriers)
        check(self._lib.aeth_ofdm_demod(self.h, x._p(), x.n, int(n_sym), eq._p() if eq is not None else None, scale.kind, scale.x,
                                        out._p(), out.n))
        return out

    def mod(self, carriers, n_sym, scale=Scale.NONE, out=None):
        """carriers[s * K + k] -> DeviceVec of n_sym * symbol time samples, every symbol behind its cyclic prefix"""
        carriers = _vec(self.ctx, carriers)
        if out is None:
            out = DeviceVec(self.ctx, int(n_sym) * self.symbol)
        check(self._lib.aeth_ofdm_mod(self.h, carriers._p(), carriers.n, int(n_sym), scale.kind, scale.x, out._p(), out.n))
        return out

    def estimate_into(self, y, x_known, n_sym, nv=0.0, kind="zf", h=None, eq=None, csi=None):
        """the estimate of n_sym training symbols y against x_known (one symbol, or n_sym of them) into the buffers given
        (DeviceVec h, DeviceVec eq, DeviceF32 csi; any may be None, not all)"""
        y, x_known = _vec(self.ctx, y), _vec(self.ctx, x_known)
        K = self.carriers
        if y.n != int(n_sym) * K or x_known.n % max(K, 1):
            raise _lib.LengthMismatch(_lib.E_LEN, f"{y.n} received and {x_known.n} known carriers for {n_sym} symbols of {K}")
        p = lambda v: v._p() if v is not None else None             # noqa: E731
        check(self._lib.aeth_ofdm_estimate(self.h, y._p(), x_known._p(), int(n_sym), x_known.n // K, float(nv), EQ_KINDS[kind],
                                           p(h), p(eq), p(csi)))
        return h, eq, csi

    def estimate(self, y, x_known, nv=0.0, kind="zf"):
        """-> (h, eq, csi): per carrier the channel H = sum Y conj(X) / sum |X|^2 over the training symbols in y
        (len(y) / carriers of them), the coefficient `demod` multiplies by ("zf": 1 / H, "mmse": conj(H) / (|H|^2 + nv),
        "matched": conj(H)) and |H|^2.  DeviceVec, DeviceVec, DeviceF32 of `carriers` entries."""
        y = _vec(self.ctx, y)
        K = self.carriers
        if y.n % max(K, 1):
            raise _lib.LengthMismatch(_lib.E_LEN, f"{y.n} received carriers are not whole symbols of {K}")
        return self.estimate_into(y, x_known, y.n // K, nv, kind, DeviceVec(self.ctx, K), DeviceVec(self.ctx, K), DeviceF32(self.ctx, K))

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            self._lib.aeth_ofdm_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            if self.ctx.h:
                self.close()
        except Exception:
            pass
