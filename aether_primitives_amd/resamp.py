"""Polyphase rational resampler: up U, real FIR, down Q in one pass (include/aether_hip.h, aeth_resamp_*).

The reference's rate changes are linear interpolation and sample picking (src/sampling.rs:7-62).  `Resampler` converts a
stream by the ratio up / down behind a proper anti-alias / anti-image filter: out[k] = sum over p of
taps[p * up + (k * down) mod up] * s[floor(k * down / up) - p].  A call over n = B * down samples makes B * up outputs."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .context import DeviceVec


def prototype(up, down, taps_per_phase):
    """up * taps_per_phase real taps (float32), computed in f64 on the host: the Hamming-windowed low-pass of cutoff
    1 / (2 max(up, down)) cycles per upsampled sample, scaled to sum to `up`.  Needs no context."""
    up, down, taps_per_phase = int(up), int(down), int(taps_per_phase)
    out = np.empty(max(up * taps_per_phase, 1), np.float32)
    check(_lib.load().aeth_resamp_prototype(up, down, taps_per_phase, out.ctypes.data_as(C.c_void_p)))
    return out[:up * taps_per_phase]


def call_vecs(rs, x, hist):
    """x and hist of an exec call of `rs` (a Resampler or an ArbResampler) as DeviceVecs, which the caller keeps until the
    call is made, and the pointer of the `rs.history` samples of history: None for zeros (no history, or an empty one)"""
    if not isinstance(x, DeviceVec):
        x = rs.ctx.vec(x)
    if hist is not None and not isinstance(hist, DeviceVec):
        hist = rs.ctx.vec(hist)
    if hist is not None and hist.n != rs.history:
        raise _lib.LengthMismatch(_lib.E_LEN, f"history holds {hist.n} samples, taps per phase - 1 = {rs.history}")
    return x, hist, (hist._p() if hist is not None and hist.n else None)


class Resampler:
    """Resampler(ctx, taps, up, down): `taps` holds P * up real taps.  A call reads `history` samples in front of its
    own: the previous call's last ones, or zeros."""

    def __init__(self, ctx, taps, up, down):
        self.ctx = ctx
        self._lib = _lib.load()
        taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        h = C.c_void_p()
        check(self._lib.aeth_resamp_create(ctx.h, taps.ctypes.data_as(C.c_void_p), taps.size, int(up), int(down), C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self._lib.aeth_resamp_destroy(self.h)
                self.h = None
        except Exception:
            pass

    @property
    def up(self): return self._lib.aeth_resamp_up(self.h)
    @property
    def down(self): return self._lib.aeth_resamp_down(self.h)
    @property
    def ntaps(self): return self._lib.aeth_resamp_ntaps(self.h)
    @property
    def tile(self): return self._lib.aeth_resamp_tile(self.h)

    @property
    def history(self):
        """input samples in front of a call's first that reach into its output: taps per phase - 1"""
        return self._lib.aeth_resamp_history(self.h)

    @property
    def route(self):
        """the kernel route: "staged" or "direct", followed by " u1" when up == 1"""
        return self._lib.aeth_resamp_route(self.h).decode()

    def out_count(self, n):
        """output samples of a call over n input samples (0 when n is not a multiple of `down`)"""
        return self._lib.aeth_resamp_out_count(self.h, int(n))

    def exec(self, x, hist=None, out=None):
        """x (and the `history` samples in front of it, or zeros) -> DeviceVec of out_count(x.n) samples"""
        x, hist, hp = call_vecs(self, x, hist)
        if out is None:
            n_out = self.out_count(x.n)
            if not n_out:
                raise _lib.LengthMismatch(_lib.E_LEN, f"{x.n} input samples are not a multiple (at least one) of down {self.down}")
            out = DeviceVec(self.ctx, n_out)
        check(self._lib.aeth_resamp_exec(self.h, hp, x._p(), x.n, out._p(), out.n))
        return out
