"""Arbitrary-ratio resampler: interpolated polyphase taps behind a Q32.32 time word (include/aether_hip.h, aeth_arb_*).

The reference's rate changes are linear interpolation and sample picking (src/sampling.rs:7-62).  `ArbResampler` converts a
stream by a ratio that is no small fraction: output m of a call stands at t = phase + m * step input samples, `step` and
`phase` being unsigned Q32.32 words (`step_word(ratio)`); its taps are those of phase floor(frac(t) * L), moved towards
the next phase by the rest of the fraction.  The chunks of a stream continue each other bit for bit when the caller passes
the previous `history` samples and the phase that `advance` returns."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .context import DeviceVec
from .resamp import call_vecs


def step_word(ratio):
    """the Q32.32 word of `ratio` input samples per output sample: ratio * 2^32 in f64, truncated"""
    return int(float(ratio) * 4294967296.0)


def advance(step, phase, n):
    """(count, next_phase) of a call over n input samples: the outputs m with phase + m * step < n * 2^32, and the phase
    of the next call.  Needs no context."""
    count, nxt = C.c_size_t(0), C.c_uint64(0)
    check(_lib.load().aeth_arb_advance(int(step), int(phase), int(n), C.byref(count), C.byref(nxt)))
    return count.value, nxt.value


class ArbResampler:
    """ArbResampler(ctx, taps, log2_phases): `taps` holds P * 2^log2_phases real taps (resamp.prototype designs them).  A
    call reads `history` samples in front of its own: the previous call's last ones, or zeros.  `phase` is the time word
    of the next call's first output; exec() uses and updates it unless a phase is passed."""

    def __init__(self, ctx, taps, log2_phases):
        self.ctx = ctx
        self._lib = _lib.load()
        taps = np.ascontiguousarray(taps, dtype=np.float32).reshape(-1)
        h = C.c_void_p()
        check(self._lib.aeth_arb_create(ctx.h, taps.ctypes.data_as(C.c_void_p), taps.size, int(log2_phases), C.byref(h)))
        self.h = h
        self.phase = 0

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self._lib.aeth_arb_destroy(self.h)
                self.h = None
        except Exception:
            pass

    @property
    def phases(self): return self._lib.aeth_arb_phases(self.h)
    @property
    def ntaps(self): return self._lib.aeth_arb_ntaps(self.h)

    @property
    def history(self):
        """input samples in front of a call's first that reach into its output: taps per phase - 1"""
        return self._lib.aeth_arb_history(self.h)

    def tile(self, step):
        """consecutive outputs one workgroup makes at this step (0: the step is out of range)"""
        return self._lib.aeth_arb_tile(self.h, int(step))

    def route(self, step):
        """the kernel route at this step: "staged" (" tab": the tap table lies in LDS too) or "direct" ("": the step is out of range)"""
        return self._lib.aeth_arb_route(self.h, int(step)).decode()

    advance = staticmethod(advance)

    def exec(self, x, step, phase=None, hist=None, out=None):
        """x (and the `history` samples in front of it, or zeros) -> DeviceVec of advance(step, phase, x.n)[0] samples.
        phase None: the call starts at self.phase and leaves the next call's phase there."""
        x, hist, hp = call_vecs(self, x, hist)
        start = self.phase if phase is None else int(phase)
        count, nxt = advance(step, start, x.n)
        if out is None:
            out = DeviceVec(self.ctx, count)
        check(self._lib.aeth_arb_exec(self.h, hp, x._p(), x.n, int(step), start, out._p(), out.n))
        if phase is None:
            self.phase = nxt
        return out
