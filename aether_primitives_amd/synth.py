"""Polyphase synthesis filter bank: weighted overlap-add behind the inverse FFT (include/aether_hip.h, aeth_synth_*).

The transpose of `Channelizer`: every frame's `channels` time samples are extended periodically to the prototype's
length, weighted and overlap-added at the hop.  P = 1 with hop < channels is the inverse STFT, P > 1 the polyphase
synthesis bank.  The output is the reconstruction delayed by ntaps - hop samples."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .chan import _Bank
from .context import DeviceVec
from .fft import SIGN_REF_BWD, Scale


def dual_window(w, hop):
    """the synthesis window that inverts a windowed, overlapped transform of len(w) points at `hop`:
    g[j] = w[j] / sum of w[j']^2 over j' = j (mod hop), computed in f64, rounded once (float32).  Needs no context."""
    w = np.ascontiguousarray(w, dtype=np.float32).reshape(-1)
    out = np.empty(max(w.size, 1), np.float32)
    check(_lib.load().aeth_synth_dual_window(w.ctypes.data_as(C.c_void_p), w.size, int(hop), out.ctypes.data_as(C.c_void_p)))
    return out[:w.size]


class Synthesizer(_Bank):
    """Synthesizer(ctx, proto, channels, hop=None, phase="frame"): `proto` holds P * channels real taps, hop defaults to
    `channels`; phase as for `Channelizer` (pass the global number of a call's first frame as `first_frame`).  A call
    reads `history` frames in front of its own: the previous call's last ones, or zeros."""
    _prefix = "aeth_synth_"

    @property
    def history(self):
        """frames in front of a call's first that reach into its output: ceil(ntaps / hop) - 1"""
        return self._lib.aeth_synth_history(self.h)

    def samples(self, n_in):
        """output samples of a call over n_in input samples (n_in must be a multiple of `channels`)"""
        return int(n_in) // self.channels * self.hop

    def _args(self, v, hist):
        v, hist = self._vecs(v, hist)
        if hist is not None and hist.n != self.history * self.channels:
            raise _lib.LengthMismatch(_lib.E_LEN, f"history holds {hist.n} samples, {self.history} frames x {self.channels} "
                                      f"channels = {self.history * self.channels}")
        return v, hist, (hist._p() if hist is not None and hist.n else None)

    def unfold(self, v, hist=None, first_frame=0, out=None):
        """the back end alone: frames of time samples -> DeviceVec of samples(v.n) stream samples"""
        v, hist, hp = self._args(v, hist)
        out = DeviceVec(self.ctx, self.samples(v.n)) if out is None else out
        check(self._lib.aeth_synth_unfold(self.h, hp, v._p(), v.n, int(first_frame), out._p(), out.n))
        return out

    def exec(self, spec, hist=None, first_frame=0, sign=SIGN_REF_BWD, s=Scale.NONE, out=None):
        """the transform of every frame of `spec` (and of `hist`: both hold spectra), then the unfold"""
        spec, hist, hp = self._args(spec, hist)
        out = DeviceVec(self.ctx, self.samples(spec.n)) if out is None else out
        check(self._lib.aeth_synth_exec(self.h, hp, spec._p(), spec.n, int(first_frame), sign, s.kind, s.x, out._p(), out.n))
        return out
