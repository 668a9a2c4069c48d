"""Polyphase analysis filter bank: windowed, overlapped FFT frames (include/aether_hip.h, aeth_chan_*).

The reference frames a stream with `chunks_mut(fft_len)` (`waterfall`, src/util/plot.rs:46-68): disjoint, rectangular
frames.  `Channelizer` weights L = P * M samples with a real prototype, folds them modulo M, transforms M points and
advances by the hop D: P = 1 is a windowed (D < M: overlapped) spectrogram, P > 1 the polyphase channelizer (D = M
critically sampled, D < M oversampled)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .context import DeviceF32, DeviceF64, DeviceVec, LEVEL_NORM
from .fft import SIGN_REF_FWD, Scale

PHASE_FRAME, PHASE_STREAM = 0, 1
RECT, HANN, HAMMING, SINC_HAMMING = 0, 1, 2, 3
_KINDS = {"rect": RECT, "hann": HANN, "hamming": HAMMING, "sinc_hamming": SINC_HAMMING}
_PHASES = {"frame": PHASE_FRAME, "stream": PHASE_STREAM}


def prototype(kind, channels, taps_per_channel):
    """channels * taps_per_channel real taps (float32), computed in f64 on the host: RECT, HANN and HAMMING (periodic
    windows), SINC_HAMMING (the low-pass of cutoff fs / (2 channels), unit DC gain).  Needs no context."""
    kind = _KINDS[kind.lower()] if isinstance(kind, str) else int(kind)
    channels, taps_per_channel = int(channels), int(taps_per_channel)
    out = np.empty(max(channels * taps_per_channel, 1), np.float32)
    check(_lib.load().aeth_chan_prototype(kind, channels, taps_per_channel, out.ctypes.data_as(C.c_void_p)))
    return out[:channels * taps_per_channel]


class _Bank:
    """what Channelizer and Synthesizer share: the handle's life, its read-outs, the coercion of a call's vectors"""
    _prefix = None                                 # of the C names: "aeth_chan_" / "aeth_synth_"

    def __init__(self, ctx, proto, channels, hop=None, phase=PHASE_FRAME, max_frames=0):
        self.ctx = ctx
        self._lib = _lib.load()
        proto = np.ascontiguousarray(proto, dtype=np.float32).reshape(-1)
        hop = channels if hop is None else hop
        phase = _PHASES[phase.lower()] if isinstance(phase, str) else int(phase)
        h = C.c_void_p()
        check(self._c("create")(ctx.h, proto.ctypes.data_as(C.c_void_p), proto.size, int(channels), int(hop), phase, int(max_frames),
                                C.byref(h)))
        self.h = h

    def _c(self, name):
        return getattr(self._lib, self._prefix + name)

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self._c("destroy")(self.h)
                self.h = None
        except Exception:
            pass

    @property
    def channels(self): return self._c("channels")(self.h)
    @property
    def ntaps(self): return self._c("ntaps")(self.h)
    @property
    def hop(self): return self._c("hop")(self.h)
    @property
    def phase(self): return self._c("phase")(self.h)
    @property
    def tile(self): return self._c("tile")(self.h)

    @property
    def route(self):
        """the inner plan's route (grammar: include/aether_hip.h, aeth_fft_route)"""
        return self._c("route")(self.h).decode()

    def _vecs(self, x, hist):
        if not isinstance(x, DeviceVec):
            x = self.ctx.vec(x)
        if hist is not None and not isinstance(hist, DeviceVec):
            hist = self.ctx.vec(hist)
        return x, hist


class Channelizer(_Bank):
    """Channelizer(ctx, proto, channels, hop=None, phase="frame"): `proto` holds P * channels real taps, hop defaults to
    `channels`.  phase="frame": every frame's phase refers to its own first sample (STFT); phase="stream": to the
    first sample ever fed (pass the global number of a call's first frame as `first_frame`)."""
    _prefix = "aeth_chan_"

    def frames(self, n):
        """frames a call over n input samples makes (n must be a multiple of the hop)"""
        return int(n) // self.hop

    def _args(self, x, hist):
        x, hist = self._vecs(x, hist)
        if hist is not None and hist.n != self.ntaps - self.hop:
            raise _lib.LengthMismatch(_lib.E_LEN, f"history holds {hist.n} samples, ntaps - hop = {self.ntaps - self.hop}")
        return x, hist, (hist._p() if hist is not None else None)

    def fold(self, x, hist=None, first_frame=0, out=None):
        """the front end alone: frames(x.n) * channels folded samples -> DeviceVec"""
        x, hist, hp = self._args(x, hist)
        out = DeviceVec(self.ctx, self.frames(x.n) * self.channels) if out is None else out
        check(self._lib.aeth_chan_fold(self.h, hp, x._p(), x.n, int(first_frame), out._p(), out.n))
        return out

    def exec(self, x, hist=None, first_frame=0, sign=SIGN_REF_FWD, s=Scale.NONE, out=None):
        """fold, then the transform of every frame -> DeviceVec of frames(x.n) * channels bins"""
        x, hist, hp = self._args(x, hist)
        out = DeviceVec(self.ctx, self.frames(x.n) * self.channels) if out is None else out
        check(self._lib.aeth_chan_exec(self.h, hp, x._p(), x.n, int(first_frame), sign, s.kind, s.x, out._p(), out.n))
        return out

    def levels(self, x, hist=None, first_frame=0, sign=SIGN_REF_FWD, s=Scale.NONE, mirror=False, kind=LEVEL_NORM, out=None):
        """fold, transform, vec_mirror if `mirror`, then the level of every bin -> DeviceF32 (`waterfall`,
        util/plot.rs:46-68, with a window and overlap)"""
        x, hist, hp = self._args(x, hist)
        out = DeviceF32(self.ctx, self.frames(x.n) * self.channels) if out is None else out
        check(self._lib.aeth_chan_exec_levels(self.h, hp, x._p(), x.n, int(first_frame), sign, s.kind, s.x, 1 if mirror else 0,
                                              int(kind), out._p(), out.n))
        return out

    @property
    def sums_chunk(self):
        """frames per chunk of `sums` (the launch geometry: the order of its additions)"""
        return self._lib.aeth_chan_sums_chunk(self.h)

    @property
    def sums_fused(self):
        """does `sums` without general=True take the one-kernel route?"""
        return bool(self._lib.aeth_chan_sums_fused(self.h))

    def sums(self, x, hist=None, first_frame=0, sign=SIGN_REF_FWD, s=Scale.NONE, mirror=False, block=0, general=False,
             want=("sum", "max")):
        """averaged spectra: fold, transform, vec_mirror if `mirror`, then per bin the sum and the maximum of q = |X|^2
        (f64) over rows of `block` frames (0: one row over the whole call) -> (sum, max) as DeviceF64 of rows * channels
        values; a plane that `want` does not name is None.  Welch's periodogram is sum / frames, the max plane is a
        spectrum analyser's max hold.  general=True never takes the one-kernel route (same bytes)."""
        x, hist, hp = self._args(x, hist)
        frames, block = self.frames(x.n), int(block)
        rows = -(-frames // block) if 0 < block < frames else 1
        n_out = rows * self.channels
        sm = DeviceF64(self.ctx, n_out) if "sum" in want else None
        mx = DeviceF64(self.ctx, n_out) if "max" in want else None
        check(self._lib.aeth_chan_exec_sums(self.h, hp, x._p(), x.n, int(first_frame), sign, s.kind, s.x, 1 if mirror else 0, block,
                                            1 if general else 0, sm._p() if sm else None, mx._p() if mx else None, n_out))
        return sm, mx
