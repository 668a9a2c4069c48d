"""Moving-window detectors on the device (include/aether_hip.h, aeth_mov_*): what a burst receiver starts with when it
does not know where the burst begins.

The reference has none.  For every sample, the sum of the last `window` lag terms x[j] * conj(x[j - lag]) (P) and of the
last `window` powers (R), and the metric |P|^2 / (R(i) R(i - lag)) -- the delay-and-correlate timing metric of Schmidl and
Cox -- or, for the POWER kind, the moving mean power.  `exec` hands out the planes, `search` only records: the best
candidate of every `block` samples and of the call, with the f64 sums there, whose angle `freq_step` turns into the `Nco`
step that removes the carrier offset.  The f64 sums are defined bit for bit (tests/mov_truth.py restates them)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import MovPeak, check
from ._records import DeviceRecordArray, _vec, n_blocks   # noqa: F401  (n_blocks: public here)
from .context import DeviceF32, DeviceVec

LAG, POWER = 0, 1

# one record as numpy sees it (struct aeth_mov_peak: 64 bytes, no padding)
PEAK_DTYPE = np.dtype([("index", np.uint64), ("first", np.uint64), ("p_re", np.float64), ("p_im", np.float64), ("r", np.float64),
                       ("r_lag", np.float64), ("metric", np.float32), ("n_nan", np.uint32), ("reserved", np.uint64)])


def history(kind, window, lag=0):
    """samples in front of x a call takes as `hist`.  Needs no context."""
    return _lib.load().aeth_mov_history(int(kind), int(window), int(lag))


def grid(kind, window):
    """a stream cut at a multiple of this, and continued with the last `history` samples, gives the planes of one call"""
    return _lib.load().aeth_mov_grid(int(kind), int(window))


class DevicePeaks(DeviceRecordArray):
    """`count` records on the device, filled by `search_into` (stream-ordered, no wait)."""

    DTYPE = PEAK_DTYPE


def _hist(ctx, hist, kind, window, lag):
    if hist is None:
        return None
    hist = _vec(ctx, hist)
    need = history(kind, window, lag)
    if hist.n != need:
        raise _lib.LengthMismatch(_lib.E_LEN, f"history holds {hist.n} samples, window {window} at lag {lag} takes {need}")
    return hist


def exec_into(ctx, x, kind, window, lag=0, hist=None, p=None, r=None, m=None):
    """the planes that are given (p: DeviceVec, r and m: DeviceF32, each of len(x)); stream-ordered, no wait"""
    x = _vec(ctx, x)
    hist = _hist(ctx, hist, kind, window, lag)
    check(_lib.load().aeth_mov_exec(ctx.h, int(kind), int(window), int(lag), hist._p() if hist is not None else None, x._p(), x.n,
                                    p._p() if p is not None else None, r._p() if r is not None else None,
                                    m._p() if m is not None else None))


def exec(ctx, x, kind, window, lag=0, hist=None, want=("p", "r", "m")):     # noqa: A001  (the library's name for the call)
    """-> {"p": DeviceVec, "r": DeviceF32, "m": DeviceF32} with the planes named in `want`"""
    x = _vec(ctx, x)
    out = {}
    if "p" in want:
        out["p"] = DeviceVec(ctx, x.n)
    if "r" in want:
        out["r"] = DeviceF32(ctx, x.n)
    if "m" in want:
        out["m"] = DeviceF32(ctx, x.n)
    exec_into(ctx, x, kind, window, lag, hist, out.get("p"), out.get("r"), out.get("m"))
    return out


def search_into(ctx, x, kind, window, lag, r_min, threshold, peaks, hist=None, block=0, best=False):
    """the block records of x into the DevicePeaks `peaks` (None: none are kept); best=True waits and returns the record
    over the whole call"""
    x = _vec(ctx, x)
    hist = _hist(ctx, hist, kind, window, lag)
    b = MovPeak() if best else None
    check(_lib.load().aeth_mov_search(ctx.h, int(kind), int(window), int(lag), float(r_min), float(threshold),
                                      hist._p() if hist is not None else None, x._p(), x.n, int(block),
                                      peaks._p() if peaks is not None else None, C.byref(b) if best else None))
    return b


def search(ctx, x, kind, window, lag, r_min, threshold, hist=None, block=0):
    """-> (records, best): one record per `block` samples as a structured array (PEAK_DTYPE; None when block == 0) and
    the record over the whole call as a MovPeak.  A candidate has a metric that is not NaN and window powers >= r_min;
    `index` is the candidate with the largest metric, `first` the lowest one with metric >= threshold (len(x): none)."""
    x = _vec(ctx, x)
    peaks = DevicePeaks(ctx, n_blocks(x.n, block)) if block else None
    best = search_into(ctx, x, kind, window, lag, r_min, threshold, peaks, hist, block, best=True)
    return (peaks.to_host() if peaks is not None else None), best


def _peak(p):
    """anything that holds one record -> MovPeak"""
    if p is None or isinstance(p, MovPeak):
        return p
    if isinstance(p, complex):
        return MovPeak(0, 0, p.real, p.imag, 0.0, 0.0, 0.0, 0, 0)
    return MovPeak(int(p["index"]), int(p["first"]), float(p["p_re"]), float(p["p_im"]), float(p["r"]), float(p["r_lag"]),
                   float(p["metric"]), int(p["n_nan"]), 0)


def freq_step(p, lag):
    """the Nco step word that REMOVES the offset the lag sum of a record (MovPeak, a row of the structured array, or a
    complex P) has seen"""
    p = _peak(p)
    return int(_lib.load().aeth_mov_freq_step(C.byref(p) if p is not None else None, int(lag)))
