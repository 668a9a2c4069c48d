"""Synchronisation estimators on the device (include/aether_hip.h, aeth_sync_*): what tells a receiver the offsets that
`Nco` and `ArbResampler` remove.

The reference has none.  `line` sums a non-linearity of the samples against the oscillator's phasor (SQUARE with step =
word(-1 / sps): the symbol-timing line of Oerder and Meyr; POW<M> with no words: the M-th power carrier phase); `lag` sums
pw_M(x[i]) * conj(pw_M(x[i - lag])) (carrier frequency).  Both are read-only f64 reductions whose records are defined bit
for bit, one per `block` samples and a total; only records leave the device."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import SyncRecord, check
from ._records import DeviceRecordArray, _vec, n_blocks   # noqa: F401  (n_blocks: public here)
from .nco import _Words

SQUARE, POW1, POW2, POW4, POW8 = 0, 1, 2, 4, 8
_MASK = (1 << 64) - 1

# one record as numpy sees it (struct aeth_sync_record: 48 bytes, no padding)
RECORD_DTYPE = np.dtype([("re", np.float64), ("im", np.float64), ("mass", np.float64), ("n", np.uint64),
                         ("n_nonfinite", np.uint64), ("reserved", np.uint64)])


def chunk():
    """samples one workgroup sums; blocks shorter than this take a workgroup each.  Needs no context."""
    return _lib.load().aeth_sync_chunk()


class DeviceRecords(DeviceRecordArray):
    """`count` records on the device, filled by `line_into` / `lag_into` (stream-ordered, no wait)."""

    DTYPE = RECORD_DTYPE


def _record(r):
    """anything that holds one record -> SyncRecord"""
    if r is None or isinstance(r, SyncRecord):
        return r
    if isinstance(r, complex):
        return SyncRecord(r.real, r.imag, 0.0, 0, 0, 0)
    return SyncRecord(float(r["re"]), float(r["im"]), float(r["mass"]), int(r["n"]), int(r["n_nonfinite"]), 0)


def line_into(ctx, x, kind, rec, words=None, position=0, block=0, total=False):
    """the line records of x into the DeviceRecords `rec` (None: none are kept); total=True waits and returns the total"""
    x = _vec(ctx, x)
    w = _Words(*(int(v) & _MASK for v in words)) if words is not None else None
    tot = SyncRecord() if total else None
    check(_lib.load().aeth_sync_line(ctx.h, int(kind), C.byref(w) if w is not None else None, int(position), x._p(), x.n, int(block),
                                     rec._p() if rec is not None else None, C.byref(tot) if total else None))
    return tot


def lag_into(ctx, x, power, lag, rec, hist=None, block=0, total=False):
    """the lag records of x into the DeviceRecords `rec` (None: none are kept); `hist`: the `lag` samples in front of x"""
    x = _vec(ctx, x)
    if hist is not None:
        hist = _vec(ctx, hist)
        if hist.n != int(lag):
            raise _lib.LengthMismatch(_lib.E_LEN, f"history holds {hist.n} samples, the lag is {lag}")
    tot = SyncRecord() if total else None
    check(_lib.load().aeth_sync_lag(ctx.h, int(power), int(lag), hist._p() if hist is not None else None, x._p(), x.n, int(block),
                                    rec._p() if rec is not None else None, C.byref(tot) if total else None))
    return tot


def line(ctx, x, kind, words=None, position=0, block=0):
    """-> (records, total): one record per `block` samples as a structured array (RECORD_DTYPE; None when block == 0)
    and the total as a SyncRecord.  `words` = (phase, step, rate) of the oscillator, None for plain sums; `position` is
    the stream position of x[0]."""
    x = _vec(ctx, x)
    rec = DeviceRecords(ctx, n_blocks(x.n, block)) if block else None
    tot = line_into(ctx, x, kind, rec, words, position, block, total=True)
    return (rec.to_host() if rec is not None else None), tot


def lag(ctx, x, power, lag, hist=None, block=0):     # noqa: A002  (the issue's name for the argument)
    """-> (records, total) of the delay-and-multiply sum of the `power`-th power at `lag` samples"""
    x = _vec(ctx, x)
    rec = DeviceRecords(ctx, n_blocks(x.n, block)) if block else None
    tot = lag_into(ctx, x, power, lag, rec, hist, block, total=True)
    return (rec.to_host() if rec is not None else None), tot


def turns(r):
    """atan2(im, re) / (2 pi) of a record (SyncRecord, a row of the structured array, or a complex); 0 for a zero sum"""
    r = _record(r)
    return float(_lib.load().aeth_sync_turns(C.byref(r) if r is not None else None))


def freq_step(r, power, lag):                        # noqa: A002
    """the Nco step word that REMOVES the offset a lag sum of that power and lag has seen"""
    r = _record(r)
    return int(_lib.load().aeth_sync_freq_step(C.byref(r) if r is not None else None, int(power), int(lag)))


def timing_phase(r, sps):
    """the ArbResampler phase (Q32.32) of the first symbol instant, for a SQUARE line taken with step = word(-1 / sps)"""
    r = _record(r)
    return int(_lib.load().aeth_sync_timing_phase(C.byref(r) if r is not None else None, float(sps)))
