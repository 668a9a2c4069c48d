"""Reed-Solomon codes on the device: a systematic encoder and a bounded-distance errors-and-erasures decoder over
symbol-interleaved frames (include/aether_hip.h, aeth_rs_*).

The reference has nothing of the kind.  Symbols are bytes over GF(2^m), 3 <= m <= 8.  A frame of depth I holds I
codewords, symbol j of codeword i at byte j I + i; `encode` leaves the data bytes in place and appends the I r parity
bytes.  `decode` returns the corrected frames (or their data part), a record {corrected, status} per codeword and a
summary {n_failed, n_corrected}: only payload and verdicts have to leave the device."""
import ctypes as C

import numpy as np

from . import _lib
from ._device import DeviceArray, Handle
from ._lib import check
from .modulation import DeviceBits

PAYLOAD = 1                                     # AETH_RS_*
MAX_ROOTS, MAX_DEPTH = 64, 64

RECORD = np.dtype([("corrected", np.uint32), ("status", np.uint32)])
SUMMARY = np.dtype([("n_failed", np.uint64), ("n_corrected", np.uint64)])


class Code(C.Structure):
    """aeth_rs_code: RS(n, n - nroots) over GF(2^m); poly carries its x^m term"""
    _fields_ = [("m", C.c_uint32), ("poly", C.c_uint32), ("fcr", C.c_uint32), ("prim", C.c_uint32), ("nroots", C.c_uint32), ("n", C.c_uint32)]

    k = property(lambda self: self.n - self.nroots)

    def __repr__(self):
        return f"Code(m={self.m}, poly={self.poly:#x}, fcr={self.fcr}, prim={self.prim}, nroots={self.nroots}, n={self.n})"


def named(name):
    """the catalogue: 'ccsds-255-223', 'ccsds-255-239', 'dvb-204-188', 'rs-15-11' (host only)"""
    code = Code()
    check(_lib.load().aeth_rs_named(name.encode(), C.byref(code)))
    return code


def _code(code):
    if isinstance(code, str):
        return named(code)
    if isinstance(code, Code):
        return code
    return Code(*(int(v) for v in code))


def generator(code):
    """the coefficients of g, lowest first, r + 1 of them (host only)"""
    code = _code(code)
    g = np.zeros(MAX_ROOTS + 1, np.uint8)
    check(_lib.load().aeth_rs_generator(C.byref(code), g.ctypes.data_as(C.c_void_p), g.size))
    return g[:code.nroots + 1].copy()


def host_encode(code, data, depth=1):
    """the definition on host memory: frames of depth * k bytes -> frames of depth * n bytes"""
    code = _code(code)
    data = np.ascontiguousarray(data, np.uint8).ravel()
    F = data.size // max(depth * code.k, 1)
    out = np.zeros(max(F * depth * code.n, 1), np.uint8)
    check(_lib.load().aeth_rs_host_encode(C.byref(code), data.ctypes.data_as(C.c_void_p), data.size, depth, out.ctypes.data_as(C.c_void_p),
                                          F * depth * code.n))
    return out[:F * depth * code.n]


def host_decode(code, coded, erasures=None, depth=1, payload=False):
    """the definition on host memory -> (bytes, records, summary)"""
    code = _code(code)
    coded = np.ascontiguousarray(coded, np.uint8).ravel()
    era = None if erasures is None else np.ascontiguousarray(erasures, np.uint8).ravel()
    assert era is None or era.size == coded.size, "one erasure flag per coded byte"
    F = coded.size // max(depth * code.n, 1)
    nb = code.k if payload else code.n
    out = np.zeros(max(F * depth * nb, 1), np.uint8)
    rec = np.zeros(max(F * depth, 1), RECORD)
    summary = np.zeros(1, SUMMARY)
    check(_lib.load().aeth_rs_host_decode(C.byref(code), coded.ctypes.data_as(C.c_void_p), coded.size,
                                          era.ctypes.data_as(C.c_void_p) if era is not None else None, depth, PAYLOAD if payload else 0,
                                          out.ctypes.data_as(C.c_void_p), F * depth * nb, rec.ctypes.data_as(C.c_void_p),
                                          summary.ctypes.data_as(C.c_void_p)))
    return out[:F * depth * nb], rec[:F * depth], summary[0]


class DeviceRecords(DeviceArray):
    """Device-resident `[aeth_rs_record]`; `.to_host()` -> structured array with `corrected` and `status`."""

    DTYPE = RECORD


class DeviceSummary(DeviceArray):
    """Device-resident aeth_rs_summary; `.to_host()` waits and returns a record with `n_failed` and `n_corrected`."""

    DTYPE = SUMMARY

    def __init__(self, ctx):
        super().__init__(ctx, 1)

    def to_host(self):
        return super().to_host()[0]


class Rs(Handle):
    """Rs(ctx, code_or_name): the object owns the field tables on the device."""

    DESTROY = "aeth_rs_destroy"

    def __init__(self, ctx, code):
        super().__init__(ctx)
        self.code = _code(code)
        check(self._lib.aeth_rs_create(ctx.h, C.byref(self.code), C.byref(self.h)))

    n = property(lambda self: int(self._lib.aeth_rs_n(self.h)))
    k = property(lambda self: int(self._lib.aeth_rs_k(self.h)))
    nroots = property(lambda self: int(self._lib.aeth_rs_nroots(self.h)))
    m = property(lambda self: int(self._lib.aeth_rs_m(self.h)))
    group = property(lambda self: int(self._lib.aeth_rs_group(self.h)))

    def lds_bytes(self, depth=1):
        return int(self._lib.aeth_rs_lds_bytes(self.h, depth))

    def encode(self, data, depth=1, out=None):
        """F frames of depth * k bytes -> F frames of depth * n bytes: the data in place (& 2^m - 1), then the parity"""
        if not isinstance(data, DeviceBits):
            data = DeviceBits(self.ctx, np.asarray(data).size, data)
        F = data.n // (depth * self.k) if 1 <= depth <= MAX_DEPTH else 0
        if out is None:
            out = DeviceBits(self.ctx, F * depth * self.n)
        check(self._lib.aeth_rs_encode(self.h, C.c_void_p(data.ptr), data.n, depth, C.c_void_p(out.ptr), out.n))
        return out

    def decode(self, coded, erasures=None, depth=1, payload=False, records=True, summary=True, out=None):
        """F frames of depth * n bytes -> (DeviceBits of F frames of depth * n bytes, or depth * k with payload=True;
        DeviceRecords or None; DeviceSummary or None).  erasures: one byte per coded byte, non-zero = erased."""
        if not isinstance(coded, DeviceBits):
            coded = DeviceBits(self.ctx, np.asarray(coded).size, coded)
        if erasures is not None and not isinstance(erasures, DeviceBits):
            erasures = DeviceBits(self.ctx, np.asarray(erasures).size, erasures)
        assert erasures is None or erasures.n == coded.n, "one erasure flag per coded byte"
        F = coded.n // (depth * self.n) if 1 <= depth <= MAX_DEPTH else 0
        if out is None:
            out = DeviceBits(self.ctx, F * depth * (self.k if payload else self.n))
        rec = DeviceRecords(self.ctx, F * depth) if records else None
        summ = DeviceSummary(self.ctx) if summary else None
        check(self._lib.aeth_rs_decode(self.h, C.c_void_p(coded.ptr), coded.n, C.c_void_p(erasures.ptr) if erasures is not None else None, depth,
                                       PAYLOAD if payload else 0, C.c_void_p(out.ptr), out.n, C.c_void_p(rec.ptr) if rec is not None else None,
                                       C.c_void_p(summ.ptr) if summ is not None else None))
        return out, rec, summ
