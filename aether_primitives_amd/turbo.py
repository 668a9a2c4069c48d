"""Turbo codes on the device: two recursive systematic encoders with their tails and a windowed max-log-MAP iterative
decoder (include/aether_hip.h, aeth_turbo_*).

The reference has nothing of the kind.  A code is a constituent code `(k, fb, ff)` -- `named("lte")`, `named("ccsds")`,
`named("k3")` or the caller's own -- a frame of 8 <= K <= 8192 information bits, a permutation `pi` of K entries
(`qpp(K, f1, f2)` or any other), a window and a warm-up length.  A coded frame has N = 3 K + 4 (k - 1) bytes, planar:
systematic, first parity, second parity, the two tails.  Bits are one byte per bit, soft values int8 with the convention of
`demod_soft` (positive: bit 0).  `decode` returns the K decisions of the last iteration run and, per codeword, a record
`{iterations, disagreements}`; with `early=True` a codeword stops after an iteration whose two constituents agree
(examples/turbo.py).  Only records, verdicts and payloads have to leave the device."""
import ctypes as C

import numpy as np

from . import _lib
from ._device import DeviceArray, Handle
from ._lib import check
from .modulation import DeviceBits, DeviceSoft

EARLY = 1                                       # AETH_TURBO_EARLY
MIN_K, MAX_K = 8, 8192

RECORD = np.dtype([("iterations", np.uint32), ("disagreements", np.uint32)])


class Code(C.Structure):
    """aeth_turbo_code"""
    _fields_ = [("k", C.c_uint32), ("fb", C.c_uint32), ("ff", C.c_uint32)]


def named(name):
    """(k, fb, ff) of "lte", "ccsds" or "k3" (host only)"""
    c = Code()
    check(_lib.load().aeth_turbo_named(str(name).encode(), C.byref(c)))
    return (int(c.k), int(c.fb), int(c.ff))


def qpp(K, f1, f2):
    """uint32 [K]: pi[i] = (f1 i + f2 i^2) mod K; refused when that is no permutation (host only)"""
    out = np.zeros(K if MIN_K <= K <= MAX_K else 1, np.uint32)
    check(_lib.load().aeth_turbo_qpp(int(K), int(f1), int(f2), out.ctypes.data_as(C.c_void_p), out.size))
    return out


class DeviceRecords(DeviceArray):
    """Device-resident `[aeth_turbo_record]`; `.to_host()` -> structured array with `iterations` and `disagreements`."""

    DTYPE = RECORD


class Turbo(Handle):
    """Turbo(ctx, code, pi, window, warmup): the object owns the interleaver, its inverse and the decoder's alpha store on the
    device.  code: a name of `named` or (k, fb, ff)."""

    DESTROY = "aeth_turbo_destroy"

    def __init__(self, ctx, code, pi, window, warmup):
        super().__init__(ctx)
        k, fb, ff = named(code) if isinstance(code, str) else code
        p = np.ascontiguousarray(pi, np.uint32)
        c = Code(int(k), int(fb), int(ff))
        check(self._lib.aeth_turbo_create(ctx.h, C.byref(c), p.size, p.ctypes.data_as(C.c_void_p), int(window), int(warmup), C.byref(self.h)))
        self.code, self.pi = (int(k), int(fb), int(ff)), p.copy()

    k = property(lambda self: int(self._lib.aeth_turbo_k(self.h)))
    n = property(lambda self: int(self._lib.aeth_turbo_n(self.h)))
    states = property(lambda self: int(self._lib.aeth_turbo_states(self.h)))
    window = property(lambda self: int(self._lib.aeth_turbo_window(self.h)))
    warmup = property(lambda self: int(self._lib.aeth_turbo_warmup(self.h)))
    windows = property(lambda self: int(self._lib.aeth_turbo_windows(self.h)))
    group = property(lambda self: int(self._lib.aeth_turbo_group(self.h)))
    lds_bytes = property(lambda self: int(self._lib.aeth_turbo_lds_bytes(self.h)))

    def encode(self, bits, out=None):
        """F K information bits -> F N coded bits"""
        if not isinstance(bits, DeviceBits):
            bits = DeviceBits(self.ctx, np.asarray(bits).size, bits)
        F = bits.n // self.k
        if out is None:
            out = DeviceBits(self.ctx, F * self.n)
        check(self._lib.aeth_turbo_encode(self.h, C.c_void_p(bits.ptr), bits.n, C.c_void_p(out.ptr), out.n))
        return out

    def decode(self, soft, max_iter=8, early=False, records=True, out=None):
        """F N soft values -> (DeviceBits of F K decisions; DeviceRecords or None)"""
        if not isinstance(soft, DeviceSoft):
            soft = DeviceSoft(self.ctx, np.asarray(soft).size, soft)
        F = soft.n // self.n
        if out is None:
            out = DeviceBits(self.ctx, F * self.k)
        rec = DeviceRecords(self.ctx, F) if records else None
        check(self._lib.aeth_turbo_decode(self.h, C.c_void_p(soft.ptr), soft.n, int(max_iter), EARLY if early else 0, C.c_void_p(out.ptr), out.n,
                                          rec._p() if rec is not None else None))
        return out, rec
