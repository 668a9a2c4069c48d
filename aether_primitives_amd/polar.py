"""Polar codes on the device: the encoder and a successive-cancellation decoder with one bit flip per codeword
(include/aether_hip.h, aeth_polar_*).

The reference has nothing of the kind.  A code is N = 2^n positions, 3 <= n <= 10, and a mask of N bytes: 1 where a
position carries information, 0 where it is frozen.  `rank(n)` orders the positions by an integer polarization weight and
`mask(n, K)` marks the K most reliable; any other mask (the 5G sequence, a design for one SNR) is passed as it is.  Bits
are one byte per bit, soft values int8 with the convention of `demod_soft` (positive: bit 0).  `decode` returns the K
information decisions (or the N re-encoded bits) and, per codeword, a record of the four least reliable information
decisions: the candidates of a CRC-aided SC-Flip decoder, which decodes the frames `Crc.check` calls bad again with
`flip = index[r]` (examples/polar.py).  Only verdicts, records and payloads have to leave the device.

`PolarList(ctx, n, mask, L)` is the list decoder (aeth_polar_list_*): L = 1, 2, 4 or 8 paths per codeword, ordered by their
metrics, and `pick` lets the words of `Crc.check` choose among the L rows on the device (examples/polar_list.py)."""
import ctypes as C

import numpy as np

from . import _lib
from ._device import DeviceArray, Handle
from ._lib import check
from .crc import DeviceU64
from .modulation import DeviceBits, DeviceSoft

CODEWORD = 1                                    # AETH_POLAR_CODEWORD
ALL = 2                                         # AETH_POLAR_ALL
NONE = 0xFFFFFFFF                               # AETH_POLAR_NONE
MIN_N, MAX_N = 3, 10

RECORD = np.dtype([("index", np.uint32, 4), ("abs", np.uint32, 4)])
LIST_RECORD = np.dtype([("metric", np.uint32, 8)])


def rank(n):
    """the 2^n positions, most reliable first (host only)"""
    out = np.zeros(1 << n if MIN_N <= n <= MAX_N else 1, np.uint32)
    check(_lib.load().aeth_polar_rank(int(n), out.ctypes.data_as(C.c_void_p), out.size))
    return out


def mask(n, K):
    """uint8 [2^n]: 1 at the K most reliable positions of `rank(n)` (host only)"""
    out = np.zeros(1 << n if MIN_N <= n <= MAX_N else 1, np.uint8)
    check(_lib.load().aeth_polar_mask(int(n), int(K), out.ctypes.data_as(C.c_void_p), out.size))
    return out


class DeviceRecords(DeviceArray):
    """Device-resident `[aeth_polar_record]`; `.to_host()` -> structured array with `index` and `abs`, four each."""

    DTYPE = RECORD


class DeviceFlips(DeviceArray):
    """Device-resident `[u32]`: one flip position per codeword."""

    DTYPE = np.dtype(np.uint32)


class Polar(Handle):
    """Polar(ctx, n, mask): the object owns the decoder's schedule and the position tables on the device."""

    DESTROY = "aeth_polar_destroy"

    def __init__(self, ctx, n, mask):
        super().__init__(ctx)
        m = np.ascontiguousarray(mask, np.uint8)
        assert m.size == (1 << n if MIN_N <= n <= MAX_N else m.size), "the mask holds 2^n bytes"
        check(self._lib.aeth_polar_create(ctx.h, int(n), m.ctypes.data_as(C.c_void_p), C.byref(self.h)))
        self.mask = m.copy()

    n = property(lambda self: int(self._lib.aeth_polar_n(self.h)))
    k = property(lambda self: int(self._lib.aeth_polar_k(self.h)))
    lanes = property(lambda self: int(self._lib.aeth_polar_lanes(self.h)))
    group = property(lambda self: int(self._lib.aeth_polar_group(self.h)))
    lds_bytes = property(lambda self: int(self._lib.aeth_polar_lds_bytes(self.h)))

    def encode(self, bits, out=None):
        """F K information bits -> F N coded bits"""
        if not isinstance(bits, DeviceBits):
            bits = DeviceBits(self.ctx, np.asarray(bits).size, bits)
        F = bits.n // self.k
        if out is None:
            out = DeviceBits(self.ctx, F * self.n)
        check(self._lib.aeth_polar_encode(self.h, C.c_void_p(bits.ptr), bits.n, C.c_void_p(out.ptr), out.n))
        return out

    def decode(self, soft, flip=None, codeword=False, records=True, out=None):
        """F N soft values -> (DeviceBits of F K decisions, or the F N re-encoded bits with codeword=True; DeviceRecords or
        None).  flip: None, a `DeviceFlips` or F host positions, one per codeword (NONE: no flip)."""
        if not isinstance(soft, DeviceSoft):
            soft = DeviceSoft(self.ctx, np.asarray(soft).size, soft)
        F = soft.n // self.n
        if flip is not None and not isinstance(flip, DeviceFlips):
            flip = DeviceFlips(self.ctx, np.asarray(flip).size, flip)
        assert flip is None or flip.n == F, "one flip position per codeword"
        if out is None:
            out = DeviceBits(self.ctx, F * (self.n if codeword else self.k))
        rec = DeviceRecords(self.ctx, F) if records else None
        check(self._lib.aeth_polar_decode(self.h, C.c_void_p(soft.ptr), soft.n, C.c_void_p(flip.ptr) if flip is not None else None,
                                          CODEWORD if codeword else 0, C.c_void_p(out.ptr), out.n, rec._p() if rec is not None else None))
        return out, rec


class DeviceListRecords(DeviceArray):
    """Device-resident `[aeth_polar_list_record]`; `.to_host()` -> structured array with `metric`, eight each."""

    DTYPE = LIST_RECORD


class DeviceWhich(DeviceArray):
    """Device-resident `[u32]`: per codeword the row `pick` took, or NONE."""

    DTYPE = np.dtype(np.uint32)


class PolarList(Handle):
    """PolarList(ctx, n, mask, L): the list decoder of L paths; the object owns its schedule and the information positions
    on the device."""

    DESTROY = "aeth_polar_list_destroy"

    def __init__(self, ctx, n, mask, L):
        super().__init__(ctx)
        m = np.ascontiguousarray(mask, np.uint8)
        assert m.size == (1 << n if MIN_N <= n <= MAX_N else m.size), "the mask holds 2^n bytes"
        check(self._lib.aeth_polar_list_create(ctx.h, int(n), m.ctypes.data_as(C.c_void_p), int(L), C.byref(self.h)))
        self.mask = m.copy()

    n = property(lambda self: int(self._lib.aeth_polar_list_n(self.h)))
    k = property(lambda self: int(self._lib.aeth_polar_list_k(self.h)))
    paths = property(lambda self: int(self._lib.aeth_polar_list_paths(self.h)))
    lanes = property(lambda self: int(self._lib.aeth_polar_list_lanes(self.h)))
    group = property(lambda self: int(self._lib.aeth_polar_list_group(self.h)))
    lds_bytes = property(lambda self: int(self._lib.aeth_polar_list_lds_bytes(self.h)))

    def decode(self, soft, all=False, codeword=False, records=True, out=None):
        """F N soft values -> (DeviceBits: per codeword the best path's K decisions, with all=True the L paths' in list
        order, with codeword=True the N re-encoded bits in place of the K; DeviceListRecords or None)"""
        if not isinstance(soft, DeviceSoft):
            soft = DeviceSoft(self.ctx, np.asarray(soft).size, soft)
        F = soft.n // self.n
        if out is None:
            out = DeviceBits(self.ctx, F * (self.paths if all else 1) * (self.n if codeword else self.k))
        rec = DeviceListRecords(self.ctx, F) if records else None
        check(self._lib.aeth_polar_list_decode(self.h, C.c_void_p(soft.ptr), soft.n, (ALL if all else 0) | (CODEWORD if codeword else 0),
                                               C.c_void_p(out.ptr), out.n, rec._p() if rec is not None else None))
        return out, rec


def pick(ctx, rows, row_bytes, L, diff, out=None):
    """F L rows of row_bytes bytes and the F L words of `Crc.check` over them -> (DeviceBits of F rows: per codeword the
    first row whose word is zero, row 0 when none is; DeviceWhich: that row's number, or NONE)"""
    if not isinstance(rows, DeviceBits):
        rows = DeviceBits(ctx, np.asarray(rows).size, rows)
    if not isinstance(diff, DeviceU64):
        diff = DeviceU64(ctx, np.asarray(diff).size, diff)
    F = diff.n // L if L else 0
    assert diff.n == F * L and rows.n == F * L * row_bytes, "L rows and L words per codeword"
    if out is None:
        out = DeviceBits(ctx, F * row_bytes)
    which = DeviceWhich(ctx, F)
    check(_lib.load().aeth_polar_list_pick(ctx.h, C.c_void_p(rows.ptr), int(row_bytes), F, int(L), C.c_void_p(diff.ptr), C.c_void_p(out.ptr),
                                           which._p()))
    return out, which
