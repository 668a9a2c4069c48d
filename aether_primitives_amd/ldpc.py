"""Quasi-cyclic LDPC codes on the device: a systematic encoder and a layered normalised min-sum decoder in integers
(include/aether_hip.h, aeth_ldpc_*).

The reference has nothing of the kind.  A code is a table of rows x cols circulant blocks of size z: entry -1 is a zero
block, entry s the identity shifted by s.  N = cols z coded bits carry K = N - rows z information bits.  Bits are one byte
per bit, soft values int8 with the convention of `demod_soft` (positive: bit 0).  `encode` writes the information bits
followed by the parity bits; `decode` returns the hard decisions and, per codeword, a record {iterations, unsatisfied}:
only bits and the verdict have to leave the device."""
import ctypes as C

import numpy as np

from . import _lib
from ._device import DeviceArray, Handle
from ._lib import check
from .modulation import DeviceBits, DeviceSoft

EARLY, PAYLOAD = 1, 2                           # AETH_LDPC_*
MAX_ITER = 1000
MAX_STATE = 65536                               # bytes of decoder state per codeword: 2 N + E z

RECORD = np.dtype([("iterations", np.uint32), ("unsatisfied", np.uint32)])


class Code(C.Structure):
    """aeth_ldpc_code"""
    _fields_ = [("rows", C.c_uint32), ("cols", C.c_uint32), ("z", C.c_uint32), ("shift", C.c_void_p)]


def _code(shift, z):
    """-> (Code, the int32 table it points into)"""
    tab = np.ascontiguousarray(shift, np.int32)
    assert tab.ndim == 2, "shift is a rows x cols table"
    return Code(tab.shape[0], tab.shape[1], int(z), tab.ctypes.data), tab


def generator(shift, z):
    """P = B^-1 A of H = [A | B] as a uint8 matrix [M][K] (host only): parity = P u over GF(2)"""
    code, tab = _code(shift, z)
    rows, cols = tab.shape
    M, K = rows * int(z), (cols - rows) * int(z)
    kw = (max(K, 0) + 63) // 64
    words = np.zeros(max(M * kw, 1), np.uint64)
    check(_lib.load().aeth_ldpc_generator(C.byref(code), words.ctypes.data_as(C.c_void_p), M * kw))
    bits = np.unpackbits(words[:M * kw].view(np.uint8), bitorder="little").reshape(M, kw * 64)
    return bits[:, :K].copy()


def staircase(rows, cols, z, col_weight=3, seed=0):
    """A test code: every information column gets `col_weight` distinct random rows with random shifts; the parity part is
    identities on the diagonal and on the first sub-diagonal, which is always invertible."""
    rng = np.random.default_rng(seed)
    shift = np.full((rows, cols), -1, np.int32)
    for c in range(cols - rows):
        for r in rng.choice(rows, size=min(col_weight, rows), replace=False):
            shift[r, c] = rng.integers(0, z)
    for r in range(rows):
        shift[r, cols - rows + r] = 0
        if r:
            shift[r, cols - rows + r - 1] = 0
    return shift


class DeviceRecords(DeviceArray):
    """Device-resident `[aeth_ldpc_record]`; `.to_host()` -> structured array with `iterations` and `unsatisfied`."""

    DTYPE = RECORD


class Ldpc(Handle):
    """Ldpc(ctx, shift, z): the object owns the generator P and the shift table on the device."""

    DESTROY = "aeth_ldpc_destroy"

    def __init__(self, ctx, shift, z):
        super().__init__(ctx)
        code, tab = _code(shift, z)
        check(self._lib.aeth_ldpc_create(ctx.h, C.byref(code), C.byref(self.h)))
        self.shift = tab.copy()

    n = property(lambda self: int(self._lib.aeth_ldpc_n(self.h)))
    k = property(lambda self: int(self._lib.aeth_ldpc_k(self.h)))
    rows = property(lambda self: int(self._lib.aeth_ldpc_rows(self.h)))
    cols = property(lambda self: int(self._lib.aeth_ldpc_cols(self.h)))
    z = property(lambda self: int(self._lib.aeth_ldpc_z(self.h)))
    edges = property(lambda self: int(self._lib.aeth_ldpc_edges(self.h)))
    lds_bytes = property(lambda self: int(self._lib.aeth_ldpc_lds_bytes(self.h)))
    group = property(lambda self: int(self._lib.aeth_ldpc_group(self.h)))

    def encode(self, bits, out=None):
        """F K information bits -> F N coded bits: the information bits & 1, then the parity bits"""
        if not isinstance(bits, DeviceBits):
            bits = DeviceBits(self.ctx, np.asarray(bits).size, bits)
        F = bits.n // self.k
        if out is None:
            out = DeviceBits(self.ctx, F * self.n)
        check(self._lib.aeth_ldpc_encode(self.h, C.c_void_p(bits.ptr), bits.n, C.c_void_p(out.ptr), out.n))
        return out

    def decode(self, soft, max_iter=20, early=True, payload=False, records=True, out=None):
        """F N soft values -> (DeviceBits of F N hard decisions, or F K with payload=True; DeviceRecords or None)"""
        if not isinstance(soft, DeviceSoft):
            soft = DeviceSoft(self.ctx, np.asarray(soft).size, soft)
        F = soft.n // self.n
        if out is None:
            out = DeviceBits(self.ctx, F * (self.k if payload else self.n))
        rec = DeviceRecords(self.ctx, F) if records else None
        flags = (EARLY if early else 0) | (PAYLOAD if payload else 0)
        check(self._lib.aeth_ldpc_decode(self.h, C.c_void_p(soft.ptr), soft.n, int(max_iter), flags, C.c_void_p(out.ptr), out.n,
                                         C.c_void_p(rec.ptr) if rec is not None else None))
        return out, rec
