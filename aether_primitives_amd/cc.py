"""Convolutional codes on the device: encoder and a block-wise soft-decision Viterbi decoder (include/aether_hip.h,
aeth_cc_*).

The reference has no forward error correction.  A `ConvCode` of constraint length k = 3 .. 7 with n = 2 .. 4 polynomials
(octal convention, current bit at the MSB: K = 7 is (0o171, 0o133)) encodes one byte per bit into n bytes per bit and
decodes int8 soft values (positive: bit 0 likelier, 0: erasure) back into bits.  Everything is integer and defined bit
for bit; the decoder is a causal system with a delay of `traceback` steps."""
import ctypes as C

import numpy as np

from . import _lib
from ._device import Handle
from ._lib import check
from .modulation import DeviceBits, DeviceSoft


class _Code(C.Structure):
    # struct aeth_cc_code
    _fields_ = [("k", C.c_uint32), ("n", C.c_uint32), ("poly", C.c_uint32 * 4)]


class ConvCode(Handle):
    """ConvCode(ctx, k, polys, block, warmup, traceback): output block D, warm-up A and traceback T in trellis steps
    (D + T <= 4096, A <= 4096).  `history` is A + T, the steps of soft values a continued `decode` wants in front."""

    DESTROY = "aeth_cc_destroy"
    NEEDS_CONTEXT = False                                            # the object holds nothing on the device

    def __init__(self, ctx, k, polys, block=512, warmup=64, traceback=64):
        super().__init__(ctx)
        polys = [int(p) for p in polys]
        code = _Code(int(k), len(polys), (C.c_uint32 * 4)(*(polys + [0] * 4)[:4]))
        check(self._lib.aeth_cc_create(ctx.h, C.byref(code), int(block), int(warmup), int(traceback), C.byref(self.h)))
        self.k, self.n, self.polys = int(k), len(polys), tuple(polys)

    @property
    def block(self):
        return int(self._lib.aeth_cc_block(self.h))

    @property
    def warmup(self):
        return int(self._lib.aeth_cc_warmup(self.h))

    @property
    def traceback(self):
        return int(self._lib.aeth_cc_traceback(self.h))

    @property
    def history(self):
        return int(self._lib.aeth_cc_history(self.h))

    def encode(self, bits, hist=None, out=None):
        """c[n t + j] = parity(reg_t & poly[j]) -> DeviceBits of n * len(bits); `hist` is the k - 1 bits before bits[0]
        (None: zeros)"""
        if not isinstance(bits, DeviceBits):
            bits = DeviceBits(self.ctx, len(bits), bits)
        if hist is not None and not isinstance(hist, DeviceBits):
            hist = DeviceBits(self.ctx, len(hist), hist)
        if hist is not None and hist.n != self.k - 1:
            raise _lib.LengthMismatch(_lib.E_LEN, f"history holds {hist.n} bits, k - 1 = {self.k - 1} wanted")
        if out is None:
            out = DeviceBits(self.ctx, bits.n * self.n)
        check(self._lib.aeth_cc_encode(self.h, C.c_void_p(hist.ptr if hist is not None else None), C.c_void_p(bits.ptr), bits.n,
                                       C.c_void_p(out.ptr), out.n))
        return out

    def decode(self, soft, hist=None, out=None):
        """out[o] = the decision for step o - traceback -> DeviceBits of len(soft) / n; `hist` is the `history` steps of
        soft values before soft[0] (None: erasures)"""
        if not isinstance(soft, DeviceSoft):
            soft = DeviceSoft(self.ctx, len(soft), soft)
        if hist is not None and not isinstance(hist, DeviceSoft):
            hist = DeviceSoft(self.ctx, len(hist), hist)
        if hist is not None and hist.n != self.history * self.n:
            raise _lib.LengthMismatch(_lib.E_LEN, f"history holds {hist.n} soft values, {self.history} steps x {self.n} wanted")
        if out is None:
            out = DeviceBits(self.ctx, soft.n // self.n)
        check(self._lib.aeth_cc_decode(self.h, C.c_void_p(hist.ptr if hist is not None else None), C.c_void_p(soft.ptr), soft.n,
                                       C.c_void_p(out.ptr), out.n))
        return out

    def decode_stream(self, soft, known_start=True):
        """a whole stream at once: a history of +127s when the encoder started from the zero state, `traceback` steps of
        erasures behind the stream to flush it, and the `traceback` leading outputs dropped -> DeviceBits of len(soft) / n"""
        if not isinstance(soft, DeviceSoft):
            soft = DeviceSoft(self.ctx, len(soft), soft)
        if soft.n % self.n:
            raise _lib.LengthMismatch(_lib.E_LEN, f"{soft.n} soft values are not a multiple of n = {self.n}")
        T, n, nbits = self.traceback, self.n, soft.n // self.n
        hist = DeviceSoft(self.ctx, self.history * n, np.full(self.history * n, 127, np.int8)) if known_start else None
        padded = DeviceSoft(self.ctx, soft.n + T * n)
        if soft.n:
            check(self._lib.aeth_copy_dev(self.ctx.h, C.c_void_p(padded.ptr), C.c_void_p(soft.ptr), soft.n))
        if T:
            self.ctx.upload(padded.ptr + soft.n, np.zeros(T * n, np.int8))
        full = self.decode(padded, hist)
        out = DeviceBits(self.ctx, nbits)
        if nbits:
            check(self._lib.aeth_copy_dev(self.ctx.h, C.c_void_p(out.ptr), C.c_void_p(full.ptr + T), nbits))
        return out
