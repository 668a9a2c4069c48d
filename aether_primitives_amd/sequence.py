"""sequence::expand / sequence::generate (reference: src/sequence.rs:18-53) for linear generators, on the device.

Every generator the reference documents is a linear recurrence over GF(2), seq[n] = seq[n-d1] ^ seq[n-d2] ^ ...
(`|n, s| (s[n-28] + s[n-31]) % 2`, :42): a *register* here is the tuple of its delays.  `Sequence` generates any range
[skip, skip + n) of 1 .. 4 registers XORed together, fused with its consumer (bits, scramble, chips, spread), so the
sequence itself never touches memory.  Bits are one byte per bit, as in the reference."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .context import DeviceVec
from .modulation import DeviceBits


class _SeqReg(C.Structure):
    # struct aeth_seq_reg
    _fields_ = [("delays", C.POINTER(C.c_uint32)), ("ndelays", C.c_size_t)]


def _reg(delays):
    d = (C.c_uint32 * max(len(delays), 1))(*[int(x) for x in delays])
    return _SeqReg(C.cast(d, C.POINTER(C.c_uint32)), len(delays)), d


def expand(seed, length):                                      # sequence.rs:18-21
    """seed's bits, least significant first, one byte each.  The reference shifts by i and panics (debug build) for
    length > 64; so does this."""
    if length > 64:
        raise OverflowError("attempt to shift right with overflow")
    return np.array([(int(seed) >> i) & 1 for i in range(length)], np.uint8)


def window(delays, init, skip):
    """The 64 sequence bits at [skip, skip + 64) of one register, bit i = seq[skip + i] (host only: aeth_seq_window)."""
    reg, keep = _reg(delays)
    w = C.c_uint64()
    check(_lib.load().aeth_seq_window(C.byref(reg), int(init) & (2 ** 64 - 1), int(skip), C.byref(w)))
    return w.value


def _pack(init_bits):
    return sum((int(b) & 1) << i for i, b in enumerate(init_bits))


def generate(init_bits, delays, n, ctx=None):                  # sequence.rs:47-53
    """sequence::generate(init, |n, s| (sum s[n - d]) % 2, len) in the reference's shape: a host array comes back.
    `init` is returned unchanged when n <= len(init), longer than n as it may be (:48).  len(init) must reach the
    largest delay (the reference's closure would index below zero) and at most 64.  With a Context the device
    generates; without one the host walks the windows (aeth_seq_window)."""
    init_bits = np.ascontiguousarray(init_bits, np.uint8)
    if n <= init_bits.size:
        return init_bits.copy()
    order = max(delays)
    if not order <= init_bits.size <= 64:
        raise ValueError(f"init holds {init_bits.size} bits: the generator looks {order} back, and 64 is the most")
    # the recurrence only reads the last `order` values: restart it from there (a byte counts by its lowest bit, as in
    # the closure's sum % 2); the init itself is passed through as it is
    out = np.empty(n, np.uint8)
    out[:init_bits.size] = init_bits
    base = init_bits.size - order
    init = _pack(init_bits[base:])
    m = n - base
    if ctx is not None:
        tail = Sequence(ctx, delays).bits(init, m, skip=0, host=True)
    else:
        tail = np.empty(m, np.uint8)
        for p in range(0, m, 64):
            w = window(delays, init, p)
            k = min(64, m - p)
            tail[p:p + k] = [(w >> i) & 1 for i in range(k)]
    out[init_bits.size:] = tail[order:]
    return out


class Sequence:
    """Sequence(ctx, (28, 31))  or  Sequence(ctx, (28, 31), (28, 29, 30, 31)): 1 .. 4 registers, XORed.
    `init` is one word per register (bit i = seq[i], as `expand` unpacks it); a single int serves one register."""

    def __init__(self, ctx, *regs):
        self.ctx = ctx
        self._lib = _lib.load()
        self.regs = tuple(tuple(int(d) for d in r) for r in regs)
        built = [_reg(r) for r in self.regs]
        arr = (_SeqReg * max(len(built), 1))(*[b[0] for b in built])
        h = C.c_void_p()
        check(self._lib.aeth_seq_create(ctx.h, arr, len(built), C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self._lib.aeth_seq_destroy(self.h)
                self.h = None
        except Exception:
            pass

    @property
    def nregs(self): return self._lib.aeth_seq_nregs(self.h)
    @property
    def chunk(self): return self._lib.aeth_seq_chunk(self.h)

    def order(self, reg=0):
        return self._lib.aeth_seq_order(self.h, reg)

    def _init(self, init):
        vals = [init] if np.isscalar(init) else list(init)
        if len(vals) != len(self.regs):
            raise ValueError(f"{len(vals)} init words for {len(self.regs)} registers")
        return (C.c_uint64 * len(vals))(*[int(v) & (2 ** 64 - 1) for v in vals])

    def window(self, init, skip=0):
        """the object's 64 output bits at [skip, skip + 64), on the host"""
        w = 0
        for r, v in zip(self.regs, self._init(init)):
            w ^= window(r, v, skip)
        return w

    def bits(self, init, n, skip=0, out=None, host=False):
        """c[i] for i in [skip, skip + n) -> DeviceBits (host=True: a numpy array, through aeth_host_seq_bits)"""
        if host:
            a = np.empty(int(n), np.uint8)
            check(self._lib.aeth_host_seq_bits(self.h, self._init(init), int(skip), a.ctypes.data_as(C.c_void_p), a.size))
            return a
        out = DeviceBits(self.ctx, n) if out is None else out
        check(self._lib.aeth_seq_bits(self.h, self._init(init), int(skip), C.c_void_p(out.ptr), out.n))
        return out

    def scramble(self, init, bits, skip=0, out=None):
        """(bits & 1) ^ c; out=bits scrambles in place"""
        if not isinstance(bits, DeviceBits):
            bits = DeviceBits(self.ctx, len(bits), bits)
        out = DeviceBits(self.ctx, bits.n) if out is None else out
        if out.n != bits.n:
            raise _lib.LengthMismatch(_lib.E_LEN, "Vectors must have same length")
        check(self._lib.aeth_seq_scramble(self.h, self._init(init), int(skip), C.c_void_p(bits.ptr), C.c_void_p(out.ptr), bits.n))
        return out

    def chips(self, init, n, skip=0, zero=1 + 1j, one=-1 - 1j, out=None):
        """c ? one : zero (defaults: GENERIC_BPSK_TABLE, modulation.rs:77) -> DeviceVec"""
        out = DeviceVec(self.ctx, n) if out is None else out
        z, o = (np.complex64(v) for v in (zero, one))
        check(self._lib.aeth_seq_chips(self.h, self._init(init), int(skip), _lib.Cf32(z.real, z.imag), _lib.Cf32(o.real, o.imag),
                                       out._p(), out.n))
        return out

    def spread(self, init, sym, sf, skip=0, out=None):
        """every symbol repeated sf times, negated where c == 1; sf=1 with out=sym scrambles the symbols in place"""
        if not isinstance(sym, DeviceVec):
            sym = self.ctx.vec(sym)
        out = DeviceVec(self.ctx, sym.n * int(sf)) if out is None else out
        check(self._lib.aeth_seq_spread(self.h, self._init(init), int(skip), sym._p(), sym.n, int(sf), out._p(), out.n))
        return out


class LteGold:
    """The pseudo-random sequence of 3GPP TS 36.211 7.2 (the reference's doc example is its x1 half, sequence.rs:34-46):
    c(n) = x1(n + 1600) ^ x2(n + 1600), x1 from init 1, x2 from c_init."""
    NC = 1600

    def __init__(self, ctx):
        self.seq = Sequence(ctx, (28, 31), (28, 29, 30, 31))

    def c(self, c_init, n, out=None, host=False):
        return self.seq.bits((1, c_init), n, skip=self.NC, out=out, host=host)


def lte_gold(ctx):
    return LteGold(ctx)
