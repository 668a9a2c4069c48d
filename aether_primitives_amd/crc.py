"""Frame checks on the device: CRC attach and check over bit frames, and bit packing (include/aether_hip.h, aeth_crc_*
and aeth_bits_*).

The reference has nothing of the kind.  A `Crc` is a width r <= 64, the generator's low r coefficients, init and xorout;
bits are one byte per bit, first bit first, and the check bits go out highest coefficient first (802.11, 3GPP).  Frames are
contiguous and of one length: `registers` is the streaming primitive, `attach` appends the r check bits to every frame,
`check` compares them and strips the payload.  Only the verdict has to leave the device: `check` returns the per-frame
`diff` words, the payload and a two-word summary {n_bad, first_bad}.  `pack_bits` / `unpack_bits` move between one byte per
bit and eight bits per byte in either bit order."""
import ctypes as C

import numpy as np

from . import _lib
from ._device import DeviceArray, Handle
from ._lib import check
from .modulation import DeviceBits

ROUTE_FRAMES, ROUTE_LONG = 1, 2                 # AETH_CRC_ROUTE_*
LSB_FIRST, MSB_FIRST = 0, 1                     # AETH_BITS_*
LANE_CHUNK = 16                                 # bytes a lane takes at a time on the frames route
GROUP_TILE = 64 * LANE_CHUNK                    # bytes the largest group takes in one pass


class DeviceU64(DeviceArray):
    """Device-resident `[u64]`: CRC registers and diff words."""

    DTYPE = np.dtype(np.uint64)


class CrcSummary(DeviceU64):
    """The two words of aeth_crc_summary on the device; `.to_host()` -> (n_bad, first_bad)."""

    def __init__(self, ctx):
        super().__init__(ctx, 2)

    def to_host(self):
        n_bad, first_bad = super().to_host()
        return int(n_bad), int(first_bad)


def named(name):
    """-> (r, poly, init, xorout) of a catalogue name (host only)"""
    r, poly, init, xorout = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint64()
    check(_lib.load().aeth_crc_named(name.encode(), C.byref(r), C.byref(poly), C.byref(init), C.byref(xorout)))
    return r.value, poly.value, init.value, xorout.value


def host_register(r, poly, init, xorout, bits):
    """the definition on host memory: the register of `bits` (one byte per bit) started from init"""
    bits = np.ascontiguousarray(bits, np.uint8)
    reg = C.c_uint64()
    check(_lib.load().aeth_crc_host(r, poly, init, xorout, bits.ctypes.data_as(C.c_void_p), bits.size, C.byref(reg)))
    return reg.value


def _bits(ctx, x):
    return x if isinstance(x, DeviceBits) else DeviceBits(ctx, np.asarray(x).size, x)


def pack_bits(bits, order=LSB_FIRST, out=None):
    """one byte per bit -> ceil(n / 8) bytes, as a `DeviceBits` buffer holding bytes"""
    nbytes = (bits.n + 7) // 8
    if out is None:
        out = DeviceBits(bits.ctx, nbytes)
    check(_lib.load().aeth_bits_pack(bits.ctx.h, C.c_void_p(bits.ptr), bits.n, int(order), C.c_void_p(out.ptr), out.n))
    return out


def unpack_bits(packed, order=LSB_FIRST, nbits=None, out=None):
    """bytes -> `nbits` (default 8 per byte) bytes of 0 / 1"""
    if out is None:
        out = DeviceBits(packed.ctx, 8 * packed.n if nbits is None else int(nbits))
    check(_lib.load().aeth_bits_unpack(packed.ctx.h, C.c_void_p(packed.ptr), packed.n, int(order), C.c_void_p(out.ptr), out.n))
    return out


DeviceBits.pack_bits = pack_bits
DeviceBits.unpack_bits = unpack_bits


class Crc(Handle):
    """Crc(ctx, r, poly, init=0, xorout=0): the object owns its weight table and the long route's scratch."""

    DESTROY = "aeth_crc_destroy"

    def __init__(self, ctx, r, poly, init=0, xorout=0):
        super().__init__(ctx)
        check(self._lib.aeth_crc_create(ctx.h, int(r), int(poly), int(init), int(xorout), C.byref(self.h)))
        self.r, self.poly, self.init, self.xorout = int(r), int(poly), int(init), int(xorout)

    @classmethod
    def named(cls, ctx, name):
        return cls(ctx, *named(name))

    @property
    def residue(self):
        """the register (before xorout) any frame followed by its own check bits leaves"""
        return int(self._lib.aeth_crc_residue(self.h))

    @property
    def route_frame_bits(self):
        return int(self._lib.aeth_crc_route_frame_bits(self.h))

    def route(self, L, F=1):
        return int(self._lib.aeth_crc_route(self.h, int(L), int(F)))

    def frames_per_workgroup(self, frame_bytes):
        return int(self._lib.aeth_crc_frames_per_workgroup(self.h, int(frame_bytes)))

    def registers(self, bits, L, F=None, state=None, out=None):
        """F frames of L bits -> DeviceU64 of registers (no xorout), frame f started from state[f] or from init"""
        bits = _bits(self.ctx, bits)
        F = (bits.n // L if L else 0) if F is None else int(F)
        assert bits.n >= L * F
        if out is None:
            out = DeviceU64(self.ctx, F)
        check(self._lib.aeth_crc_exec(self.h, C.c_void_p(bits.ptr), int(L), F, C.c_void_p(state.ptr) if state is not None else None,
                                      C.c_void_p(out.ptr)))
        return out

    def attach(self, bits, L, out=None):
        """frames of L bits -> frames of L + r bytes: the message & 1, then the check bits"""
        bits = _bits(self.ctx, bits)
        F = bits.n // L if L else 0
        assert bits.n == L * F
        if out is None:
            out = DeviceBits(self.ctx, F * (L + self.r))
        check(self._lib.aeth_crc_attach(self.h, C.c_void_p(bits.ptr), int(L), F, C.c_void_p(out.ptr)))
        return out

    def check(self, frames, L, mask=0, diff=True, payload=True, summary=True):
        """frames of L + r bytes -> (diff DeviceU64, payload DeviceBits, summary): each None when not asked for;
        summary=True gives a `CrcSummary` on the device, summary="host" downloads it as (n_bad, first_bad)"""
        frames = _bits(self.ctx, frames)
        F = frames.n // (L + self.r)
        assert frames.n == F * (L + self.r)
        d = DeviceU64(self.ctx, F) if diff else None
        p = DeviceBits(self.ctx, F * L) if payload else None
        s = CrcSummary(self.ctx) if summary else None
        ptr = lambda b: C.c_void_p(b.ptr) if b is not None else None
        check(self._lib.aeth_crc_check(self.h, C.c_void_p(frames.ptr), int(L), F, int(mask), ptr(d), ptr(p), ptr(s)))
        if summary == "host":
            s = s.to_host()
        return d, p, s
