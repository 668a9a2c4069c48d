"""GPU: aeth_bits_pack / aeth_bits_unpack against numpy.packbits / unpackbits, byte for byte, in both bit orders, at every
alignment 0 .. 15 of both sides, between guard bytes; input bits are drawn from 0 .. 255 so that only the low bit may
count.  End to end: bytes -> unpack LSB first -> crc-32 attach -> pack LSB first is the frame with the usual CRC-32 behind
it, lowest byte first."""
import ctypes as C
import zlib

import numpy as np
import pytest

import aether_primitives_amd as ap
from aether_primitives_amd import _lib, crc
import crc_truth as T
from test_gpu_crc import Mem, mem          # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 7, 8, 9, 127, 128, 129, 8191, 8192, 8193, (1 << 20) + 5)
ORDERS = ((crc.LSB_FIRST, True), (crc.MSB_FIRST, False))


def d_pack(ctx, mem, bits, order, in_off=0, out_off=0):              # noqa: F811
    o = mem.out((bits.size + 7) // 8, out_off)
    _lib.check(_lib.load().aeth_bits_pack(ctx.h, C.c_void_p(mem.inp(bits, in_off)), bits.size, order, mem.ptr(o), (bits.size + 7) // 8))
    return mem.get(o)


def d_unpack(ctx, mem, packed, order, nbits, in_off=0, out_off=0):   # noqa: F811
    o = mem.out(nbits, out_off)
    _lib.check(_lib.load().aeth_bits_unpack(ctx.h, C.c_void_p(mem.inp(packed, in_off)), packed.size, order, mem.ptr(o), nbits))
    return mem.get(o)


@pytest.mark.parametrize("order,lsb", ORDERS)
@pytest.mark.parametrize("nbits", SIZES)
def test_sizes_in_both_orders(ctx, mem, nbits, order, lsb):          # noqa: F811
    rng = np.random.default_rng(nbits)
    x = rng.integers(0, 256, nbits, dtype=np.uint8)
    packed = d_pack(ctx, mem, x, order, 5, 3)
    assert packed.tobytes() == T.pack(x, lsb).tobytes() == np.packbits(x & 1, bitorder="little" if lsb else "big").tobytes()
    assert d_unpack(ctx, mem, packed, order, nbits, 3, 5).tobytes() == (x & 1).tobytes()
    extra = np.concatenate([packed, rng.integers(0, 256, 3, dtype=np.uint8)])         # nbits <= 8 nbytes: the rest is not read into the output
    assert d_unpack(ctx, mem, extra, order, nbits, 1, 9).tobytes() == (x & 1).tobytes()


@pytest.mark.parametrize("order,lsb", ORDERS)
@pytest.mark.parametrize("nbits", (129, 8193))
def test_every_alignment_of_both_sides(ctx, mem, nbits, order, lsb):  # noqa: F811
    rng = np.random.default_rng(nbits + order)
    x = rng.integers(0, 256, nbits, dtype=np.uint8)
    want = T.pack(x, lsb)
    for a in range(16):
        for b in (range(16) if nbits == 129 else (0, 1, 7, 15)):
            assert d_pack(ctx, mem, x, order, a, b).tobytes() == want.tobytes(), (a, b)
            assert d_unpack(ctx, mem, want, order, nbits, b, a).tobytes() == (x & 1).tobytes(), (a, b)
        mem.free()


def test_through_the_python_layer(ctx):
    x = np.random.default_rng(4).integers(0, 256, 1003, dtype=np.uint8)
    bits = ap.DeviceBits(ctx, x.size, x)
    for order, lsb in ORDERS:
        p = bits.pack_bits(order)
        assert p.n == 126 and p.to_host().tobytes() == T.pack(x, lsb).tobytes()
        assert p.unpack_bits(order, nbits=1003).to_host().tobytes() == (x & 1).tobytes()
        assert ap.unpack_bits(p, order).n == 1008


def test_frames_with_the_usual_crc32_behind_them(ctx):
    rng = np.random.default_rng(6)
    F, N = 64, 1500
    data = rng.integers(0, 256, F * N, dtype=np.uint8)
    c = ap.Crc.named(ctx, "crc-32")
    bits = ap.unpack_bits(ap.DeviceBits(ctx, data.size, data), crc.LSB_FIRST)
    framed = ap.pack_bits(c.attach(bits, 8 * N), crc.LSB_FIRST).to_host().tobytes()
    want = b"".join(data[f * N:(f + 1) * N].tobytes() + zlib.crc32(data[f * N:(f + 1) * N].tobytes()).to_bytes(4, "little") for f in range(F))
    assert framed == want
    d, p, s = c.check(ap.unpack_bits(ap.DeviceBits(ctx, len(want), np.frombuffer(want, np.uint8)), crc.LSB_FIRST), 8 * N, summary="host")
    assert s == (0, F) and not d.to_host().any() and ap.pack_bits(p, crc.LSB_FIRST).to_host().tobytes() == data.tobytes()
    c.close()
