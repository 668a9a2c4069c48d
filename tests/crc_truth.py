"""The definition of include/aether_hip.h (aeth_crc_*, aeth_bits_*) restated as plain loops and numpy: register, check
bits, attach, check, pack and unpack.  Nothing here calls the library."""
import numpy as np

NAMED = {                      # name: (r, poly, init, xorout, check value over b"123456789")
    "crc-8": (8, 0x07, 0, 0, 0xF4),
    "crc-8/lte": (8, 0x9B, 0, 0, 0xEA),
    "crc-16/xmodem": (16, 0x1021, 0, 0, 0x31C3),
    "crc-16/ibm-3740": (16, 0x1021, 0xFFFF, 0, 0x29B1),
    "crc-16/genibus": (16, 0x1021, 0xFFFF, 0xFFFF, 0xD64E),
    "crc-24/lte-a": (24, 0x864CFB, 0, 0, 0xCDE703),
    "crc-24/lte-b": (24, 0x800063, 0, 0, 0x23EF52),
    "crc-32/bzip2": (32, 0x04C11DB7, 0xFFFFFFFF, 0xFFFFFFFF, 0xFC891918),
    "crc-32": (32, 0x04C11DB7, 0xFFFFFFFF, 0xFFFFFFFF, None),          # bytes unpacked LSB first: see test_crc_truth.py
    "crc-64/ecma-182": (64, 0x42F0E1EBA9EA3693, 0, 0, 0x6C40DF5F0B497347),
}
WIDTHS = (1, 3, 8, 16, 24, 32, 33, 63, 64)


def register(r, poly, reg, bits):
    """the register after `bits` (any integers: only the lowest bit counts), started from `reg`"""
    m = (1 << r) - 1
    for b in np.asarray(bits).ravel().tolist():
        fb = ((reg >> (r - 1)) & 1) ^ (int(b) & 1)
        reg = (reg << 1) & m
        if fb:
            reg ^= poly
    return reg


def check_bits(r, value):
    return np.array([(value >> (r - 1 - j)) & 1 for j in range(r)], np.uint8)


def word(bits):
    """bits read as a word, first bit highest"""
    v = 0
    for b in np.asarray(bits).ravel().tolist():
        v = (v << 1) | (int(b) & 1)
    return v


def registers(r, poly, init, bits, L, F, state=None):
    """the registers of F frames of L bits: the same loop, all frames of a bit position at a time (uint64 columns)"""
    bits = (np.asarray(bits, np.uint8).reshape(F, L) & 1).astype(np.uint64)
    reg = np.full(F, init, np.uint64) if state is None else np.asarray(state, np.uint64).copy()
    m, p, top = np.uint64((1 << r) - 1), np.uint64(poly), np.uint64(r - 1)
    one = np.uint64(1)
    for i in range(L):
        fb = ((reg >> top) & one) ^ bits[:, i]
        reg = ((reg << one) & m) ^ (p * fb)
    return reg


def attach(r, poly, init, xorout, bits, L, F):
    bits = np.asarray(bits, np.uint8).reshape(F, L)
    out = np.empty((F, L + r), np.uint8)
    value = registers(r, poly, init, bits, L, F) ^ np.uint64(xorout)
    out[:, :L] = bits & 1
    for j in range(r):
        out[:, L + j] = (value >> np.uint64(r - 1 - j)) & np.uint64(1)
    return out.ravel()


def check(r, poly, init, xorout, frames, L, F, mask=0):
    """-> (diff [F] uint64, payload [F L], (n_bad, first_bad))"""
    frames = np.asarray(frames, np.uint8).reshape(F, L + r)
    recv = np.zeros(F, np.uint64)
    for j in range(r):
        recv |= (frames[:, L + j] & 1).astype(np.uint64) << np.uint64(r - 1 - j)
    diff = recv ^ registers(r, poly, init, frames[:, :L], L, F) ^ np.uint64(xorout) ^ np.uint64(mask)
    bad = np.flatnonzero(diff)
    return diff, (frames[:, :L] & 1).ravel(), (int(bad.size), int(bad[0]) if bad.size else F)


def pack(bits, lsb_first):
    return np.packbits(np.asarray(bits, np.uint8) & 1, bitorder="little" if lsb_first else "big")


def unpack(packed, lsb_first, nbits):
    return np.unpackbits(np.asarray(packed, np.uint8), bitorder="little" if lsb_first else "big")[:nbits]


def random_params(rng, r):
    """(r, odd poly, init, xorout), all below 2^r"""
    m = (1 << r) - 1
    draw = lambda: int(rng.integers(0, 1 << 32)) << 32 | int(rng.integers(0, 1 << 32))
    return r, (draw() & m) | 1, draw() & m, draw() & m


def register_long(r, poly, reg, bits, chunk=4096):
    """the register of one long frame without a Python step per bit: the frame is cut into chunks whose registers from 0
    come from `registers` (all chunks of a bit position at a time), and since a step is linear over GF(2) the state after
    a chunk is (the state before it run over `chunk` zero bits) ^ (the chunk's register from 0).  The zero run is a linear
    map, tabulated once from the r unit states.  tests/test_crc_truth.py checks this against `register`."""
    bits = np.asarray(bits, np.uint8)
    n_full = bits.size // chunk
    if n_full:
        regs = registers(r, poly, 0, bits[:n_full * chunk], chunk, n_full)
        units = registers(r, poly, 0, np.zeros((r, chunk), np.uint8), chunk, r, state=np.uint64(1) << np.arange(r, dtype=np.uint64))
        units = [int(u) for u in units]
        for c in regs.tolist():
            run = 0
            for j in range(r):
                if (reg >> j) & 1:
                    run ^= units[j]
            reg = run ^ int(c)
    return register(r, poly, reg, bits[n_full * chunk:])
