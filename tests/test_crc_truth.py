"""CPU: the CRC definition against its catalogue check values, against Python's own CRCs, and the algebra the device side
relies on (residue, burst detection), through the restatement of tests/crc_truth.py and through the library's host
functions aeth_crc_named / aeth_crc_host, which run the same plain C++ header as the device side's host algebra."""
import binascii
import zlib

import numpy as np
import pytest

import crc_truth as T
from aether_primitives_amd import _lib, crc

DATA = b"123456789"


def msb_bits(data):
    return np.unpackbits(np.frombuffer(data, np.uint8))


def lsb_bits(data):
    return np.unpackbits(np.frombuffer(data, np.uint8), bitorder="little")


@pytest.mark.parametrize("name", sorted(T.NAMED))
def test_named_rows_reproduce_their_check_values(name):
    r, poly, init, xorout, value = T.NAMED[name]
    assert crc.named(name) == (r, poly, init, xorout)
    if name == "crc-32":                                   # the caller unpacks LSB first; the check bits packed LSB first are zlib's
        bits = lsb_bits(DATA)
        for reg in (T.register(r, poly, init, bits), crc.host_register(r, poly, init, xorout, bits)):
            fcs = T.pack(T.check_bits(r, reg ^ xorout), True).tobytes()
            assert fcs == zlib.crc32(DATA).to_bytes(4, "little") == bytes.fromhex("2639f4cb")
        return
    bits = msb_bits(DATA)
    assert T.register(r, poly, init, bits) ^ xorout == value
    assert crc.host_register(r, poly, init, xorout, bits) ^ xorout == value
    assert int(T.registers(r, poly, init, bits, bits.size, 1)[0]) ^ xorout == value


def test_unknown_name_lists_the_known_ones():
    with pytest.raises(_lib.AetherError) as e:
        crc.named("crc-32/nope")
    assert e.value.code == _lib.E_ARG
    for name in T.NAMED:
        assert name in str(e.value)


def test_python_crcs_agree_on_random_strings():
    rng = np.random.default_rng(11)
    for n in list(range(0, 40)) + [63, 64, 65, 255, 256, 299, 300]:
        data = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        m, l = msb_bits(data), lsb_bits(data)
        for name, ref in (("crc-16/ibm-3740", binascii.crc_hqx(data, 0xFFFF)), ("crc-16/xmodem", binascii.crc_hqx(data, 0))):
            r, poly, init, xorout, _ = T.NAMED[name]
            assert T.register(r, poly, init, m) ^ xorout == ref, (name, n)
            assert crc.host_register(r, poly, init, xorout, m) ^ xorout == ref, (name, n)
        r, poly, init, xorout, _ = T.NAMED["crc-32"]
        for reg in (T.register(r, poly, init, l), crc.host_register(r, poly, init, xorout, l)):
            assert T.pack(T.check_bits(r, reg ^ xorout), True).tobytes() == zlib.crc32(data).to_bytes(4, "little"), n


def params():
    rng = np.random.default_rng(5)
    out = [(n,) + T.NAMED[n][:4] for n in sorted(T.NAMED)]
    for r in T.WIDTHS:
        for k in range(3):
            out.append((f"random r={r} #{k}",) + T.random_params(rng, r))
    return out


@pytest.mark.parametrize("p", params(), ids=lambda p: p[0])
def test_residue_is_the_register_over_message_and_check_bits(p):
    _, r, poly, init, xorout = p
    rng = np.random.default_rng(r)
    lib = _lib.load()
    residue = T.register(r, poly, 0, T.check_bits(r, xorout))
    for L in (0, 1, 17, 100):
        bits = rng.integers(0, 256, L, dtype=np.uint8)
        frame = T.attach(r, poly, init, xorout, bits, L, 1)
        assert T.register(r, poly, init, frame) == residue
        assert crc.host_register(r, poly, init, xorout, frame) == residue
    # the library's own value needs an object, hence a context: tests/test_gpu_crc.py compares Crc.residue with this
    if (r, poly, init, xorout) == T.NAMED["crc-32"][:4]:
        assert residue == 0xC704DD7B
    if (r, poly, init, xorout) == T.NAMED["crc-16/genibus"][:4]:
        assert residue == 0x1D0F
    assert lib.aeth_crc_residue(None) == 0


def test_vectorised_and_long_restatements_equal_the_plain_loop():
    rng = np.random.default_rng(3)
    for r in T.WIDTHS:
        _, poly, init, _ = T.random_params(rng, r)
        bits = rng.integers(0, 256, 7 * 333, dtype=np.uint8)
        state = rng.integers(0, 1 << 62, 7, dtype=np.uint64) & np.uint64((1 << r) - 1)
        got = T.registers(r, poly, init, bits, 333, 7, state=state)
        assert got.tolist() == [T.register(r, poly, int(state[f]), bits[f * 333:(f + 1) * 333]) for f in range(7)]
        assert T.register_long(r, poly, init, bits, chunk=100) == T.register(r, poly, init, bits)
        assert T.register_long(r, poly, init, bits[:99], chunk=100) == T.register(r, poly, init, bits[:99])
    data = rng.integers(0, 256, 100000, dtype=np.uint8)
    r, poly, init, xorout, _ = T.NAMED["crc-32"]
    reg = T.register_long(r, poly, init, lsb_bits(data.tobytes()))
    assert T.pack(T.check_bits(r, reg ^ xorout), True).tobytes() == zlib.crc32(data.tobytes()).to_bytes(4, "little")


@pytest.mark.parametrize("name", ("crc-8", "crc-16/xmodem"))
def test_every_burst_up_to_the_width_is_detected(name):
    """every error pattern that starts and ends with a flipped bit and spans at most r bits, at every position of an
    attached frame of a 40-bit message"""
    r, poly, init, xorout, _ = T.NAMED[name]
    rng = np.random.default_rng(9)
    L = 40
    frame = T.attach(r, poly, init, xorout, rng.integers(0, 2, L, dtype=np.uint8), L, 1)
    patterns = [1] + [(1 << (w - 1)) | (mid << 1) | 1 for w in range(2, r + 1) for mid in range(1 << (w - 2))]
    cases = [(pat, pos) for pat in patterns for pos in range(L + r - pat.bit_length() + 1)]
    bad = np.repeat(frame[None, :], len(cases), axis=0)
    for i, (pat, pos) in enumerate(cases):
        w = pat.bit_length()
        bad[i, pos:pos + w] ^= np.array([(pat >> (w - 1 - k)) & 1 for k in range(w)], np.uint8)
    diff, _, (n_bad, first) = T.check(r, poly, init, xorout, bad, L, len(cases))
    assert n_bad == len(cases) and first == 0 and diff.all()
    assert not T.check(r, poly, init, xorout, frame, L, 1)[0].any()
