"""CPU: aeth_seq_window -- the 64 sequence bits at [skip, skip + 64) of one register, by powers of the 64 x 64 step
matrix on the host (csrc/aeth_seq_core.h) -- against known answers (tests/golden/sequence_kat.json), the reference's own
test vector (src/sequence.rs:61-68), the periods of the maximal-length registers, and a plain-loop restatement of
sequence::generate (tests/seq_truth.py).  Nothing here touches a device."""
import ctypes as C
import json
import os
import random
import sys

import numpy as np
import pytest

import seq_truth
from aether_primitives_amd import _lib, sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "sequence_kat.json")))
w = sequence.window


def h(s):
    return int(s, 16)


def bits_of(window, n=64):
    return [(window >> i) & 1 for i in range(n)]


def test_simple_sequence_of_the_reference():
    k = KAT["simple_sequence"]
    assert bits_of(w(k["delays"], h(k["init"]), 0), 6) == k["first"] == [1, 0, 1, 1, 0, 1]        # sequence.rs:61-68


def test_m_sequence_of_order_7():
    k = KAT["m7"]
    d, init = k["delays"], h(k["init"])
    packed = (w(d, init, 0) | (w(d, init, 64) << 64)) & ((1 << 127) - 1)
    assert packed == h(k["packed_0_126"])
    assert w(d, init, 127) == w(d, init, 0)
    # ... and these are the chips examples/sync.py plants: 0 -> +1, 1 -> -1
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    try:
        import sync
    finally:
        sys.path.pop(0)
    chips = 1.0 - 2.0 * np.array(bits_of(packed, 127))
    assert (chips.astype(np.complex64) == sync.m_sequence()).all()
    assert (seq_truth.m_sequence_bits() == np.array(bits_of(packed, 127), np.uint8)).all()


def test_lte_x1():
    k = KAT["x1"]
    d, init = k["delays"], h(k["init"])
    w0 = w(d, init, 0)
    # x1(31) = x1(3) ^ x1(0) = 1 is the first one after the init bit: nothing else is set below x1(59) = x1(31) ^ x1(28)
    assert w0 & ((1 << 59) - 1) == (1 << 0) | (1 << 31)
    assert w0 == h(k["window_0"])
    assert k["far_skip"] == 2 ** 40 + 12345 and w(d, init, k["far_skip"]) == h(k["far_window"])
    for p in k["period_checks"]:
        assert w(d, init, p) == w(d, init, p + k["period"])


def test_lte_gold_c():
    k = KAT["lte"]
    for c_init, want in k["c"].items():
        assert w(k["x1"], 1, k["nc"]) ^ w(k["x2"], h(c_init), k["nc"]) == h(want), c_init


def test_order_64():
    k = KAT["order64"]
    assert 2 ** 50 + 7 == 1125899906842631
    for skip, want in k["windows"].items():
        assert w(k["delays"], h(k["init"]), int(skip)) == h(want), skip


def test_positions_below_the_order_are_the_init_bits_and_higher_bits_are_ignored():
    assert w((60, 61, 63, 64), 0x0123456789abcdef, 0) == 0x0123456789abcdef
    assert w((3, 5), 0b10110, 0) & 31 == 0b10110
    assert w((3, 5), 0b10110 | (0xabc << 5), 0) == w((3, 5), 0b10110, 0)
    assert w((6, 7), 0, 0) == 0 and w((6, 7), 0, 2 ** 63) == 0                                    # all-zero init: zeros
    assert w((28, 31), 1, 2 ** 64 - 1) == seq_truth.py_window((28, 31), 1, 2 ** 64 - 1)           # any uint64_t skips


def test_random_registers_against_the_plain_loop():
    r = random.Random(815)
    for _ in range(200):
        delays = tuple(r.sample(range(1, 65), r.randint(1, 6)))
        init, skip = r.getrandbits(64), r.randrange(5000)
        s = seq_truth.plain(delays, init, skip + 64)
        want = sum(int(s[skip + i]) << i for i in range(64))
        assert w(delays, init, skip) == want, (delays, hex(init), skip)


@pytest.mark.parametrize("delays", [(1,), (1, 2), (6, 7), (28, 31), (28, 29, 30, 31), (60, 61, 63, 64), (3, 17, 40)])
def test_the_truth_helpers_agree_with_each_other(delays):
    """the GPU tests take their truth from seq_truth.block and seq_truth.py_window: both against the plain loop"""
    init = 0x9e3779b97f4a7c15
    n = 70000 + 1024 * max(delays)
    a = seq_truth.plain(delays, init, n)
    assert (seq_truth.block(delays, init, n) == a).all()
    for skip in (0, 1, 63, 64, 1600, 4097, n - 64):
        assert bits_of(seq_truth.py_window(delays, init, skip)) == list(a[skip:skip + 64]), skip
    assert (seq_truth.one(delays, init, 1600, 3000) == a[1600:4600]).all()
    state = a[5000:5064]
    assert (seq_truth.block(delays, 0, 66000, state=state) == a[5000:71000]).all()


def test_the_truth_is_right_where_the_long_device_call_is_compared():
    """tests/test_gpu_sequence_long.py compares slices of a 2^30-position call around the starts of chunks 2^j
    (C = 16384 positions each) with seq_truth.truth, which there goes through py_window and block(state=...): the same
    route against the period of the order-7 register, which uses neither"""
    regs, inits, ch, n = ((6, 7),), (0x7f,), 16384, 4160
    period = seq_truth.m_sequence_bits()
    tiled = np.tile(period, n // 127 + 2)
    for skip in (0, 1600, 2 ** 40 + 12345):
        for j in range(18):
            for p in ((ch << j) - 64, ch << j, ((1 << j) - 1) * ch + 4096):
                got = seq_truth.truth(regs, inits, skip + p, n)
                assert (got == tiled[(skip + p) % 127:][:n]).all(), (skip, j, p)


def test_mirror_expand_and_generate_keep_the_reference_quirks():
    assert list(sequence.expand(1 + 4 + 16, 32)) == [1, 0, 1, 0, 1] + [0] * 27                    # sequence.rs:8-16
    with pytest.raises(OverflowError):
        sequence.expand(1, 65)                                                                    # :20 panics in debug
    assert list(sequence.generate([1, 0], (1, 2), 6)) == [1, 0, 1, 1, 0, 1]                       # :61-68
    assert list(sequence.generate([1, 0, 1], (1, 2), 2)) == [1, 0, 1]                             # len <= init.len(): as is
    x1 = sequence.generate(sequence.expand(1, 31), (28, 31), 1600)                                # the doc example, :42-46
    assert x1.size == 1600 and (x1 == seq_truth.plain((28, 31), 1, 1600)).all()
    # an init longer than the order: the recurrence continues from its last values
    init = [1, 1, 0, 1, 0, 0, 1, 0, 1]
    s = list(init)
    while len(s) < 300:
        s.append((s[-2] + s[-5]) % 2)
    assert list(sequence.generate(init, (2, 5), 300)) == s


def test_window_refuses_bad_registers():
    lib = _lib.load()
    out = C.c_uint64(0x5a)
    d = (C.c_uint32 * 3)(3, 5, 3)
    reg = sequence._SeqReg(C.cast(d, C.POINTER(C.c_uint32)), 3)
    assert lib.aeth_seq_window(C.byref(reg), 1, 0, C.byref(out)) == _lib.E_ARG and b"repeated" in lib.aeth_last_error()
    assert lib.aeth_seq_window(None, 1, 0, C.byref(out)) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    reg.ndelays = 2
    assert lib.aeth_seq_window(C.byref(reg), 1, 0, None) == _lib.E_ARG and b"null" in lib.aeth_last_error()
    assert out.value == 0x5a
