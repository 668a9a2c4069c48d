"""CPU: the call frontier the six coding modules share, one table row per call: every overlap refusal with its full text
(each output against each input, each pair of outputs, one unit at the low and at the high end), the same pairs placed
adjacent and then refused by the grid check at 2^31 workgroups, the order of the checks, and the codeword length texts of
ldpc and polar.  Handles and addresses are fakes (those of the test_*_args.py files): every call ends in a refusal, so
nothing reaches device work.  Adjacency is tested where a grid check follows the overlap check (cc, ldpc, rs, polar); behind
the overlap check of the remap, crc, bit-packing and rs host calls comes the work itself."""
import collections
import ctypes as C

import pytest

from aether_primitives_amd import _lib, rs
from aether_primitives_amd.cc import _Code

from test_crc_args import fake_crc
from test_ldpc_args import fake as fake_ldpc
from test_polar_args import fake as fake_polar
from test_rs_args import GOOD, fake as fake_rs

FAKE = (C.c_char * 4096)()
CTX = C.cast(FAKE, C.c_void_p)           # never dereferenced: every call below returns before any device work
BASE = 1 << 50                           # slot i lives at (i + 1) BASE: far enough apart for the counts of the grid limit
E_ARG, E_LEN, E_ALIGN, E_UNSUPPORTED = _lib.E_ARG, _lib.E_LEN, _lib.E_ALIGN, _lib.E_UNSUPPORTED
GRID = "{} {} in one call: more than 2^31 workgroups"


class FakeRemap(C.Structure):
    """what aeth_remap_exec reads of an object before it refuses: the periods and the `reach` vector (begin, end, capacity)"""
    _fields_ = [("ctx", C.c_void_p), ("r_in", C.c_uint32), ("r_out", C.c_uint32), ("g", C.c_uint32), ("tab", C.c_void_p),
                ("reach", C.c_void_p * 3), ("rest", C.c_uint64 * 8)]


REACH = (C.c_uint32 * 2)(1, 2)                                           # the identity map of period 2
REMAP = FakeRemap(CTX.value, 2, 2, 0, None, (C.c_void_p * 3)(C.addressof(REACH), C.addressof(REACH) + 8, C.addressof(REACH) + 8))
POLAR, LDPC, RS, CRC = fake_polar(), fake_ldpc(), fake_rs(), fake_crc()  # N = 32, K = 12, G = 8; N = 30, K = 15, G = 51; RS(15, 11), groups of 64; r = 16
CODE = rs.Code(*GOOD)
CC = C.c_void_p()                                                        # k = 3, n = 2, block 8, warm-up 4, traceback 4: no device needed


@pytest.fixture(scope="module")
def lib():
    lib = _lib.load()
    code = _Code(3, 2, (C.c_uint32 * 4)(0o7, 0o5, 0, 0))
    assert lib.aeth_cc_create(CTX, C.byref(code), 8, 4, 4, C.byref(CC)) == _lib.OK
    yield lib
    assert lib.aeth_cc_destroy(CC) == _lib.OK


def P(v):
    return None if v is None else C.c_void_p(v)


Slot = collections.namedtuple("Slot", "name out align")
# slots: in the order of their home addresses; lens(c): their bytes at count c; call(lib, c, a): the good call at count c
# on the addresses a[name] (None: a null pointer); small: a count far below every limit; io / oo: the overlap texts;
# grid: (count, text) of the refusal that follows the overlap check, or None
Row = collections.namedtuple("Row", "name slots lens call small io oo grid")


def I(name, align=1):
    return Slot(name, False, align)


def O(name, align=1):
    return Slot(name, True, align)


ROWS = (
    Row("cc_encode", (I("hist"), I("bits"), O("coded")), lambda c: (2, c, 2 * c),
        lambda lib, c, a: lib.aeth_cc_encode(CC, P(a["hist"]), P(a["bits"]), c, P(a["coded"]), 2 * c),
        40, "the output overlaps an input", None, (1 << 39, f"{1 << 39} bits need 2^31 workgroups or more")),
    Row("cc_decode", (I("hist"), I("soft"), O("bits")), lambda c: (16, 2 * c, c),
        lambda lib, c, a: lib.aeth_cc_decode(CC, P(a["hist"]), P(a["soft"]), 2 * c, P(a["bits"]), c),
        40, "the output overlaps an input", None, (1 << 38, f"{1 << 38} bits in blocks of 8 need 2^31 workgroups or more")),
    Row("remap_exec", (I("in"), O("out")), lambda c: (c, c),
        lambda lib, c, a: lib.aeth_remap_exec(C.byref(REMAP), P(a["in"]), c, P(a["out"]), c, 0),
        40, "the output overlaps the input", None, None),
    Row("crc_exec", (I("bits"), I("state_in", 8), O("state_out", 8)), lambda c: (8 * c, 8 * c, 8 * c),
        lambda lib, c, a: lib.aeth_crc_exec(C.byref(CRC), P(a["bits"]), 8, c, P(a["state_in"]), P(a["state_out"])),
        5, "the output states overlap an input", None, None),
    Row("crc_attach", (I("in"), O("out")), lambda c: (8 * c, 24 * c),
        lambda lib, c, a: lib.aeth_crc_attach(C.byref(CRC), P(a["in"]), 8, c, P(a["out"])),
        5, "the output overlaps the input", None, None),
    Row("crc_check", (I("in"), O("diff", 8), O("payload"), O("summary", 8)), lambda c: (24 * c, 8 * c, 8 * c, 16),
        lambda lib, c, a: lib.aeth_crc_check(C.byref(CRC), P(a["in"]), 8, c, 0, P(a["diff"]), P(a["payload"]), P(a["summary"])),
        5, "an output overlaps the input", "two outputs overlap", None),
    Row("bits_pack", (I("bits"), O("bytes")), lambda c: (8 * c, c),
        lambda lib, c, a: lib.aeth_bits_pack(CTX, P(a["bits"]), 8 * c, 0, P(a["bytes"]), c),
        5, "the output overlaps the input", None, None),
    Row("bits_unpack", (I("bytes"), O("bits")), lambda c: (c, 8 * c),
        lambda lib, c, a: lib.aeth_bits_unpack(CTX, P(a["bytes"]), c, 0, P(a["bits"]), 8 * c),
        5, "the output overlaps the input", None, None),
    Row("ldpc_encode", (I("bits"), O("coded")), lambda c: (15 * c, 30 * c),
        lambda lib, c, a: lib.aeth_ldpc_encode(C.byref(LDPC), P(a["bits"]), 15 * c, P(a["coded"]), 30 * c),
        3, "the output overlaps the input", None, (8 << 31, GRID.format(8 << 31, "codewords"))),
    Row("ldpc_decode", (I("soft"), O("bits"), O("rec", 4)), lambda c: (30 * c, 30 * c, 8 * c),
        lambda lib, c, a: lib.aeth_ldpc_decode(C.byref(LDPC), P(a["soft"]), 30 * c, 10, 0, P(a["bits"]), 30 * c, P(a["rec"])),
        3, "an output overlaps the input", "the two outputs overlap", (51 << 31, GRID.format(51 << 31, "codewords"))),
    Row("rs_encode", (I("data"), O("coded")), lambda c: (11 * c, 15 * c),
        lambda lib, c, a: lib.aeth_rs_encode(C.byref(RS), P(a["data"]), 11 * c, 1, P(a["coded"]), 15 * c),
        10, "the output overlaps the input", None, (64 << 31, GRID.format(64 << 31, "frames"))),
    Row("rs_decode", (I("in"), I("era"), O("out"), O("rec", 4), O("summary", 8)), lambda c: (15 * c, 15 * c, 15 * c, 8 * c, 16),
        lambda lib, c, a: lib.aeth_rs_decode(C.byref(RS), P(a["in"]), 15 * c, P(a["era"]), 1, 0, P(a["out"]), 15 * c, P(a["rec"]), P(a["summary"])),
        10, "an output overlaps an input", "two outputs overlap", (64 << 31, GRID.format(64 << 31, "frames"))),
    Row("rs_host_encode", (I("data"), O("coded")), lambda c: (11 * c, 15 * c),
        lambda lib, c, a: lib.aeth_rs_host_encode(C.byref(CODE), P(a["data"]), 11 * c, 1, P(a["coded"]), 15 * c),
        10, "the output overlaps the input", None, None),
    Row("rs_host_decode", (I("in"), I("era"), O("out")), lambda c: (15 * c, 15 * c, 15 * c),
        lambda lib, c, a: lib.aeth_rs_host_decode(C.byref(CODE), P(a["in"]), 15 * c, P(a["era"]), 1, 0, P(a["out"]), 15 * c, None, None),
        10, "the output overlaps an input", None, None),
    Row("polar_encode", (I("bits"), O("coded")), lambda c: (12 * c, 32 * c),
        lambda lib, c, a: lib.aeth_polar_encode(C.byref(POLAR), P(a["bits"]), 12 * c, P(a["coded"]), 32 * c),
        3, "the output overlaps the input", None, (1 << 40, GRID.format(1 << 40, "codewords"))),
    Row("polar_decode", (I("soft"), I("flip", 4), O("bits"), O("rec", 4)), lambda c: (32 * c, 4 * c, 12 * c, 32 * c),
        lambda lib, c, a: lib.aeth_polar_decode(C.byref(POLAR), P(a["soft"]), 32 * c, P(a["flip"]), 0, P(a["bits"]), 12 * c, P(a["rec"])),
        3, "an output overlaps an input", "the two outputs overlap", (8 << 31, GRID.format(8 << 31, "codewords"))),
)
BY_NAME = {r.name: r for r in ROWS}
GRIDDED = [r for r in ROWS if r.grid]


def home(row):
    return {s.name: (i + 1) * BASE for i, s in enumerate(row.slots)}


def pairs(row):
    """(output, other, text): every output against every input, then every pair of outputs"""
    outs, ins = [s for s in row.slots if s.out], [s for s in row.slots if not s.out]
    got = [(o, i, row.io) for o in outs for i in ins]
    return got + [(outs[x], outs[y], row.oo) for x in range(len(outs)) for y in range(x + 1, len(outs))]


def placed(row, c, p, q, shared, high):
    """the home addresses, but with p and q sharing `shared` units (0: adjacent) at q's low or high end; the unit is the
    coarser alignment of the two, and the one with the finer alignment moves"""
    a, lens = home(row), dict(zip((s.name for s in row.slots), row.lens(c)))
    mover, fixed = (p, q) if p.align <= q.align else (q, p)
    n = shared * max(p.align, q.align)
    a[mover.name] = a[fixed.name] + lens[fixed.name] - n if high else a[fixed.name] - lens[mover.name] + n
    assert all(a[s.name] % s.align == 0 for s in row.slots), (row.name, a)
    return a


def refused(lib, rc, code, text):
    assert rc == code and lib.aeth_last_error().decode() == text, (rc, lib.aeth_last_error())


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_the_good_call_of_a_row_is_consistent(lib, row):
    """the row's own lengths pass the length checks: with every pointer null the call gets as far as the null check"""
    rc = row.call(lib, row.small, {s.name: None for s in row.slots})
    assert rc == E_ARG and b"null" in lib.aeth_last_error(), (rc, lib.aeth_last_error())


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_every_pair_that_shares_one_unit(lib, row):
    assert len(pairs(row)) == sum(1 for s in row.slots if s.out) * sum(1 for s in row.slots if not s.out) + \
        (0, 0, 1, 3)[sum(1 for s in row.slots if s.out)]
    for p, q, text in pairs(row):
        for high in (False, True):
            refused(lib, row.call(lib, row.small, placed(row, row.small, p, q, 1, high)), E_ARG, text)
            a = placed(row, row.small, p, q, 1, high)                     # ... and with every slot outside the pair absent
            others = {s.name: None for s in row.slots if s not in (p, q) and s.name in OPTIONAL.get(row.name, ())}
            refused(lib, row.call(lib, row.small, {**a, **others}), E_ARG, text)


# the slots a call takes a null pointer for
OPTIONAL = {"cc_encode": ("hist",), "cc_decode": ("hist",), "crc_exec": ("state_in",), "crc_check": ("diff", "payload", "summary"),
            "ldpc_decode": ("rec",), "rs_decode": ("era", "rec", "summary"), "rs_host_decode": ("era",), "polar_decode": ("flip", "rec")}


@pytest.mark.parametrize("row", GRIDDED, ids=[r.name for r in GRIDDED])
def test_adjacent_ranges_pass_and_the_grid_check_refuses(lib, row):
    count, text = row.grid
    refused(lib, row.call(lib, count, home(row)), E_UNSUPPORTED, text)
    for p, q, overlap in pairs(row):
        for high in (False, True):
            refused(lib, row.call(lib, count, placed(row, count, p, q, 0, high)), E_UNSUPPORTED, text)
            refused(lib, row.call(lib, count, placed(row, count, p, q, 1, high)), E_ARG, overlap)   # overlapping + over the grid limit


def test_the_smallest_count_of_two_to_the_31_workgroups(lib):
    """the table's counts are whole groups; the refusal starts one codeword behind 2^31 - 1 full workgroups"""
    for name, per in (("ldpc_decode", 51), ("rs_decode", 64), ("polar_decode", 8)):
        row = BY_NAME[name]
        count = row.grid[0] - per + 1                                    # the smallest count of 2^31 workgroups
        refused(lib, row.call(lib, count, home(row)), E_UNSUPPORTED, row.grid[1].replace(str(row.grid[0]), str(count)))


A, B, D, E, H = (i * BASE for i in range(1, 6))
G32 = 1 << 32

# one bad call per consecutive pair of checks, wrong in both ways: the earlier check answers
ORDER = {
    "polar_decode": (
        (lambda l: l.aeth_polar_decode(C.byref(POLAR), P(A), 31, None, 2, P(B), 12, None), E_ARG, "unknown flag bits 0x2"),
        (lambda l: l.aeth_polar_decode(C.byref(POLAR), None, 31, None, 0, P(B), 12, None), E_LEN, "nsoft 31 is no multiple of N = 32"),
        (lambda l: l.aeth_polar_decode(C.byref(POLAR), None, 32, None, 0, P(B), 12, P(D + 1)), E_ARG, "null pointer"),
        (lambda l: l.aeth_polar_decode(C.byref(POLAR), P(A), 32, P(E + 2), 0, P(A + 31), 12, None), E_ALIGN, "flip_dev not 4-byte aligned"),
        (lambda l: l.aeth_polar_decode(C.byref(POLAR), P(A), 32, None, 0, P(A + 31), 12, P(D + 1)), E_ALIGN, "rec_dev not 4-byte aligned"),
        (lambda l: l.aeth_polar_decode(C.byref(POLAR), P(A), 32 << 34, None, 0, P(A - 1), 12 << 34, None), E_ARG, "an output overlaps an input")),
    "polar_encode": (
        (lambda l: l.aeth_polar_encode(C.byref(POLAR), None, 11, P(B), 32), E_LEN, "nbits 11 is no multiple of K = 12"),
        (lambda l: l.aeth_polar_encode(C.byref(POLAR), P(A), 12 << 40, P(A - 1), 32 << 40), E_ARG, "the output overlaps the input")),
    "ldpc_decode": (
        (lambda l: l.aeth_ldpc_decode(C.byref(LDPC), P(A), 31, 10, 4, P(B), 30, None), E_ARG, "unknown flag bits 0x4"),
        (lambda l: l.aeth_ldpc_decode(C.byref(LDPC), P(A), 31, 1001, 0, P(B), 30, None), E_ARG, "max_iter 1001 above 1000"),
        (lambda l: l.aeth_ldpc_decode(C.byref(LDPC), None, 31, 10, 0, P(B), 30, None), E_LEN, "nsoft 31 is no multiple of N = 30"),
        (lambda l: l.aeth_ldpc_decode(C.byref(LDPC), None, 30, 10, 0, P(B), 30, P(D + 2)), E_ARG, "null pointer"),
        (lambda l: l.aeth_ldpc_decode(C.byref(LDPC), P(A), 30, 10, 0, P(A + 29), 30, P(D + 2)), E_ALIGN, "rec_dev not 4-byte aligned"),
        (lambda l: l.aeth_ldpc_decode(C.byref(LDPC), P(A), 30 * (51 << 31), 10, 0, P(A - 1), 30 * (51 << 31), None), E_ARG, "an output overlaps the input")),
    "ldpc_encode": (
        (lambda l: l.aeth_ldpc_encode(C.byref(LDPC), None, 14, P(B), 30), E_LEN, "nbits 14 is no multiple of K = 15"),
        (lambda l: l.aeth_ldpc_encode(C.byref(LDPC), P(A), 15 * (8 << 31), P(A - 1), 30 * (8 << 31)), E_ARG, "the output overlaps the input")),
    "rs_decode": (
        (lambda l: l.aeth_rs_decode(C.byref(RS), P(A), 15, None, 65, 2, P(B), 15, None, None), E_ARG, "depth 65 outside 1 .. 64"),
        (lambda l: l.aeth_rs_decode(C.byref(RS), P(A), 16, None, 1, 2, P(B), 15, None, None), E_ARG, "unknown flag bits 0x2"),
        (lambda l: l.aeth_rs_decode(C.byref(RS), None, 16, None, 1, 0, P(B), 15, None, None), E_LEN, "nin 16 is no multiple of the frame of 15 bytes"),
        (lambda l: l.aeth_rs_decode(C.byref(RS), None, 15, None, 1, 0, P(B), 15, P(D + 1), None), E_ARG, "null pointer"),
        (lambda l: l.aeth_rs_decode(C.byref(RS), P(A), 15, None, 1, 0, P(A + 14), 15, P(D + 1), None), E_ALIGN, "rec_dev not 4-byte aligned"),
        (lambda l: l.aeth_rs_decode(C.byref(RS), P(A), 15, None, 1, 0, P(A + 14), 15, None, P(E + 4)), E_ALIGN, "summary_dev not 8-byte aligned"),
        (lambda l: l.aeth_rs_decode(C.byref(RS), P(A), 15 * (64 << 31), None, 1, 0, P(A - 1), 15 * (64 << 31), None, None), E_ARG, "an output overlaps an input")),
    "rs_encode": (
        (lambda l: l.aeth_rs_encode(C.byref(RS), None, 12, 1, P(B), 15), E_LEN, "ndata 12 is no multiple of the frame of 11 bytes"),
        (lambda l: l.aeth_rs_encode(C.byref(RS), P(A), 11 * (64 << 31), 1, P(A - 1), 15 * (64 << 31)), E_ARG, "the output overlaps the input")),
    "rs_host_decode": (
        (lambda l: l.aeth_rs_host_decode(C.byref(CODE), P(A), 16, None, 1, 2, P(B), 15, None, None), E_ARG, "unknown flag bits 0x2"),
        (lambda l: l.aeth_rs_host_decode(C.byref(CODE), None, 16, None, 1, 0, P(B), 15, None, None), E_LEN, "nin 16 is no multiple of the frame of 15 bytes"),
        (lambda l: l.aeth_rs_host_decode(C.byref(CODE), None, 15, P(B + 14), 1, 0, P(B), 15, None, None), E_ARG, "null pointer")),
    "rs_host_encode": (
        (lambda l: l.aeth_rs_host_encode(C.byref(CODE), None, 12, 1, P(B), 15), E_LEN, "ndata 12 is no multiple of the frame of 11 bytes"),),
    "cc_encode": (
        (lambda l: l.aeth_cc_encode(CC, None, None, 8, P(B), 17), E_LEN, "output holds 17 coded bits, 8 bits x 2 give 16"),
        (lambda l: l.aeth_cc_encode(CC, P(B + 1), None, 8, P(B), 16), E_ARG, "null pointer"),
        (lambda l: l.aeth_cc_encode(CC, None, P(A), 1 << 39, P(A - 1), 2 << 39), E_ARG, "the output overlaps an input")),
    "cc_decode": (
        (lambda l: l.aeth_cc_decode(CC, None, None, 17, P(B), 8), E_LEN, "input holds 17 soft values, 8 bits x 2 need 16"),
        (lambda l: l.aeth_cc_decode(CC, P(B + 1), None, 16, P(B), 8), E_ARG, "null pointer"),
        (lambda l: l.aeth_cc_decode(CC, None, P(A), 2 << 38, P(A - 1), 1 << 38), E_ARG, "the output overlaps an input")),
    "remap_exec": (
        (lambda l: l.aeth_remap_exec(C.byref(REMAP), P(A), G32, None, 4, 0), E_UNSUPPORTED, f"n_in {G32}: 2^32 or more in one call (cut the stream at a period)"),
        (lambda l: l.aeth_remap_exec(C.byref(REMAP), P(A), 3, None, 4, 0), E_LEN, "input holds 3 bytes, 4 outputs read 4")),
    "crc_exec": (
        (lambda l: l.aeth_crc_exec(C.byref(CRC), P(A), G32, 1, None, None), E_UNSUPPORTED,
         f"1 frames of {G32} bits: the input reaches 2^32 bytes (cut the frames and carry the state)"),
        (lambda l: l.aeth_crc_exec(C.byref(CRC), None, 8, 1, P(B + 4), P(D)), E_ARG, "null pointer"),
        (lambda l: l.aeth_crc_exec(C.byref(CRC), P(D + 4), 8, 1, P(B + 4), P(D)), E_ALIGN, "state pointer not 8-byte aligned")),
    "crc_attach": (
        (lambda l: l.aeth_crc_attach(C.byref(CRC), P(A), G32 - 16, 1, None), E_UNSUPPORTED, f"1 frames of {G32 - 16} + 16 bits: the output reaches 2^32 bytes"),),
    "crc_check": (
        (lambda l: l.aeth_crc_check(C.byref(CRC), P(A), 8, 1, 0x10000, None, None, None), E_ARG, "mask 0x10000 at or above 2^16"),
        (lambda l: l.aeth_crc_check(C.byref(CRC), None, G32 - 16, 1, 0, None, None, None), E_ARG, "diff_dev, payload_dev and summary_dev are all null"),
        (lambda l: l.aeth_crc_check(C.byref(CRC), None, G32 - 16, 1, 0, P(B), None, None), E_UNSUPPORTED, f"1 frames of {G32 - 16} + 16 bits: the input reaches 2^32 bytes"),
        (lambda l: l.aeth_crc_check(C.byref(CRC), None, 8, 1, 0, P(B + 4), None, None), E_ARG, "in_dev is null"),
        (lambda l: l.aeth_crc_check(C.byref(CRC), P(A), 8, 1, 0, P(B + 4), P(A + 23), None), E_ALIGN, "diff_dev or summary_dev not 8-byte aligned")),
    "bits_pack": (
        (lambda l: l.aeth_bits_pack(CTX, P(A), 64, 2, P(B), 7), E_ARG, "unknown bit order 2"),
        (lambda l: l.aeth_bits_pack(CTX, None, 64, 0, P(B), 7), E_LEN, "64 bits pack into 8 bytes, not 7"),
        (lambda l: l.aeth_bits_pack(CTX, None, G32, 0, P(B), G32 // 8), E_UNSUPPORTED, f"nbits {G32}: 2^32 or more in one call (cut at a multiple of 8)")),
    "bits_unpack": (
        (lambda l: l.aeth_bits_unpack(CTX, P(A), 8, 2, P(B), 65), E_ARG, "unknown bit order 2"),
        (lambda l: l.aeth_bits_unpack(CTX, None, 8, 0, P(B), 65), E_LEN, "65 bits need 9 bytes, the input holds 8"),
        (lambda l: l.aeth_bits_unpack(CTX, None, G32 // 8, 0, P(B), G32), E_UNSUPPORTED, f"nbits {G32}: 2^32 or more in one call (cut at a multiple of 8)")),
}


@pytest.mark.parametrize("row", ROWS, ids=[r.name for r in ROWS])
def test_the_earlier_check_answers(lib, row):
    for call, code, text in ORDER[row.name]:
        refused(lib, call(lib), code, text)


def test_codeword_lengths_of_ldpc_and_polar(lib):
    p, q = C.byref(POLAR), C.byref(LDPC)
    refused(lib, lib.aeth_polar_encode(p, P(A), 11, P(B), 32), E_LEN, "nbits 11 is no multiple of K = 12")
    refused(lib, lib.aeth_polar_encode(p, P(A), 12, P(B), 31), E_LEN, "1 codewords of N = 32 are 32 coded bits, not 31")
    refused(lib, lib.aeth_polar_encode(p, P(A), 24, P(B), 32), E_LEN, "2 codewords of N = 32 are 64 coded bits, not 32")
    refused(lib, lib.aeth_polar_encode(p, P(A), 12 << 59, P(B), 32), E_LEN, f"{1 << 59} codewords of N = 32 are {(1 << 64) - 1} coded bits, not 32")
    refused(lib, lib.aeth_polar_decode(p, P(A), 33, None, 0, P(B), 12, None), E_LEN, "nsoft 33 is no multiple of N = 32")
    refused(lib, lib.aeth_polar_decode(p, P(A), 32, None, 0, P(B), 32, None), E_LEN, "1 codewords give 12 bits (12 each), not 32")
    refused(lib, lib.aeth_polar_decode(p, P(A), 64, None, 1, P(B), 24, None), E_LEN, "2 codewords give 64 bits (32 each), not 24")
    refused(lib, lib.aeth_ldpc_encode(q, P(A), 16, P(B), 30), E_LEN, "nbits 16 is no multiple of K = 15")
    refused(lib, lib.aeth_ldpc_encode(q, P(A), 15, P(B), 29), E_LEN, "1 codewords of N = 30 are 30 coded bits, not 29")
    refused(lib, lib.aeth_ldpc_encode(q, P(A), 30, P(B), 30), E_LEN, "2 codewords of N = 30 are 60 coded bits, not 30")
    refused(lib, lib.aeth_ldpc_decode(q, P(A), 29, 10, 0, P(B), 30, None), E_LEN, "nsoft 29 is no multiple of N = 30")
    refused(lib, lib.aeth_ldpc_decode(q, P(A), 30, 10, 0, P(B), 15, None), E_LEN, "1 codewords give 30 bits (30 each), not 15")
    refused(lib, lib.aeth_ldpc_decode(q, P(A), 60, 10, 2, P(B), 60, None), E_LEN, "2 codewords give 30 bits (15 each), not 60")
