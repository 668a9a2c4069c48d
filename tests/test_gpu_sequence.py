"""GPU: the device LFSR sequences (csrc/aeth_sequence.hip) -- bits, scramble, chips, spread -- byte for byte against a
restatement of sequence::generate (reference: src/sequence.rs:47-53; tests/seq_truth.py).  Nothing compares against a
tolerance.

Launch geometry: a workgroup is 256 lanes = 4 waves; a wave owns C = seq.chunk = 16384 consecutive positions, made in
4 rounds of 4096 (64 lanes x one 64-bit word); a workgroup covers 4 C = 65536.  The largest length, 40 C + 4097 + 5 =
659462, is 41 chunks = 11 workgroups; the last workgroup runs one wave, whose second round holds 6 positions.  Pointers
that are not 16-byte aligned move up to 15 bytes (one cf32) in front of that grid."""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

import seq_truth
from aether_primitives_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = json.load(open(os.path.join(ROOT, "tests", "golden", "sequence_kat.json")))
CH = 16384                                         # asserted against seq.chunk below
NMAX = 40 * CH + 4097 + 5
LENGTHS = (1, 63, 64, 65, 4095, 4097, CH - 1, CH, CH + 1, NMAX)
FAR = 2 ** 40 + 12345
X1, X2 = (28, 31), (28, 29, 30, 31)
P31 = 2 ** 31 - 1

# name -> (registers, init words)
SETS = {
    "d1": (((1,),), (1,)),
    "fib": (((1, 2),), (0b01,)),
    "m7": (((6, 7),), (0x7f,)),
    "x1": ((X1,), (1,)),
    "gold": ((X1, X2), (1, 0x12345)),
    "o64": (((60, 61, 63, 64),), (0x0123456789abcdef,)),
    "four": (((3, 5), (6, 7), X2, (60, 61, 63, 64)), (0b10110, 0x55, 0x7fffffff, 0xfedcba9876543210)),
    "zero": ((X1,), (0,)),
}


def skips_of(name):
    order = max(max(r) for r in SETS[name][0])
    return sorted({0, 1, order - 1, order, 63, 64, 1600, FAR})


@functools.lru_cache(maxsize=None)
def truth(name, skip, n=NMAX + 256):
    """c[skip .. skip + n) as bytes of 0 / 1; computed once per (set, skip) and never written to"""
    regs, inits = SETS[name]
    if name == "m7":                                               # any skip: tile the 127-chip period
        period = seq_truth.m_sequence_bits()
        t = np.tile(period, n // 127 + 3)[skip % 127:][:n]
    elif name == "x1" and skip > (1 << 21):                        # beyond reach: the period of x1 is 2^31 - 1
        t = seq_truth.truth(regs, inits, skip % P31, n)
    else:
        t = seq_truth.truth(regs, inits, skip, n)
    t = np.ascontiguousarray(t)
    t.flags.writeable = False
    return t


@pytest.fixture(scope="module")
def seqs(ctx):
    import aether_primitives_amd as ap
    made = {name: ap.Sequence(ctx, *regs) for name, (regs, _) in SETS.items()}
    for s in made.values():
        assert s.chunk == CH
    assert -(-NMAX // (4 * CH)) >= 3 and NMAX % 4096 not in (0, 4095)      # three workgroups and more, ragged tail
    yield made
    made.clear()


class Raw:
    """a byte buffer in HBM with room for guards and byte offsets"""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        self.ptr = ctx.alloc(nbytes)

    def put(self, a):
        self.ctx.upload(self.ptr, np.ascontiguousarray(a))

    def get(self, nbytes=None, dtype=np.uint8):
        out = np.empty(self.nbytes if nbytes is None else nbytes, np.uint8)
        self.ctx.download(self.ptr, out)
        return out.view(dtype)

    def __del__(self):
        try:
            if self.ptr and self.ctx.h:
                self.ctx.free(self.ptr); self.ptr = None
        except Exception:
            pass


def _bits_at(seq, init, skip, ptr, n):
    _lib.check(seq._lib.aeth_seq_bits(seq.h, seq._init(init), skip, C.c_void_p(ptr), n))


GUARD = 32


@pytest.mark.parametrize("name", sorted(SETS))
def test_bits_every_length_skip_and_alignment(ctx, seqs, name):
    seq, init = seqs[name], SETS[name][1]
    buf = Raw(ctx, NMAX + 2 * GUARD + 16)
    fill = np.full(buf.nbytes, 0xAA, np.uint8)
    offs = (0, 1, 3, 5)
    k = 0
    for skip in skips_of(name):
        t = truth(name, skip)
        for n in LENGTHS:
            off = offs[k % 4]; k += 1
            buf.put(fill[:n + 2 * GUARD + 16])
            _bits_at(seq, init, skip, buf.ptr + GUARD + off, n)
            got = buf.get(n + 2 * GUARD + 16)
            body = got[GUARD + off:GUARD + off + n]
            assert (body == t[:n]).all(), (name, skip, n, off, int(np.argmax(body != t[:n])))
            assert (got[:GUARD + off] == 0xAA).all() and (got[GUARD + off + n:] == 0xAA).all(), (name, skip, n, off)
    if name == "zero":
        assert not truth(name, 1600).any()


@pytest.mark.parametrize("name", ["gold", "o64", "four", "m7"])
def test_bits_in_one_call_equal_bits_in_pieces(ctx, seqs, name):
    seq, init = seqs[name], SETS[name][1]
    n, skip = 2 * CH + 4097 + 5, 1600
    rng = np.random.default_rng(815)
    buf = Raw(ctx, n + 16)
    _bits_at(seq, init, skip, buf.ptr, n)
    whole = buf.get(n)
    assert (whole == truth(name, skip)[:n]).all()
    for cut in (1, 4096, CH, CH + 7, int(rng.integers(2, n - 1))):
        buf.put(np.full(n, 0xAA, np.uint8))
        _bits_at(seq, init, skip, buf.ptr, cut)
        _bits_at(seq, init, skip + cut, buf.ptr + cut, n - cut)
        assert (buf.get(n) == whole).all(), (name, cut)


@pytest.mark.parametrize("name", sorted(SETS))
def test_scramble(ctx, seqs, name):
    seq, init = seqs[name], SETS[name][1]
    lib = seq._lib
    rng = np.random.default_rng(816)
    data = rng.integers(0, 256, NMAX + 64, dtype=np.uint8)           # bytes other than 0 / 1: only bit 0 counts
    src, dst = Raw(ctx, NMAX + 64), Raw(ctx, NMAX + 64)
    src.put(data)
    sk = skips_of(name)
    for n, skip, ioff, ooff in ((65, sk[0], 0, 0), (4097, sk[2], 3, 0), (CH + 1, 64, 0, 5), (CH - 1, sk[3], 7, 7),
                                (NMAX, FAR, 1, 3), (NMAX, 1, 16, 0)):
        t = truth(name, skip)[:n]
        want = (data[ioff:ioff + n] & 1) ^ t
        dst.put(np.full(dst.nbytes, 0xAA, np.uint8))
        _lib.check(lib.aeth_seq_scramble(seq.h, seq._init(init), skip, C.c_void_p(src.ptr + ioff), C.c_void_p(dst.ptr + 16 + ooff), n))
        got = dst.get()
        assert (got[16 + ooff:16 + ooff + n] == want).all(), (name, n, skip, ioff, ooff)
        assert (got[:16 + ooff] == 0xAA).all() and (got[16 + ooff + n:] == 0xAA).all()
        assert (src.get(NMAX + 64) == data).all()
        # in place, then once more: in & 1 comes back
        p = C.c_void_p(dst.ptr + ooff)
        dst.put(data)
        _lib.check(lib.aeth_seq_scramble(seq.h, seq._init(init), skip, p, p, n))
        got = dst.get()
        assert (got[ooff:ooff + n] == (data[ooff:ooff + n] & 1) ^ t).all(), (name, n, skip, ooff)
        assert (got[:ooff] == data[:ooff]).all() and (got[ooff + n:] == data[ooff + n:]).all()
        _lib.check(lib.aeth_seq_scramble(seq.h, seq._init(init), skip, p, p, n))
        assert (dst.get()[ooff:ooff + n] == data[ooff:ooff + n] & 1).all()
    # the mirror: DeviceBits in and out
    out = seq.scramble(init, data[:1000], skip=5)
    assert (out.to_host() == (data[:1000] & 1) ^ truth(name, 5)[:1000]).all()


MAPPINGS = (((1 + 1j), (-1 - 1j)), ((1 + 0j), (-1 + 0j)))           # the reference's BPSK table; real +-1 chips


@pytest.mark.parametrize("name", sorted(SETS))
def test_chips(ctx, seqs, name):
    seq, init = seqs[name], SETS[name][1]
    sk = skips_of(name)
    vec = ctx.empty(NMAX + 4)
    guard = np.full(NMAX + 4, np.complex64(complex(123.0, -456.0)))
    k = 0
    for n in (1, 2, 63, 4097, CH + 1, NMAX):
        for skip in (sk[0], sk[3], FAR):
            zero, one = MAPPINGS[k % 2]
            first = (k // 2) % 2 + 1                                 # 1: 8- but not 16-byte aligned; 2: 16-byte aligned
            k += 1
            ctx.upload(vec.ptr, guard)
            seq.chips(init, n, skip=skip, zero=zero, one=one, out=vec.slice(first, first + n))
            got = vec.to_host()
            want = np.where(truth(name, skip)[:n] != 0, np.complex64(one), np.complex64(zero)).astype(np.complex64)
            assert (got[first:first + n].view(np.uint32) == want.view(np.uint32)).all(), (name, n, skip, first)
            assert (got[:first] == guard[:first]).all() and (got[first + n:] == guard[first + n:]).all()
    # values are copied bit for bit: a NaN payload and a negative zero
    z = _lib.Cf32.from_buffer_copy(np.array([0x7fc12345, 0x80000000], np.uint32).tobytes())
    o = _lib.Cf32.from_buffer_copy(np.array([0xffc00001, 0x00000001], np.uint32).tobytes())
    _lib.check(seq._lib.aeth_seq_chips(seq.h, seq._init(init), 1600, z, o, vec._p(), 1000))
    got = vec.to_host()[:1000].view(np.uint32).reshape(-1, 2)
    t = truth(name, 1600)[:1000]
    want = np.where(t[:, None] != 0, np.array([0xffc00001, 0x00000001], np.uint32), np.array([0x7fc12345, 0x80000000], np.uint32))
    assert (got == want).all()


def _symbols(n, seed):
    rng = np.random.default_rng(seed)
    s = (rng.standard_normal(n) + 1j * rng.standard_normal(n)).astype(np.complex64)
    u = s.view(np.uint32)
    u[0], u[1] = 0x80000000, 0x00000000                               # (-0.0, +0.0)
    if n > 2:
        u[4], u[5] = 0x7fc12345, 0xffc00001                           # NaNs with payloads
    return s


def _spread_truth(sym, sf, t):
    u = np.repeat(sym.view(np.uint32).reshape(-1, 2), sf, axis=0)
    return u ^ (t[:u.shape[0], None].astype(np.uint32) << 31)


@pytest.mark.parametrize("sf", [1, 3, 64, 127])
@pytest.mark.parametrize("name", ["m7", "gold", "four"])
def test_spread(ctx, seqs, name, sf):
    seq, init = seqs[name], SETS[name][1]
    sk = skips_of(name)
    for nsym, skip, first in ((1, sk[0], 0), (-(-(CH + 1) // sf), sk[3], 1), (-(-NMAX // sf), FAR, 0), (-(-NMAX // sf) + 1, 64, 1)):
        sym = _symbols(nsym, 817 + nsym % 7)
        n = nsym * sf
        d_sym = ctx.vec(sym)
        vec = ctx.empty(n + 3)
        guard = np.full(n + 3, np.complex64(complex(123.0, -456.0)))
        ctx.upload(vec.ptr, guard)
        out = vec.slice(first, first + n)
        seq.spread(init, d_sym, sf, skip=skip, out=out)
        t = truth(name, skip)
        got = vec.to_host()
        want = _spread_truth(sym, sf, t)
        assert (got[first:first + n].view(np.uint32).reshape(-1, 2) == want).all(), (name, sf, nsym, skip, first)
        assert (got[:first] == guard[:first]).all() and (got[first + n:] == guard[first + n:]).all()
        assert (d_sym.to_host().view(np.uint32) == sym.view(np.uint32)).all()
        # spread again over the result (sf = 1, in place): the repeated symbols come back bit for bit
        seq.spread(init, out, 1, skip=skip, out=out)
        again = vec.to_host()[first:first + n].view(np.uint32).reshape(-1, 2)
        assert (again == np.repeat(sym.view(np.uint32).reshape(-1, 2), sf, axis=0)).all(), (name, sf, nsym, skip, first)
        if sf == 1:                                                    # in place at sf = 1, from the symbols themselves
            seq.spread(init, d_sym, 1, skip=skip, out=d_sym)
            assert (d_sym.to_host().view(np.uint32).reshape(-1, 2) == want).all()


def test_spread_refuses_a_wrong_length(ctx, seqs):
    seq = seqs["m7"]
    with pytest.raises(_lib.LengthMismatch):
        seq.spread(0x7f, ctx.vec(np.ones(4, np.complex64)), 127, out=ctx.empty(4 * 127 - 1))


@pytest.mark.parametrize("name", ["x1", "gold", "four"])
def test_host_bits_equal_device_bits(ctx, seqs, name):
    seq, init = seqs[name], SETS[name][1]
    for n, skip in ((1, 0), (4097, 1600), (CH + 1, FAR), (NMAX, 63)):       # below and above the pinned-bounce size
        host = seq.bits(init, n, skip=skip, host=True)
        dev = seq.bits(init, n, skip=skip).to_host()
        assert (host == dev).all() and (host == truth(name, skip)[:n]).all(), (name, n, skip)
    assert seq.bits(init, 0, host=True).size == 0 and seq.bits(init, 0).n == 0


def test_overlap_lane_gives_the_same_bytes(seqs):
    import aether_primitives_amd as ap
    ctx2 = ap.Context(0)
    try:
        ctx2.set_overlap(True)
        name = "gold"
        regs, init = SETS[name]
        seq = ap.Sequence(ctx2, *regs)
        n, skip = 4 * CH + 4097 + 5, 1600
        t = truth(name, skip)[:n]
        sym = _symbols(n, 818)
        d_sym = ctx2.vec(sym)
        for rep in range(3):
            b = seq.bits(init, n, skip=skip)
            s = seq.scramble(init, b, skip=skip)
            c = seq.chips(init, n, skip=skip)
            p = seq.spread(init, d_sym, 1, skip=skip)
            assert (b.to_host() == t).all() and not s.to_host().any()
            assert (c.to_host() == np.where(t != 0, np.complex64(-1 - 1j), np.complex64(1 + 1j))).all()
            assert (p.to_host().view(np.uint32).reshape(-1, 2) == _spread_truth(sym, 1, t)).all()
        del seq
    finally:
        ctx2.close()


def test_generate_mirror_in_the_shape_of_the_reference(ctx):
    from aether_primitives_amd import sequence
    assert list(sequence.generate([1, 0], (1, 2), 6, ctx=ctx)) == [1, 0, 1, 1, 0, 1]              # sequence.rs:61-68
    assert list(sequence.generate([1, 0, 1], (1, 2), 2, ctx=ctx)) == [1, 0, 1]                    # len <= init.len()
    assert list(sequence.generate([1, 0, 1], (1, 2), 3, ctx=ctx)) == [1, 0, 1]
    x1 = sequence.generate(sequence.expand(1, 31), X1, 1600 + 5000, ctx=ctx)                      # the doc example, :42-46
    assert (x1 == seq_truth.plain(X1, 1, 6600)).all()
    init = [1, 1, 0, 1, 0, 0, 1, 0, 1]                                                            # longer than the order
    assert (sequence.generate(init, (2, 5), 5000, ctx=ctx) == sequence.generate(init, (2, 5), 5000)).all()


def test_lte_gold(ctx):
    import aether_primitives_amd as ap
    gold = ap.lte_gold(ctx)
    for c_init, want in KAT["lte"]["c"].items():
        c = gold.c(int(c_init, 16), 64).to_host()
        assert sum(int(b) << i for i, b in enumerate(c)) == int(want, 16), c_init
        assert gold.seq.window((1, int(c_init, 16)), 1600) == int(want, 16)
    assert (gold.c(0x12345, 5000, host=True) == truth("gold", 1600)[:5000]).all()
