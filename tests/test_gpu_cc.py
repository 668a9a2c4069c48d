"""GPU: the convolutional-code kernels and the soft demodulator against the numpy restatement (tests/cc_truth.py), byte
for byte: every decode shape under five kinds of input, with and without history, with the soft pointer at byte offsets
0 .. 3 and the output at offsets 0 and 1 between guard bytes; streams cut at a multiple of D; the encoder; the soft
demodulator on four tables with NaN, infinities, -0.0 and saturating values; and the refusals, which launch nothing."""
import ctypes as C

import numpy as np
import pytest

import aether_primitives_amd as ap
import cc_truth
from aether_primitives_amd import _lib
from cc_truth import SMALL_SHAPES

pytestmark = pytest.mark.gpu

K7 = (0o171, 0o133)
# (k, polys, D, A, T, N)
SHAPES = tuple(s + (5 * s[2] + 3,) for s in SMALL_SHAPES) + (
    (7, K7, 33, 31, 30, 33 * 70 + 1),            # D + T is not a multiple of 32
    (7, K7, 512, 64, 64, 512 * 130 + 17),
    (7, K7, 4000, 96, 96, 8001),                 # the limit D + T = 4096
    (3, (0o7, 0o5), 8, 3, 5, 8 * 16 * 3 + 5),    # full and partly filled waves of 16 blocks
)
KINDS = ("ties", "uniform", "max", "min", "noisy")
GUARD = 16


def make_soft(kind, k, polys, steps, seed):
    """`steps` trellis steps of soft values"""
    rng = np.random.default_rng(seed)
    n = len(polys)
    if kind == "ties":
        return rng.integers(-1, 2, steps * n).astype(np.int8)
    if kind == "uniform":
        return rng.integers(-128, 128, steps * n).astype(np.int8)
    if kind == "max":
        return np.full(steps * n, 127, np.int8)
    if kind == "min":
        return np.full(steps * n, -128, np.int8)
    coded = cc_truth.encode(k, polys, rng.integers(0, 2, steps).astype(np.uint8))
    return np.clip(np.rint((1.0 - 2.0 * coded) * 40.0 + rng.normal(0.0, 30.0, coded.size)), -128, 127).astype(np.int8)


class Buf:
    """`n` device bytes at byte offset `off` of an allocation, between guard bytes"""

    def __init__(self, ctx, n, off=0, host=None):
        self.ctx, self.n, self.off = ctx, n, off
        self.base = ctx.alloc(n + 2 * GUARD + 8)
        self.ptr = self.base + GUARD + off
        self.image = np.full(n + 2 * GUARD + 8, 0xA5, np.uint8)
        if host is not None:
            self.image[GUARD + off:GUARD + off + n] = np.ascontiguousarray(host).view(np.uint8)
        ctx.upload(self.base, self.image)

    def read(self):
        """the n bytes; the bytes around them must be as uploaded"""
        got = np.empty_like(self.image)
        self.ctx.download(self.base, got)
        lo, hi = GUARD + self.off, GUARD + self.off + self.n
        assert (got[:lo] == 0xA5).all() and (got[hi:] == 0xA5).all(), "guard bytes were written"
        return got[lo:hi]

    def __del__(self):
        try:
            self.ctx.free(self.base)
        except Exception:
            pass


def raw_decode(ctx, cc, soft, hist, soff, ooff):
    s = Buf(ctx, soft.size, soff, soft)
    h = Buf(ctx, hist.size, (soff + 1) % 4, hist) if hist is not None else None
    o = Buf(ctx, soft.size // cc.n, ooff)
    _lib.check(_lib.load().aeth_cc_decode(cc.h, C.c_void_p(h.ptr if h else None), C.c_void_p(s.ptr), soft.size, C.c_void_p(o.ptr), o.n))
    return o.read()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k,polys,D,A,T,N", SHAPES)
def test_decode_is_the_truth_byte_for_byte(ctx, k, polys, D, A, T, N, kind):
    n = len(polys)
    cc = ap.ConvCode(ctx, k, polys, D, A, T)
    assert (cc.block, cc.warmup, cc.traceback, cc.history) == (D, A, T, A + T)
    ext = make_soft(kind, k, polys, A + T + N, 1000 * k + D)
    soft = ext[(A + T) * n:]
    for hist in (None, ext[:(A + T) * n]):
        want = cc_truth.decode(k, polys, D, A, T, soft, hist)
        for soff in range(4):
            for ooff in (0, 1):
                got = raw_decode(ctx, cc, soft, hist, soff, ooff)
                assert (got == want).all(), (hist is not None, soff, ooff, int(np.flatnonzero(got != want)[0]))


@pytest.mark.parametrize("k,polys,D,A,T,N", SHAPES)
def test_two_calls_cut_at_a_block_boundary_equal_one_call_and_runs_repeat(ctx, k, polys, D, A, T, N):
    n = len(polys)
    cc = ap.ConvCode(ctx, k, polys, D, A, T)
    ext = make_soft("noisy", k, polys, A + T + N, 77)
    hist, soft = ext[:(A + T) * n], ext[(A + T) * n:]
    whole = cc.decode(soft, hist).to_host()
    assert (whole == cc_truth.decode(k, polys, D, A, T, soft, hist)).all()
    assert (cc.decode(soft, hist).to_host() == whole).all()         # the same bytes run to run
    cut = D * max(1, (N // D) // 2)
    first = cc.decode(soft[:cut * n], hist).to_host()
    second = cc.decode(soft[cut * n:], ext[cut * n:(cut + A + T) * n]).to_host()
    assert (np.concatenate([first, second]) == whole).all()


@pytest.mark.parametrize("k,polys,D,A,T", SMALL_SHAPES)
def test_decode_stream_recovers_a_noise_free_codeword(ctx, k, polys, D, A, T):
    cc = ap.ConvCode(ctx, k, polys, D, A, T)
    bits = np.random.default_rng(3).integers(0, 2, 5 * D + 3).astype(np.uint8)
    coded = cc.encode(bits).to_host()
    soft = (1 - 2 * coded.astype(np.int8)).astype(np.int8)
    got = cc.decode_stream(soft).to_host()
    assert (got == cc_truth.decode_stream(k, polys, D, A, T, soft)).all() and (got == bits).all()


@pytest.mark.parametrize("N", (1, 7, 64, 65, 4099))
@pytest.mark.parametrize("k,polys", ((7, K7), (7, (0o133, 0o171, 0o165)), (4, (0o15, 0o17, 0o13, 0o11)), (3, (0o7, 0o5))))
def test_encoder_bit_for_bit(ctx, k, polys, N):
    rng = np.random.default_rng(N + k)
    cc = ap.ConvCode(ctx, k, polys)
    bits = rng.integers(0, 256, N).astype(np.uint8)                  # input bytes > 1 are taken & 1
    hist = rng.integers(0, 256, k - 1).astype(np.uint8)
    assert (cc.encode(bits).to_host() == cc_truth.encode(k, polys, bits)).all()
    whole = cc.encode(bits, hist).to_host()
    assert (whole == cc_truth.encode(k, polys, bits, hist)).all()
    # through raw pointers at odd offsets, between guard bytes
    b, h, o = Buf(ctx, N, 3, bits), Buf(ctx, k - 1, 1, hist), Buf(ctx, N * len(polys), 1)
    _lib.check(_lib.load().aeth_cc_encode(cc.h, C.c_void_p(h.ptr), C.c_void_p(b.ptr), N, C.c_void_p(o.ptr), o.n))
    assert (o.read() == whole).all()
    if N > k:                                                        # chunks of a stream concatenate
        cut = N // 2
        ext = np.concatenate([hist, bits])
        two = np.concatenate([cc.encode(bits[:cut], hist).to_host(), cc.encode(bits[cut:], ext[cut:cut + k - 1]).to_host()])
        assert (two == whole).all()


def tables():
    rng = np.random.default_rng(21)
    lv = np.array([-3, -1, 3, 1], np.float32)
    qam16 = np.array([complex(lv[i & 3], lv[i >> 2]) for i in range(16)], np.complex64) / np.float32(np.sqrt(10.0))
    t256 = (rng.normal(size=256) + 1j * rng.normal(size=256)).astype(np.complex64)
    return {"bpsk": ap.modulation.GENERIC_BPSK_TABLE, "qpsk": ap.modulation.GENERIC_QPSK_TABLE, "qam16": qam16, "t256": t256}


SPECIAL = np.array([complex(np.nan, 0.5), complex(0.5, np.nan), complex(np.inf, 0.25), complex(-np.inf, np.inf), complex(-0.0, 0.0),
                    complex(0.0, -0.0), 1e20 + 1e20j, -1e20 + 3j, 1e-30 - 1e-30j, 250.0 - 250.0j, 3e38 + 3e38j], np.complex64)


@pytest.mark.parametrize("nsym", (1, 63, 4097))
@pytest.mark.parametrize("name", ("bpsk", "qpsk", "qam16", "t256"))
def test_soft_demodulator_bit_for_bit(ctx, name, nsym):
    table = tables()[name]
    m = ap.modulation.table(ctx, table)
    rng = np.random.default_rng(nsym)
    sym = (table[rng.integers(0, table.size, nsym)] + (rng.normal(size=nsym) + 1j * rng.normal(size=nsym)) * 0.4).astype(np.complex64)
    if nsym > SPECIAL.size:
        sym[rng.choice(nsym, SPECIAL.size, replace=False)] = SPECIAL
    else:
        sym[0] = SPECIAL[nsym % SPECIAL.size]
    for scale in (8.0, 0.37, 1e6, -3.0):
        got = m.demod_soft(ctx.vec(sym), scale).to_host()
        want = cc_truth.demod_soft(table, sym, scale)
        assert got.dtype == np.int8 and (got == want).all(), (scale, int(np.flatnonzero(got != want)[0]))
    # the output at an odd address between guard bytes (byte stores); QPSK with a NULL table: the generic table
    v, bps = ctx.vec(sym), m.BITS_PER_SYMBOL
    o = Buf(ctx, bps * nsym, 1)
    tab = None if name == "qpsk" else m.table.ctypes.data_as(C.c_void_p)
    _lib.check(_lib.load().aeth_demod_soft(ctx.h, v._p(), nsym, bps, tab, 8.0, C.c_void_p(o.ptr), o.n))
    assert (o.read().view(np.int8) == cc_truth.demod_soft(table, sym, 8.0)).all()


def _free_bytes():
    hip = _lib.load()                              # hipMemGetInfo of the runtime the library is bound to
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_refused_creates_leave_nothing_allocated(ctx):
    ctx.sync()
    free0 = _free_bytes()
    for _ in range(25):
        for args, code in (((8, K7), _lib.E_UNSUPPORTED), ((7, (0o171, 0o400)), _lib.E_ARG), ((7, K7, 4000, 64, 97), _lib.E_ARG),
                           ((7, K7, 512, 4097, 64), _lib.E_ARG)):
            with pytest.raises(ap.AetherError) as e:
                ap.ConvCode(ctx, *args)
            assert e.value.code == code
    ctx.sync()
    assert _free_bytes() == free0


def test_refused_calls_launch_nothing(ctx):
    lib = _lib.load()
    cc = ap.ConvCode(ctx, 7, K7, 64, 16, 24)
    soft = make_soft("noisy", 7, K7, 200, 5)
    s, o = Buf(ctx, soft.size, 0, soft), Buf(ctx, 400, 0)
    assert lib.aeth_cc_decode(cc.h, None, C.c_void_p(s.ptr), soft.size, C.c_void_p(o.ptr), 199) == _lib.E_LEN
    assert lib.aeth_cc_decode(cc.h, None, C.c_void_p(s.ptr), soft.size, C.c_void_p(s.ptr + 399), 200) == _lib.E_ARG
    assert lib.aeth_cc_decode(cc.h, C.c_void_p(o.ptr + 100), C.c_void_p(s.ptr), soft.size, C.c_void_p(o.ptr), 200) == _lib.E_ARG
    assert lib.aeth_cc_encode(cc.h, None, C.c_void_p(s.ptr), 200, C.c_void_p(o.ptr), 399) == _lib.E_LEN
    assert lib.aeth_cc_encode(cc.h, None, C.c_void_p(s.ptr), 200, C.c_void_p(s.ptr + 199), 400) == _lib.E_ARG
    v = ctx.vec(np.ones(50, np.complex64))
    assert lib.aeth_demod_soft(ctx.h, v._p(), 50, 2, None, 1.0, C.c_void_p(o.ptr), 99) == _lib.E_LEN
    ctx.sync()
    assert (o.read() == 0xA5).all() and (s.read().view(np.int8) == soft).all()
    with pytest.raises(ap.LengthMismatch):
        cc.decode(soft[:-1])
    with pytest.raises(ap.LengthMismatch):
        cc.decode(soft, soft[:10])
