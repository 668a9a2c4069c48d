"""GPU: aeth_crc_exec / attach / check (include/aether_hip.h) against the restatement tests/crc_truth.py, byte for byte;
attach and check outputs lie between guard bytes that are checked unchanged, and input bytes are drawn from 0 .. 255 so
that only the low bit may count.

  1. widths 1 .. 64 with random parameters and every named row x frame lengths around 8, 16, 64, 1024 (the lane chunk and
     the largest group's pass) x frame counts around 64 and around the frames per workgroup of the length.
  2. every output alignment x four input alignments at one mid-sized shape.
  3. the route boundary: route_frame_bits - 1, + 0, + 1.
  4. the long route: 2, 255, 256, 257 chunks (the combine launch's lanes take chunks 256 apart), three long frames, a last
     chunk of one bit and one a bit short of full.
  5. streaming: a frame of about 10^5 bits cut anywhere, the state carried on the device, random start states.
  6. check with planted errors, a mask, every subset of the three outputs.
  7. the same calls twice; a child process under AETH_TUNING=1 with both cache policies and with the long route forced
     (AETH_CRC_ROUTE=2, which also runs frames of one chunk there): the bytes of this process."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
if __name__ == "__main__":
    sys.path[:0] = [ROOT, HERE]

import aether_primitives_amd as ap                    # noqa: E402
from aether_primitives_amd import _lib, crc           # noqa: E402
import crc_truth as T                                 # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0xA5
LENGTHS = (0, 1, 7, 8, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025)
COUNTS = (1, 2, 63, 64, 65)


def params():
    rng = np.random.default_rng(2024)
    out = [(f"r{r}",) + T.random_params(rng, r) for r in T.WIDTHS]
    return out + [(n,) + T.NAMED[n][:4] for n in sorted(T.NAMED)]


PARAMS = params()
BY_NAME = {p[0]: p[1:] for p in PARAMS}


class Mem:
    """device buffers of one test: inputs at an offset behind an allocation's start, outputs between guards"""

    def __init__(self, ctx):
        self.ctx, self.held = ctx, []

    def inp(self, a, off=0):
        a = np.ascontiguousarray(a)
        base = self.ctx.alloc(off + a.nbytes + 16)
        self.held.append(base)
        if a.nbytes:
            self.ctx.upload(base + off, a.view(np.uint8))
        return base + off

    def out(self, n, off=0):
        base = self.ctx.alloc(GUARD + off + n + GUARD)
        self.held.append(base)
        self.ctx.upload(base, np.full(GUARD + off + n + GUARD, SENTINEL, np.uint8))
        return (base, n, off)

    @staticmethod
    def ptr(o):
        return C.c_void_p(o[0] + GUARD + o[2]) if o is not None else None

    def get(self, o, dtype=np.uint8):
        base, n, off = o
        got = np.empty(GUARD + off + n + GUARD, np.uint8)
        self.ctx.download(base, got)
        lo = GUARD + off
        assert (got[:lo] == SENTINEL).all(), "bytes in front of the output were written"
        assert (got[lo + n:] == SENTINEL).all(), "bytes behind the output were written"
        return got[lo:lo + n].copy().view(dtype)

    def free(self):
        for b in self.held:
            self.ctx.free(b)
        self.held = []


@pytest.fixture
def mem(ctx):
    m = Mem(ctx)
    yield m
    m.free()


def noisy(rng, bits):
    """the same low bits under random upper bits"""
    return (np.asarray(bits, np.uint8) & 1) | (rng.integers(0, 128, np.asarray(bits).size, dtype=np.uint8) << 1)


def d_exec(mem, c, bits, L, F, state=None, in_off=0):
    o = mem.out(8 * F, 8)
    st = C.c_void_p(mem.inp(np.asarray(state, np.uint64))) if state is not None else None
    _lib.check(c._lib.aeth_crc_exec(c.h, C.c_void_p(mem.inp(bits[:L * F], in_off)), L, F, st, mem.ptr(o)))
    return mem.get(o, np.uint64)


def d_attach(mem, c, bits, L, F, in_off=0, out_off=0):
    o = mem.out(F * (L + c.r), out_off)
    _lib.check(c._lib.aeth_crc_attach(c.h, C.c_void_p(mem.inp(bits[:L * F], in_off)), L, F, mem.ptr(o)))
    return mem.get(o)


def d_check(mem, c, frames, L, F, mask=0, want=(True, True, True), in_off=0, out_off=0):
    """-> (diff, payload, (n_bad, first_bad)), None where not asked for"""
    d = mem.out(8 * F, 8) if want[0] else None
    p = mem.out(F * L, out_off) if want[1] else None
    s = mem.out(16, 8) if want[2] else None
    _lib.check(c._lib.aeth_crc_check(c.h, C.c_void_p(mem.inp(frames[:F * (L + c.r)], in_off)), L, F, mask, mem.ptr(d), mem.ptr(p), mem.ptr(s)))
    return (mem.get(d, np.uint64) if d else None, mem.get(p) if p else None, tuple(int(v) for v in mem.get(s, np.uint64)) if s else None)


def all_three(mem, c, p, rng, L, counts, long_truth=False):
    """exec, attach and check of max(counts) random frames and of every smaller count, against the restatement"""
    r, poly, init, xorout = p
    Fm = max(counts)
    bits = rng.integers(0, 256, L * Fm, dtype=np.uint8)
    if long_truth:
        regs = np.array([T.register_long(r, poly, init, bits[f * L:(f + 1) * L]) for f in range(Fm)], np.uint64)
    else:
        regs = T.registers(r, poly, init, bits, L, Fm)
    att = np.empty((Fm, L + r), np.uint8)
    att[:, :L] = bits.reshape(Fm, L) & 1
    for j in range(r):
        att[:, L + j] = ((regs ^ np.uint64(xorout)) >> np.uint64(r - 1 - j)) & np.uint64(1)
    recv = noisy(rng, att.ravel()).reshape(Fm, L + r)
    flips = rng.integers(0, 3, Fm) == 0                               # about a third of the frames get one flipped bit
    pos = rng.integers(0, L + r, Fm)
    recv[flips, pos[flips]] ^= 1
    want_diff = np.zeros(Fm, np.uint64)
    for f in np.flatnonzero(flips):
        if pos[f] >= L:
            want_diff[f] = np.uint64(1) << np.uint64(r - 1 - (pos[f] - L))
        else:
            e = np.zeros(L, np.uint8); e[pos[f]] = 1
            want_diff[f] = T.register(r, poly, 0, e)                  # linear: the diff of an error is its register from 0
    for F in counts:
        tag = (p, L, F)
        assert d_exec(mem, c, bits, L, F).tolist() == regs[:F].tolist(), tag
        assert d_attach(mem, c, bits, L, F).tobytes() == att[:F].tobytes(), tag
        diff, pay, summ = d_check(mem, c, recv.ravel(), L, F)
        assert diff.tolist() == want_diff[:F].tolist(), tag
        assert pay.tobytes() == (recv[:F, :L] & 1).tobytes(), tag
        bad = np.flatnonzero(want_diff[:F])
        assert summ == (bad.size, int(bad[0]) if bad.size else F), tag
        mem.free()
    return regs


# ---- 1 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", PARAMS, ids=lambda p: p[0])
def test_widths_lengths_and_frame_counts(ctx, mem, p):
    c = ap.Crc(ctx, *p[1:])
    assert (c._lib.aeth_crc_width(c.h), c._lib.aeth_crc_poly(c.h), c._lib.aeth_crc_init(c.h), c._lib.aeth_crc_xorout(c.h)) == p[1:]
    assert c.residue == T.register(p[1], p[2], 0, T.check_bits(p[1], p[4]))
    rng = np.random.default_rng(p[1])
    for L in LENGTHS:
        assert c.route(L, 1) == crc.ROUTE_FRAMES
        fpw = c.frames_per_workgroup(L + p[1])
        assert fpw in (4, 8, 16, 32, 64)
        all_three(mem, c, p[1:], rng, L, sorted(set(COUNTS + (fpw - 1, fpw, fpw + 1))))
    c.close()


def test_the_diff_of_a_flipped_message_bit_is_its_register_from_zero():
    """the planted-error expectation above uses linearity; here it is checked against the restatement's own check()"""
    r, poly, init, xorout = BY_NAME["crc-24/lte-a"]
    rng = np.random.default_rng(1)
    bits = rng.integers(0, 2, 50, dtype=np.uint8)
    frame = T.attach(r, poly, init, xorout, bits, 50, 1)
    frame[17] ^= 1
    e = np.zeros(50, np.uint8); e[17] = 1
    assert int(T.check(r, poly, init, xorout, frame, 50, 1)[0][0]) == T.register(r, poly, 0, e)


# ---- 2 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_off", (0, 1, 3, 15))
def test_every_output_alignment(ctx, mem, in_off):
    r, poly, init, xorout = p = BY_NAME["crc-24/lte-a"]
    c = ap.Crc(ctx, *p)
    rng = np.random.default_rng(in_off)
    L, F = 333, 5
    bits = rng.integers(0, 256, L * F, dtype=np.uint8)
    att = T.attach(r, poly, init, xorout, bits, L, F)
    recv = noisy(rng, att)
    for out_off in range(16):
        assert d_attach(mem, c, bits, L, F, in_off, out_off).tobytes() == att.tobytes(), out_off
        diff, pay, summ = d_check(mem, c, recv, L, F, 0, (True, True, True), in_off, out_off)
        assert not diff.any() and summ == (0, F) and pay.tobytes() == (bits & 1).tobytes(), out_off
        mem.free()
    c.close()


# ---- 3, 4 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("crc-24/lte-a", "r64", "r1"))
def test_the_route_boundary(ctx, mem, name):
    c = ap.Crc(ctx, *BY_NAME[name])
    B = c.route_frame_bits
    assert B >= 1024 and (c.route(B, 1), c.route(B + 1, 1)) == (crc.ROUTE_FRAMES, crc.ROUTE_LONG)
    rng = np.random.default_rng(7)
    for L in (B - 1, B, B + 1):
        all_three(mem, c, BY_NAME[name], rng, L, (3,))
    c.close()


@pytest.mark.parametrize("name", ("crc-32", "r33"))
def test_long_frames_of_many_chunks(ctx, mem, name):
    """exec over 255, 256 and 257 chunks and over last chunks of one bit and of one bit short; crc-32 also against zlib"""
    import zlib
    p = BY_NAME[name]
    r, poly, init, xorout = p
    c = ap.Crc(ctx, *p)
    B = c.route_frame_bits
    rng = np.random.default_rng(8)
    data = rng.integers(0, 256, (257 * B + 8) // 8, dtype=np.uint8)
    bits = noisy(rng, np.unpackbits(data, bitorder="little"))
    for L in (254 * B + 1, 255 * B - 1, 255 * B, 256 * B, 256 * B + 1, 257 * B):
        want = T.register_long(r, poly, init, bits[:L])
        assert int(d_exec(mem, c, bits, L, 1, in_off=3)[0]) == want, L
        if name == "crc-32" and L % 8 == 0:
            assert T.pack(T.check_bits(r, want ^ xorout), True).tobytes() == zlib.crc32(data[:L // 8].tobytes()).to_bytes(4, "little")
        mem.free()
    c.close()


@pytest.mark.parametrize("name", ("crc-16/genibus", "r63"))
def test_three_long_frames_through_attach_and_check(ctx, mem, name):
    c = ap.Crc(ctx, *BY_NAME[name])
    B = c.route_frame_bits
    rng = np.random.default_rng(9)
    for L in (2 * B + 1, 3 * B - 1, 4 * B + 5 * 16 + 3):
        assert c.route(L, 3) == crc.ROUTE_LONG
        all_three(mem, c, BY_NAME[name], rng, L, (1, 3), long_truth=True)
    c.close()


# ---- 5 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("crc-24/lte-b", "r64"))
def test_a_frame_cut_anywhere_with_the_state_carried_on_the_device(ctx, mem, name):
    p = BY_NAME[name]
    r, poly, init, xorout = p
    c = ap.Crc(ctx, *p)
    B = c.route_frame_bits
    rng = np.random.default_rng(10)
    L, F = 100003, 2
    bits = rng.integers(0, 256, L * F, dtype=np.uint8)
    state = rng.integers(0, 1 << 63, F, dtype=np.uint64) & np.uint64((1 << r) - 1)
    want = [T.register_long(r, poly, int(state[f]), bits[f * L:(f + 1) * L]) for f in range(F)]
    assert d_exec(mem, c, bits, L, F, state).tolist() == want
    assert d_exec(mem, c, bits, L, F).tolist() == [T.register_long(r, poly, init, bits[f * L:(f + 1) * L]) for f in range(F)]
    two = bits.reshape(F, L)
    for cut in (0, 1, 63, B - 1, B, B + 1, 5 * B, L - 1, L):
        a, b = np.ascontiguousarray(two[:, :cut]).ravel(), np.ascontiguousarray(two[:, cut:]).ravel()
        s_in = ap.DeviceU64(ctx, F, state)
        dev = lambda x: ap.DeviceBits(ctx, x.size, x if x.size else None)
        mid = c.registers(dev(a), cut, F, state=s_in)
        end = c.registers(dev(b), L - cut, F, state=mid)
        assert end.to_host().tolist() == want, cut
    mem.free()
    c.close()


# ---- 6 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("crc-16/xmodem", "crc-24/lte-a", "r64", "r3"))
def test_check_with_planted_errors(ctx, mem, name):
    p = BY_NAME[name]
    r, poly, init, xorout = p
    c = ap.Crc(ctx, *p)
    rng = np.random.default_rng(12)
    L, F = 54, 1000
    bits = rng.integers(0, 256, L * F, dtype=np.uint8)
    good = noisy(rng, T.attach(r, poly, init, xorout, bits, L, F)).reshape(F, L + r)

    def run(frames, want=(True, True, True), mask=0):
        got = d_check(mem, c, frames.ravel(), L, F, mask, want)
        ref = T.check(r, poly, init, xorout, frames, L, F, mask)
        if want[0]:
            assert got[0].tolist() == ref[0].tolist()
        if want[1]:
            assert got[1].tobytes() == ref[1].tobytes()
            assert frames is not good or got[1].tobytes() == (bits & 1).tobytes()
        if want[2]:
            assert got[2] == ref[2]
        mem.free()
        return got, ref

    got, ref = run(good)
    assert ref[2] == (0, F) and not ref[0].any()
    for f, pos in ((0, 0), (F - 1, 0), (500, L - 1), (7, 0)) + tuple((100 + j, L + j) for j in range(r)):
        bad = good.copy()
        bad[f, pos] ^= 1
        got, ref = run(bad)
        assert ref[2] == (1, f) and int(ref[0][f]) != 0
        if pos >= L:
            assert int(got[0][f]) == 1 << (r - 1 - (pos - L))
    chosen = (3, 64, 65, 511, 998, 999)
    bad = good.copy()
    for f in chosen:
        bad[f, int(rng.integers(0, L + r))] ^= 1
    got, ref = run(bad)
    assert ref[2] == (len(chosen), 3) and np.flatnonzero(got[0]).tolist() == list(chosen)
    for want in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (True, False, True), (False, True, True)):
        run(bad, want)
    # an RNTI-style mask: attached with xorout ^ rnti, good under mask = rnti, the rnti itself under mask = 0
    rnti = int(rng.integers(1, 1 << min(r, 16))) & ((1 << r) - 1) or 1
    masked = noisy(rng, T.attach(r, poly, init, xorout ^ rnti, bits, L, F)).reshape(F, L + r)
    got, ref = run(masked, mask=rnti)
    assert got[2] == (0, F) and not got[0].any()
    got, ref = run(masked, mask=0)
    assert (got[0] == np.uint64(rnti)).all() and got[2] == (F, 0)
    # F = 0: nothing but the summary {0, 0}
    s = mem.out(16, 8)
    _lib.check(c._lib.aeth_crc_check(c.h, None, L, 0, 0, None, None, mem.ptr(s)))
    assert mem.get(s, np.uint64).tolist() == [0, 0]
    c.close()


# ---- 7 -----------------------------------------------------------------------------------------------------------------
def repro_calls(ctx):
    """one buffer of bytes from calls on both routes, through the Python layer"""
    out = b""
    rng = np.random.default_rng(77)
    for name, L, F in (("crc-24/lte-a", 6144, 9), ("crc-16/xmodem", 54, 700), ("r64", 1000, 65), ("crc-32", 40000, 3), ("r33", 16384, 2),
                       ("r8", 17, 130), ("r1", 16385, 1)):
        c = ap.Crc(ctx, *BY_NAME[name])
        bits = rng.integers(0, 256, L * F, dtype=np.uint8)
        state = ap.DeviceU64(ctx, F, rng.integers(0, 1 << 63, F, dtype=np.uint64) & np.uint64((1 << c.r) - 1))
        out += c.registers(bits, L, F).to_host().tobytes() + c.registers(bits, L, F, state=state).to_host().tobytes()
        att = c.attach(bits, L)
        host = att.to_host()
        host[rng.integers(0, host.size, 3)] ^= 1
        d, p, s = c.check(host, L, summary="host")
        out += host.tobytes() + d.to_host().tobytes() + p.to_host().tobytes() + np.array(s, np.uint64).tobytes()
        c.close()
    return out


def test_same_bytes_twice(ctx):
    assert repro_calls(ctx) == repro_calls(ctx), "the same calls gave other bytes"


def _child(outdir):
    ctx = ap.Context(0)
    for tag, env in (("nt0", {"AETH_NT": "0"}), ("nt1", {"AETH_NT": "1"}), ("long", {"AETH_CRC_ROUTE": "2"})):
        for k in ("AETH_NT", "AETH_CRC_ROUTE"):
            os.environ.pop(k, None)
        os.environ.update(env)
        with open(os.path.join(outdir, f"{tag}.bin"), "wb") as f:
            f.write(repro_calls(ctx))
    ctx.close()
    print("crc child ok")


def test_bytes_depend_neither_on_the_cache_policy_nor_on_the_route(ctx, tmp_path):
    """AETH_TUNING=1 with AETH_NT=0, AETH_NT=1 and AETH_CRC_ROUTE=2 in a child process: the bytes of this process"""
    env = dict(os.environ, AETH_TUNING="1")
    for k in ("AETH_NT", "AETH_CRC_ROUTE"):
        env.pop(k, None)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child", str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    want = repro_calls(ctx)
    for tag in ("nt0", "nt1", "long"):
        assert open(tmp_path / f"{tag}.bin", "rb").read() == want, f"{tag} changed the bytes"


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--child":
    _child(sys.argv[2])
