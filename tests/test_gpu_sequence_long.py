"""GPU: the device LFSR sequences (csrc/aeth_sequence.hip) where tests/test_gpu_sequence.py does not reach: jump levels
6 .. 16, spreading factors of a round and more, and both cache policies forced.  Truth is tests/seq_truth.py; every
comparison is byte for byte (uint32 for uint32 for cf32), nothing against a tolerance.

A wave reaches chunk c (C = 16384 positions) by one matrix-vector product per set bit j of c, with the table rows of
level j, loaded eight levels at a time (jb = 0, 8, 16, 24); a call of up to 2^j chunks passes nlevels = j.  The calls
here:

  bits, scramble     1025 C + 4102 positions   1026 chunks   nlevels 11   every chunk compared
  chips, spread       257 C + 4102              258 chunks   nlevels  9   every chunk compared
  bits          2^30 + C + 4102               65538 chunks   nlevels 17   about 45 slices compared: both sides of the
                                                                          start of chunk 2^j for j = 0 .. 16, chunk
                                                                          65535 (sixteen bits set), chunks 65536 and
                                                                          65537, 24 chunks drawn at random
  spread, sf >= one round   <= 900021            <= 55 chunks   nlevels  6
  both cache policies       2 C + 4102              3 chunks   nlevels  2

Levels 17 .. 31 need one call of 2 GiB .. 32 TiB and are not run.  What carries over to them: the loop body of
`generate` is the same for every level j; three of the four batches (jb = 0, 8, 16) have executed, the third with one
level in it and seven switched off by `jb + i < nlevels`; and the content of the table for every j is P^(2^(14 + j)),
the very matrices aeth_seq_window multiplies at skip 2^64 - 1 (tests/test_seq_window.py).  The 1 GiB call is above the
128 MiB at which a launch streams past the cache, so it is also the non-temporal build of `bits` at length; all five
non-temporal builds (bits, scramble, chips, spread with sf = 1 aligned, spread generic) and their five cached twins run
in the child process at the bottom, under AETH_NT = 1 and 0."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):                             # also run as a script: the AETH_NT child
    if _p not in sys.path:
        sys.path.insert(0, _p)

import seq_truth                                                           # noqa: E402
import test_gpu_sequence as base                                           # noqa: E402
from test_gpu_sequence import CH, FAR, MAPPINGS, SETS, Raw, _bits_at, _spread_truth, _symbols      # noqa: E402

import aether_primitives_amd as ap                                         # noqa: E402
from aether_primitives_amd import _lib                                     # noqa: E402

pytestmark = pytest.mark.gpu

NB = 1025 * CH + 4097 + 5                           # bits, scramble
NC = 257 * CH + 4097 + 5                            # chips, spread
NL = 2 ** 30 + CH + 4097 + 5                        # the long bits call
NP = 2 * CH + 4097 + 5                              # both cache policies
GUARD = 32
CGUARD = np.complex64(complex(123.0, -456.0))


def nlevels(n, nhead):
    """bits of the largest chunk index of a call whose first nhead elements sit in front of the 16-byte aligned body"""
    return (-(-(n - nhead) // CH) - 1).bit_length()


@functools.lru_cache(maxsize=4)
def truth(name, skip):
    """c[skip .. skip + NB + 256) of a set, as test_gpu_sequence.truth makes it; the last few (set, skip) are kept"""
    return base.truth.__wrapped__(name, skip, NB + 256)


@pytest.fixture(scope="module")
def seqs(ctx):
    made = {name: ap.Sequence(ctx, *regs) for name, (regs, _) in SETS.items()}
    for s in made.values():
        assert s.chunk == CH == 16384
    yield made
    made.clear()


def _slot(first):
    """element offset into a 16-byte aligned cf32 buffer: first = 0 -> 16-byte aligned, 1 -> 8- but not 16-byte; both
    leave room for a guard in front"""
    return 2 if first == 0 else 1


def _guarded_vec(ctx, n, first):
    """n cf32 at _slot(first) of a buffer of guards -> (whole, the slice, the guards, slot)"""
    slot = _slot(first)
    guard = np.full(n + 6, CGUARD)
    vec = ctx.empty(n + 6)
    ctx.upload(vec.ptr, guard)
    return vec, vec.slice(slot, slot + n), guard, slot


def _u32(a):
    return a.view(np.uint32).reshape(-1, 2)


def _first_bad(got, want):
    bad = got != want
    return int(np.argmax(bad.reshape(bad.shape[0], -1).any(axis=1))) if bad.any() else None


# ---- 1. levels 6 - 10: every epilogue, every position ---------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SETS))
def test_bits_1026_chunks(ctx, seqs, name):
    seq, init = seqs[name], SETS[name][1]
    n = NB
    buf = Raw(ctx, n + 2 * GUARD + 16)
    fill = np.full(buf.nbytes, 0xAA, np.uint8)
    for skip in (0, FAR):
        t = truth(name, skip)[:n]
        for off in (0, 5):
            nhead = -off & 15
            assert -(-(n - nhead) // CH) == 1026 and nlevels(n, nhead) == 11
            buf.put(fill)
            _bits_at(seq, init, skip, buf.ptr + GUARD + off, n)
            got = buf.get()
            body = got[GUARD + off:GUARD + off + n]
            assert (body == t).all(), (name, skip, off, _first_bad(body, t))
            assert (got[:GUARD + off] == 0xAA).all() and (got[GUARD + off + n:] == 0xAA).all(), (name, skip, off)


@pytest.mark.parametrize("name", ["gold", "four"])
def test_scramble_1026_chunks(ctx, seqs, name):
    seq, init = seqs[name], SETS[name][1]
    lib = seq._lib
    n = NB
    data = np.random.default_rng(816).integers(0, 256, n + 64, dtype=np.uint8)
    src, dst = Raw(ctx, n + 64), Raw(ctx, n + 64)
    src.put(data)
    fill = np.full(dst.nbytes, 0xAA, np.uint8)
    for skip in (1600, FAR):
        t = truth(name, skip)[:n]
        for ioff, ooff in ((3, 0), (0, 5)):                             # `in` misaligned against `out`, both ways
            assert nlevels(n, -ooff & 15) == 11
            want = (data[ioff:ioff + n] & 1) ^ t
            dst.put(fill)
            _lib.check(lib.aeth_seq_scramble(seq.h, seq._init(init), skip, C.c_void_p(src.ptr + ioff), C.c_void_p(dst.ptr + 16 + ooff), n))
            got = dst.get()
            body = got[16 + ooff:16 + ooff + n]
            assert (body == want).all(), (name, skip, ioff, ooff, _first_bad(body, want))
            assert (got[:16 + ooff] == 0xAA).all() and (got[16 + ooff + n:] == 0xAA).all(), (name, skip, ioff, ooff)
        assert (src.get() == data).all()
        ooff = 7                                                        # in place, then once more: in & 1 comes back
        assert nlevels(n, -ooff & 15) == 11
        p = C.c_void_p(dst.ptr + ooff)
        dst.put(data)
        _lib.check(lib.aeth_seq_scramble(seq.h, seq._init(init), skip, p, p, n))
        got = dst.get()
        want = (data[ooff:ooff + n] & 1) ^ t
        assert (got[ooff:ooff + n] == want).all(), (name, skip, _first_bad(got[ooff:ooff + n], want))
        assert (got[:ooff] == data[:ooff]).all() and (got[ooff + n:] == data[ooff + n:]).all()
        _lib.check(lib.aeth_seq_scramble(seq.h, seq._init(init), skip, p, p, n))
        got = dst.get()
        assert (got[ooff:ooff + n] == data[ooff:ooff + n] & 1).all(), (name, skip)
        assert (got[:ooff] == data[:ooff]).all() and (got[ooff + n:] == data[ooff + n:]).all()


@pytest.mark.parametrize("name", ["gold", "four", "o64"])
def test_chips_258_chunks(ctx, seqs, name):
    seq, init = seqs[name], SETS[name][1]
    n = NC
    vec = ctx.empty(n + 4)
    guard = np.full(n + 4, CGUARD)
    for skip in (1600, FAR):
        t = truth(name, skip)[:n]
        for first in (1, 2):                                            # 1: 8- but not 16-byte aligned; 2: 16-byte aligned
            assert -(-(n - first % 2) // CH) == 258 and nlevels(n, first % 2) == 9
            for zero, one in MAPPINGS:
                ctx.upload(vec.ptr, guard)
                seq.chips(init, n, skip=skip, zero=zero, one=one, out=vec.slice(first, first + n))
                got = vec.to_host()
                want = np.where(t != 0, np.complex64(one), np.complex64(zero)).astype(np.complex64)
                body = got[first:first + n]
                assert (_u32(body) == _u32(want)).all(), (name, skip, first, one, _first_bad(_u32(body), _u32(want)))
                assert (got[:first] == guard[:first]).all() and (got[first + n:] == guard[first + n:]).all()


@pytest.mark.parametrize("name", ["gold", "four"])
def test_spread_258_chunks(ctx, seqs, name):
    seq, init = seqs[name], SETS[name][1]
    n = NC
    sym1 = _symbols(n, 819)
    nsym3 = -(-n // 3)
    sym3 = _symbols(nsym3, 820)
    d_sym3 = ctx.vec(sym3)
    for skip in (1600, FAR):
        t = truth(name, skip)
        # sf = 1, symbols and output both on an odd slot: the build that loads its symbols 16 bytes at a time
        assert nlevels(n, 1) == 9
        svec, d_sym, sguard, sslot = _guarded_vec(ctx, n, 1)
        ctx.upload(d_sym.ptr, sym1)
        vec, out, guard, slot = _guarded_vec(ctx, n, 1)
        seq.spread(init, d_sym, 1, skip=skip, out=out)
        got = vec.to_host()
        want = _spread_truth(sym1, 1, t)
        body = _u32(got[slot:slot + n])
        assert (body == want).all(), (name, skip, "sf1", _first_bad(body, want))
        assert (got[:slot] == guard[:slot]).all() and (got[slot + n:] == guard[slot + n:]).all()
        assert (_u32(d_sym.to_host()) == _u32(sym1)).all()
        # in place on that slot
        seq.spread(init, d_sym, 1, skip=skip, out=d_sym)
        got = svec.to_host()
        body = _u32(got[sslot:sslot + n])
        assert (body == want).all(), (name, skip, "sf1 in place", _first_bad(body, want))
        assert (got[:sslot] == sguard[:sslot]).all() and (got[sslot + n:] == sguard[sslot + n:]).all()
        del svec, d_sym, vec, out
        # sf = 3: a symbol index per position
        n3 = nsym3 * 3
        want = _spread_truth(sym3, 3, t)
        for first in (0, 1):
            assert nlevels(n3, first) == 9
            vec, out, guard, slot = _guarded_vec(ctx, n3, first)
            seq.spread(init, d_sym3, 3, skip=skip, out=out)
            got = vec.to_host()
            body = _u32(got[slot:slot + n3])
            assert (body == want).all(), (name, skip, "sf3", first, _first_bad(body, want))
            assert (got[:slot] == guard[:slot]).all() and (got[slot + n3:] == guard[slot + n3:]).all()
            del vec, out
        assert (_u32(d_sym3.to_host()) == _u32(sym3)).all()


# ---- 2. levels 11 - 16: one call of 1 GiB, compared on slices -------------------------------------------------------------
def _long_slices(n, b):
    """byte ranges [lo, hi) of the call to compare; chunk k is [b + k C, b + (k + 1) C)"""
    nchunks = -(-(n - b) // CH)
    r = [(0, b + 4096 + 64)]
    r += [(b + (CH << j) - 64, b + (CH << j) + 4096 + 64) for j in range(17)]
    r.append((b + 65535 * CH, b + 65536 * CH))                         # sixteen bits set
    r.append((b + 65536 * CH, n))                                      # bit 16 alone, then bits 16 and 0, to the end
    picks = sorted(int(k) for k in np.random.default_rng(815).integers(0, nchunks - 2, 24))
    assert sum(k >= 2 ** 15 for k in picks) >= 8
    r += [(b + k * CH, b + (k + 1) * CH) for k in picks]
    assert all(0 <= lo < hi <= n for lo, hi in r)
    return r


@pytest.mark.parametrize("name,skip", [("gold", 1600), ("four", FAR)])
def test_bits_65538_chunks_on_slices(ctx, seqs, name, skip):
    seq, (regs, init) = seqs[name], SETS[name]
    n, front = NL, GUARD + 5
    back = 96 - front
    nhead = -front & 15
    assert nhead == 11 and -(-(n - nhead) // CH) == 65538 and nlevels(n, nhead) == 17
    buf = Raw(ctx, n + 96)
    try:
        ctx.upload(buf.ptr, np.full(front, 0xAA, np.uint8))               # the guards: two small uploads
        ctx.upload(buf.ptr + front + n, np.full(back, 0xAA, np.uint8))
        _bits_at(seq, init, skip, buf.ptr + front, n)
        slices = _long_slices(n, nhead)
        assert len(slices) == 44
        for lo, hi in slices:
            got = np.empty(hi - lo, np.uint8)
            ctx.download(buf.ptr + front + lo, got)
            want = seq_truth.truth(regs, init, skip + lo, hi - lo)
            assert (got == want).all(), (name, skip, lo, hi, "chunk", (lo + _first_bad(got, want) - nhead) // CH, "byte", lo + _first_bad(got, want))
        g = np.empty(front, np.uint8)
        ctx.download(buf.ptr, g)
        assert (g == 0xAA).all()
        g = np.empty(back, np.uint8)
        ctx.download(buf.ptr + front + n, g)
        assert (g == 0xAA).all()
    finally:
        ctx.free(buf.ptr); buf.ptr = None                               # before the next test allocates


# ---- 3. spread: a symbol as long as a round, a chunk, and longer ----------------------------------------------------------
LONG_SF = ((161, 4096, 1), (130, 5000, 1), (41, 16384, 0), (41, 16385, 1), (7, 100003, 1), (3, 300007, 0))


@pytest.mark.parametrize("nsym,sf,first", LONG_SF)
@pytest.mark.parametrize("name", ["m7", "gold"])
def test_spread_long_symbols(ctx, seqs, name, nsym, sf, first):
    seq, init = seqs[name], SETS[name][1]
    n = nsym * sf
    assert n <= 900021 and nlevels(n, first) == 6
    sym = _symbols(nsym, 821 + nsym)
    d_sym = ctx.vec(sym)
    for skip in (1600, FAR):
        vec, out, guard, slot = _guarded_vec(ctx, n, first)
        seq.spread(init, d_sym, sf, skip=skip, out=out)
        got = vec.to_host()
        want = _spread_truth(sym, sf, truth(name, skip))
        body = _u32(got[slot:slot + n])
        assert (body == want).all(), (name, nsym, sf, first, skip, _first_bad(body, want))
        assert (got[:slot] == guard[:slot]).all() and (got[slot + n:] == guard[slot + n:]).all()
        assert (_u32(d_sym.to_host()) == _u32(sym)).all()


# ---- 4. the same bytes under both cache policies, forced --------------------------------------------------------------------
POLICY_SET, POLICY_SKIP = "four", FAR
POLICY_CASES = ("bits 0", "bits 5", "scramble 3->0", "scramble in place 7", "chips 1", "chips 2", "spread sf1 odd odd",
                "spread sf1 0->1", "spread sf3")


def _policy_inputs():
    n = NP
    data = np.random.default_rng(822).integers(0, 256, n + 64, dtype=np.uint8)
    return data, _symbols(n, 823), _symbols(-(-n // 3), 824)


def _policy_bytes(ctx, seq):
    """every case of POLICY_CASES -> the bytes of its output with its guards"""
    init = SETS[POLICY_SET][1]
    lib, n, skip = seq._lib, NP, POLICY_SKIP
    data, sym1, sym3 = _policy_inputs()
    out = []
    for off in (0, 5):
        buf = Raw(ctx, n + 2 * GUARD + 16)
        buf.put(np.full(buf.nbytes, 0xAA, np.uint8))
        _bits_at(seq, init, skip, buf.ptr + GUARD + off, n)
        out.append(buf.get().tobytes())
    src, dst = Raw(ctx, n + 64), Raw(ctx, n + 64)
    src.put(data)
    dst.put(np.full(dst.nbytes, 0xAA, np.uint8))
    _lib.check(lib.aeth_seq_scramble(seq.h, seq._init(init), skip, C.c_void_p(src.ptr + 3), C.c_void_p(dst.ptr + 16), n))
    out.append(dst.get().tobytes())
    dst.put(data)
    p = C.c_void_p(dst.ptr + 7)
    _lib.check(lib.aeth_seq_scramble(seq.h, seq._init(init), skip, p, p, n))
    out.append(dst.get().tobytes())
    for first in (1, 2):
        vec = ctx.vec(np.full(n + 4, CGUARD))
        seq.chips(init, n, skip=skip, out=vec.slice(first, first + n))
        out.append(vec.to_host().tobytes())
    for sslot, oslot in ((1, 1), (0, 1)):                               # equal odd alignment: the SF1 build; else the generic one
        d_sym = ctx.vec(np.concatenate([np.zeros(sslot, np.complex64), sym1]))
        vec = ctx.vec(np.full(n + 4, CGUARD))
        seq.spread(init, d_sym.slice(sslot, sslot + n), 1, skip=skip, out=vec.slice(oslot, oslot + n))
        out.append(vec.to_host().tobytes())
    n3 = sym3.size * 3
    vec = ctx.vec(np.full(n3 + 4, CGUARD))
    seq.spread(init, ctx.vec(sym3), 3, skip=skip, out=vec.slice(1, 1 + n3))
    out.append(vec.to_host().tobytes())
    assert len(out) == len(POLICY_CASES)
    return out


def _policy_truth():
    """what _policy_bytes must return, from seq_truth alone"""
    regs, init = SETS[POLICY_SET]
    n = NP
    data, sym1, sym3 = _policy_inputs()
    n3 = sym3.size * 3
    t = seq_truth.truth(regs, init, POLICY_SKIP, n3)
    out = []
    for off in (0, 5):
        w = np.full(n + 2 * GUARD + 16, 0xAA, np.uint8)
        w[GUARD + off:GUARD + off + n] = t[:n]
        out.append(w.tobytes())
    w = np.full(n + 64, 0xAA, np.uint8)
    w[16:16 + n] = (data[3:3 + n] & 1) ^ t[:n]
    out.append(w.tobytes())
    w = data.copy()
    w[7:7 + n] = (data[7:7 + n] & 1) ^ t[:n]
    out.append(w.tobytes())
    zero, one = MAPPINGS[0]                                             # the defaults of Sequence.chips
    for first in (1, 2):
        w = np.full(n + 4, CGUARD)
        w[first:first + n] = np.where(t[:n] != 0, np.complex64(one), np.complex64(zero))
        out.append(w.tobytes())
    for _ in range(2):
        w = np.full(n + 4, CGUARD)
        w[1:1 + n].view(np.uint32).reshape(-1, 2)[:] = _spread_truth(sym1, 1, t)
        out.append(w.tobytes())
    w = np.full(n3 + 4, CGUARD)
    w[1:1 + n3].view(np.uint32).reshape(-1, 2)[:] = _spread_truth(sym3, 3, t)
    out.append(w.tobytes())
    return out


def _child(outdir):
    ctx = ap.Context(0)
    seq = ap.Sequence(ctx, *SETS[POLICY_SET][0])
    for nt in ("0", "1"):
        os.environ["AETH_NT"] = nt
        for i, b in enumerate(_policy_bytes(ctx, seq)):
            with open(os.path.join(outdir, f"nt{nt}_{i}.bin"), "wb") as f:
                f.write(b)
    del seq
    ctx.close()
    print("sequence child ok")


def test_results_are_the_same_under_both_cache_policies(ctx, seqs, tmp_path):
    assert nlevels(NP, 0) == nlevels(NP, 11) == nlevels(NP, 1) == nlevels(-(-NP // 3) * 3, 1) == 2
    env = dict(os.environ, AETH_TUNING="1")
    env.pop("AETH_NT", None)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child", str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    mine = _policy_bytes(ctx, seqs[POLICY_SET])
    for i, (case, got, want) in enumerate(zip(POLICY_CASES, mine, _policy_truth())):
        assert got == want, f"{case}: not the truth"
        for nt in ("0", "1"):
            assert open(tmp_path / f"nt{nt}_{i}.bin", "rb").read() == got, f"AETH_NT={nt} changed the result of {case}"


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--child":
    _child(sys.argv[2])
