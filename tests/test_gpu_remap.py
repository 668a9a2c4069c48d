"""GPU: aeth_remap_exec (include/aether_hip.h) against the numpy restatement tests/remap_truth.py, byte for byte, with
guard bytes around every output checked unchanged.

  1. degenerate maps: the 1 -> 1 identity, an all-fill table under two fills, repetition, puncture 3/4 and its inverse.
  2. periods that are no multiple of 4 or 16, random maps with -1 entries and repeats.
  3. every output alignment x input alignments 0, 1, 3, 15 at lengths around 16 and around the period.
  4. tile edges: g - 1, g, g + 1, 2 g + 1 periods (g from aeth_remap_tile), with and without a partial last period.
  5. the route boundary: the largest period on the tile route, the next one on the gather route, rows_cols(255, 257) and a
     period of 2^20.
  6. a stream cut at period boundaries, a repeated run, both cache policies (a child process).
  7. int8 data: every value passes unchanged.
  8. exec refusals launch nothing; refused creates leave the device's free memory unchanged.
  9. ConvCode.encode -> Remap -> Remap.inverse() -> decode_stream returns the bits at rate 2/3 and 3/4."""
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
from aether_primitives_amd import _lib, remap         # noqa: E402
import remap_truth as rt                              # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = 0xA5
TILE, GATHER = remap.ROUTE_TILE, remap.ROUTE_GATHER


def data(n, seed, dtype=np.uint8):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).view(dtype)


def random_map(r_out, r_in, seed):
    """entries in [-1, r_in): about one in six is -1, and repeats come by themselves"""
    rng = np.random.default_rng(seed)
    m = rng.integers(0, r_in, r_out).astype(np.int32)
    m[rng.integers(0, 6, r_out) == 0] = -1
    return m


def run(ctx, rm, x, n_out, fill=0, in_off=0, out_off=0, n_in=None):
    """x at `in_off` bytes behind an allocation's start, the output `out_off` bytes behind GUARD sentinels: -> the n_out
    bytes as x's dtype; the guards on both sides are checked"""
    x = np.ascontiguousarray(x)
    n_in = x.size if n_in is None else n_in
    din = ctx.alloc(in_off + x.size + 16)
    dout = ctx.alloc(GUARD + out_off + n_out + GUARD)
    try:
        if x.size:
            ctx.upload(din + in_off, x.view(np.uint8))
        ctx.upload(dout, np.full(GUARD + out_off + n_out + GUARD, SENTINEL, np.uint8))
        _lib.check(rm._lib.aeth_remap_exec(rm.h, C.c_void_p(din + in_off), n_in, C.c_void_p(dout + GUARD + out_off), n_out, fill))
        got = np.empty(GUARD + out_off + n_out + GUARD, np.uint8)
        ctx.download(dout, got)
    finally:
        ctx.free(din); ctx.free(dout)
    lo = GUARD + out_off
    assert (got[:lo] == SENTINEL).all(), "bytes in front of the output were written"
    assert (got[lo + n_out:] == SENTINEL).all(), "bytes behind the output were written"
    return got[lo:lo + n_out].view(x.dtype)


def check(ctx, rm, n_out, seed, fill=0, in_off=0, out_off=0, dtype=np.uint8):
    need = rm.in_count(n_out)
    assert need == rt.in_count(rm.map, rm.r_in, n_out)
    x = data(need, seed, dtype)
    got = run(ctx, rm, x, n_out, fill, in_off, out_off)
    want = rt.remap(x, rm.map, rm.r_in, n_out, fill)
    assert got.tobytes() == want.tobytes(), (rm.r_in, rm.r_out, n_out, fill, in_off, out_off, np.flatnonzero(got != want)[:8])


# ---- 1: degenerate maps ------------------------------------------------------------------------------------------------
def test_identity_of_period_one(ctx):
    rm = ap.Remap(ctx, [0], 1)
    assert (rm.r_in, rm.r_out, rm.route) == (1, 1, TILE) and rm.tile >= 1
    for n in (1, 5, 4097, 3 * rm.tile + 7):
        check(ctx, rm, n, n)


@pytest.mark.parametrize("fill", (0x00, 0x80, 0xff))
def test_a_table_of_minus_one_writes_the_fill(ctx, fill):
    rm = ap.Remap(ctx, [-1], 1)
    for n in (1, 33, 5000):
        assert rm.in_count(n) == n                                    # whole periods count, whatever the table reads
        got = run(ctx, rm, data(n, n), n, fill)
        assert (got == fill).all()


def test_repetition(ctx):
    rm = ap.Remap(ctx, [0, 0, 1, 1], 2)
    for n in (4, 6, 7, 4000, 4003):
        check(ctx, rm, n, n)


@pytest.mark.parametrize("fill", (0x00, 0x80))
def test_puncture_three_quarters_and_its_inverse(ctx, fill):
    p = ap.Remap.puncture(ctx, [1, 1, 1, 0, 0, 1])
    d = p.inverse()
    assert (p.r_in, p.r_out, d.r_in, d.r_out) == (6, 4, 4, 6)
    assert d.map.tolist() == [0, 1, 2, -1, -1, 3]
    for q in (1, 7, 1000):
        check(ctx, p, 4 * q, q, fill)
        check(ctx, d, 6 * q, q, fill)
        check(ctx, d, 6 * q + 4, q, fill)                             # a partial period that ends in fills
    x = data(6000, 5)
    back = run(ctx, d, run(ctx, p, x, 4000), 6000, fill)
    keep = np.tile(np.array([1, 1, 1, 0, 0, 1], bool), 1000)
    assert (back[keep] == x[keep]).all() and (back[~keep] == fill).all()


# ---- 2: odd periods ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r_in", (5, 64, 288))
@pytest.mark.parametrize("r_out", (3, 7, 13, 48, 192, 193))
def test_random_maps_at_odd_periods(ctx, r_out, r_in):
    rm = ap.Remap(ctx, random_map(r_out, r_in, 1000 * r_out + r_in), r_in)
    assert rm.route == TILE
    for n_out in (r_out, 5 * r_out + r_out // 2, (2 * rm.tile + 3) * r_out + 1):
        check(ctx, rm, n_out, n_out, fill=0x3c, in_off=r_out % 16, out_off=r_in % 16)


# ---- 3: alignment ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_off", (0, 1, 3, 15))
def test_every_output_alignment(ctx, in_off):
    rm = ap.Remap.bicm16(ctx, 192, 4)
    for out_off in range(16):
        for n_out in (1, 15, 16, 17, 191, 192, 193):
            check(ctx, rm, n_out, 16 * n_out + out_off, in_off=in_off, out_off=out_off)


@pytest.mark.parametrize("in_off,out_off", ((0, 0), (1, 15), (15, 1), (3, 8)))
def test_alignment_on_the_gather_route(ctx, in_off, out_off):
    m, r_in = remap.rows_cols_map(255, 257)
    rm = ap.Remap(ctx, m, r_in)
    assert rm.route == GATHER and rm.tile == 0
    for n_out in (1, 15, 16, 17, 65535, 65536 + 33):
        check(ctx, rm, n_out, n_out, in_off=in_off, out_off=out_off)


# ---- 4: tile edges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("r_out,r_in", ((192, 288), (193, 193), (6, 4), (3001, 2999)))
def test_tile_edges(ctx, r_out, r_in):
    rm = ap.Remap(ctx, random_map(r_out, r_in, r_out + r_in), r_in)
    g = rm.tile
    assert rm.route == TILE and g >= 1
    for q in (g - 1, g, g + 1, 2 * g + 1):
        for part in (0, 1, r_out - 1):
            if q * r_out + part:
                check(ctx, rm, q * r_out + part, q + part, fill=0x11, in_off=5, out_off=11)


# ---- 5: the route boundary ---------------------------------------------------------------------------------------------
def test_the_largest_tile_period_and_the_next_one_up(ctx):
    def route(r):
        return ap.Remap(ctx, np.arange(r, dtype=np.int32), r).route
    lo, hi = 1024, 32768                                              # the tile and its table fit 32 KiB: tile below, gather above
    assert route(lo) == TILE and route(hi) == GATHER
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if route(mid) == TILE else (lo, mid)
    for r, want in ((lo, TILE), (hi, GATHER)):
        rm = ap.Remap(ctx, random_map(r, r, r), r)
        assert rm.route == want and (rm.tile >= 1) == (want == TILE)
        for n_out in (r, 3 * r + 1, 2 * r + r - 1):
            check(ctx, rm, n_out, n_out, fill=0x77, in_off=9, out_off=6)
    print(f"largest tile period {lo}")


def test_rows_cols_255_by_257_on_the_gather_route(ctx):
    rm = ap.Remap.rows_cols(ctx, 255, 257)
    assert rm.route == GATHER
    for n_out in (65535, 4 * 65535 + 100):
        check(ctx, rm, n_out, n_out)


def test_a_period_of_two_to_the_twenty(ctx):
    r = 1 << 20
    m = random_map(r, r, 20)
    rm = ap.Remap(ctx, m, r)
    assert rm.route == GATHER and (rm.r_in, rm.r_out) == (r, r)
    check(ctx, rm, r, 1, fill=0xee)
    check(ctx, rm, r + 12345, 2, fill=0xee, in_off=7, out_off=13)


# ---- 6: chunks and reproducibility -------------------------------------------------------------------------------------
def repro_calls(ctx):
    """a fixed list of calls on both routes -> their bytes"""
    b = b""
    pm, p = remap.puncture_map([1, 1, 1, 0, 0, 1])
    tm, t_in = remap.compose_maps(pm, p, *remap.bicm16_map(192, 4))
    for m, r_in, n_out, seed in ((tm, t_in, 192 * 300 + 77, 1), (random_map(193, 64, 2), 64, 193 * 150, 2),
                                 (remap.rows_cols_map(255, 257)[0], 65535, 65535 * 2 + 5, 3)):
        rm = ap.Remap(ctx, m, r_in)
        x = data(rm.in_count(n_out), seed)
        got = run(ctx, rm, x, n_out, 0x42, in_off=3, out_off=5)
        assert got.tobytes() == rt.remap(x, m, r_in, n_out, 0x42).tobytes()
        b += got.tobytes()
    return b


def test_same_bytes_twice(ctx):
    assert repro_calls(ctx) == repro_calls(ctx), "the same calls gave other bytes"


def _child(outdir):
    ctx = ap.Context(0)
    for nt in ("0", "1"):
        os.environ["AETH_NT"] = nt
        with open(os.path.join(outdir, f"nt{nt}.bin"), "wb") as f:
            f.write(repro_calls(ctx))
    ctx.close()
    print("remap child ok")


def test_bytes_do_not_depend_on_the_cache_policy(ctx, tmp_path):
    """AETH_TUNING=1 with AETH_NT=0 and AETH_NT=1 in a child process: the bytes of this process"""
    env = dict(os.environ, AETH_TUNING="1")
    env.pop("AETH_NT", None)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child", str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    want = repro_calls(ctx)
    for nt in ("0", "1"):
        assert open(tmp_path / f"nt{nt}.bin", "rb").read() == want, f"AETH_NT={nt} changed the bytes"


@pytest.mark.parametrize("which", ("tile", "gather"))
def test_a_stream_cut_at_period_boundaries_equals_one_call(ctx, which):
    if which == "tile":
        rm = ap.Remap(ctx, random_map(192, 288, 9), 288)
    else:
        rm = ap.Remap.rows_cols(ctx, 255, 257)
    q, cuts = 40, (0, 7, 29, 40)
    x = data(q * rm.r_in, 77)
    whole = run(ctx, rm, x, q * rm.r_out, 0x99)
    parts = [run(ctx, rm, x[a * rm.r_in:b * rm.r_in], (b - a) * rm.r_out, 0x99, in_off=a % 16, out_off=b % 16) for a, b in zip(cuts, cuts[1:])]
    assert np.concatenate(parts).tobytes() == whole.tobytes()


# ---- 7: int8 ------------------------------------------------------------------------------------------------------------
def test_every_int8_value_passes_unchanged(ctx):
    rm = ap.Remap.rows_cols(ctx, 16, 16)
    x = np.arange(-128, 128).astype(np.int8)
    soft = ap.DeviceSoft(ctx, 256, x)
    out = rm.exec(soft)
    assert isinstance(out, ap.DeviceSoft) and out.n == 256
    assert out.to_host().tobytes() == x.reshape(16, 16).T.reshape(-1).tobytes()
    bits = rm.exec(ap.DeviceBits(ctx, 256, x.view(np.uint8)))
    assert isinstance(bits, ap.DeviceBits) and bits.to_host().tobytes() == out.to_host().tobytes()
    d = ap.Remap.puncture(ctx, [1, 0, 1]).inverse()
    got = d.exec(ap.DeviceSoft(ctx, 256, x), fill=0x80)
    assert got.n == 384 and got.to_host().tobytes() == rt.remap(x, d.map, d.r_in, 384, 0x80).tobytes()


# ---- 8: refusals ---------------------------------------------------------------------------------------------------------
def test_exec_refusals_launch_nothing(ctx):
    lib = _lib.load()
    rm = ap.Remap(ctx, random_map(192, 288, 4), 288)
    n_out = 192 * 3 + 50
    need = rm.in_count(n_out)
    din, dout = ctx.alloc(need + 16), ctx.alloc(n_out + 16)
    try:
        ctx.upload(dout, np.full(n_out + 16, SENTINEL, np.uint8))
        rc = lib.aeth_remap_exec(rm.h, C.c_void_p(din), need - 1, C.c_void_p(dout), n_out, 0)
        msg = lib.aeth_last_error().decode()
        assert rc == _lib.E_LEN and str(need - 1) in msg and str(need) in msg, msg
        assert lib.aeth_remap_exec(rm.h, C.c_void_p(din), need + 7, C.c_void_p(din + need + 6), n_out, 0) == _lib.E_ARG
        assert b"overlaps" in lib.aeth_last_error()
        assert lib.aeth_remap_exec(rm.h, None, need, C.c_void_p(dout), n_out, 0) == _lib.E_ARG and b"null" in lib.aeth_last_error()
        assert lib.aeth_remap_exec(rm.h, C.c_void_p(din), need, None, n_out, 0) == _lib.E_ARG and b"null" in lib.aeth_last_error()
        # lengths of 2^32: the pointers are never followed
        a, b = C.c_void_p(0x100000), C.c_void_p(0x7000_0000_0000)
        assert lib.aeth_remap_exec(rm.h, a, 1 << 33, b, 1 << 32, 0) == _lib.E_UNSUPPORTED and str(1 << 32).encode() in lib.aeth_last_error()
        assert lib.aeth_remap_exec(rm.h, a, 1 << 32, b, 192, 0) == _lib.E_UNSUPPORTED and str(1 << 32).encode() in lib.aeth_last_error()
        assert lib.aeth_remap_exec(rm.h, None, 0, None, 0, 0) == _lib.OK                 # nothing to do
        got = np.empty(n_out + 16, np.uint8)
        ctx.download(dout, got)
        assert (got == SENTINEL).all(), "a refused call wrote to its output"
    finally:
        ctx.free(din); ctx.free(dout)


def _free_bytes():
    hip = _lib.load()                              # hipMemGetInfo of the runtime the library is bound to
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_refused_creates_leave_free_memory_unchanged(ctx):
    lib, h = _lib.load(), C.c_void_p(0x55)
    m = np.arange(4096, dtype=np.int32)
    bad = m.copy()
    bad[4095] = 4096
    ctx.sync()
    free0 = _free_bytes()
    for _ in range(25):
        for tab, r_out, r_in, named in ((bad, 4096, 4096, "map[4095] = 4096"), (m, 4096, 0, "input period 0"),
                                        (m, 0, 4096, "output period 0"), (m, 4096, (1 << 20) + 1, "input period 1048577")):
            assert lib.aeth_remap_create(ctx.h, tab.ctypes.data_as(C.c_void_p), r_out, r_in, C.byref(h)) == _lib.E_ARG and not h.value
            assert named.encode() in lib.aeth_last_error()
    ctx.sync()
    assert _free_bytes() == free0
    rm = ap.Remap(ctx, m, 4096)                                        # the accepted table is served, and freed again
    check(ctx, rm, 4096 * 3, 1)
    rm.close()


# ---- 9: the chain ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", ([1, 1, 1, 0], [1, 1, 1, 0, 0, 1]))
def test_encode_puncture_depuncture_decode_returns_the_bits(ctx, keep):
    nbits = 12 * 250                                                  # coded bits: a multiple of both patterns
    code = ap.ConvCode(ctx, 7, (0o133, 0o171))
    p = ap.Remap.puncture(ctx, keep)
    bits = np.random.default_rng(len(keep)).integers(0, 2, nbits, dtype=np.uint8)
    sent = p.exec(code.encode(ap.DeviceBits(ctx, nbits, bits)))
    assert sent.n == 2 * nbits * sum(keep) // len(keep)
    soft = ap.DeviceSoft(ctx, sent.n, (127 - 254 * sent.to_host().astype(np.int16)).astype(np.int8))
    back = p.inverse().exec(soft, fill=0)
    assert back.n == 2 * nbits and (back.to_host().reshape(-1, len(keep))[:, np.array(keep) == 0] == 0).all()
    assert (code.decode_stream(back).to_host() == bits).all()


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        _child(sys.argv[2])
