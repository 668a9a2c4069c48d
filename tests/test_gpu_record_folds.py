"""GPU: the three output flavours of the record reductions (records only, total only, both) on every path behind the
chunk kernel (csrc/aeth_reduce.h, run_blocks): a block that is one chunk (no fold), blocks of several chunks (the
per-block fold), and the total folded from the caller's records or from the slab's.

For sync.line_into, sync.lag_into (lag 5, no history) and mov.search_into (LAG W=16 L=64, POWER W=33), n = 3 chunks + 17
of the family's own chunk, block in (0, 64, chunk, chunk + 1, 2 chunk + 5):
  - the record bytes of "records only" are those of "both", the total's bytes of "total only" are those of "both";
  - the total is the host's fold of the device's block records: mov by mov_truth.fold_records (any order gives the same
    record), sync bit for bit by THE TREE restated below, and within the bound of tests/test_gpu_sync.py for any order of
    f64 additions against sync_truth.fsum: nb * 2^-52 * sum |record| (nb - 1 additions, each within 2^-53 relative of a
    partial sum that never exceeds sum |record|, plus fsum's own rounding);
  - two sentinel records on either side of the record array are untouched."""
import ctypes as C
import types

import numpy as np
import pytest

from aether_primitives_amd import mov, nco, sync
import mov_truth as mt
import sync_truth as st

pytestmark = pytest.mark.gpu

WORDS = (0x0123_4567_89ab_cdef, nco.word(0.0371), nco.word(-2.5e-7))
N0 = 2 ** 41 + 12345
MOV_CHUNK = 1024
EPS = 2.0 ** -52


def signal(n, seed):
    r = np.random.default_rng(seed)
    return ((r.standard_normal(n) + 1j * r.standard_normal(n)) * 0.7).astype(np.complex64)


def blocks_of(chunk):
    return (0, 64, chunk, chunk + 1, 2 * chunk + 5)


def flavours(ctx, call, dtype, nb):
    """call(rec, total) three ways -> (records of "records only", of "both", total of "total only", of "both"), the totals
    as rows of `dtype`; checks the sentinels"""
    size = dtype.itemsize
    fill = np.frombuffer(b"\x5a" * (size * (nb + 4)), dtype)
    dev = ctx.alloc(fill.nbytes)
    inner = types.SimpleNamespace(_p=lambda: C.c_void_p(dev + 2 * size))      # the records, two sentinels on either side
    got = []
    try:
        for total in (False, True):
            buf = fill.copy()
            ctx.upload(dev, buf)
            tot = call(inner, total)
            assert (tot is not None) == total
            ctx.sync()
            ctx.download(dev, buf)
            assert buf[:2].tobytes() == b"\x5a" * (2 * size) == buf[-2:].tobytes(), ("sentinels", total)
            got.append(buf[2:-2].copy())
        only = call(None, True)
    finally:
        ctx.free(dev)
    return got[0], got[1], np.frombuffer(bytes(only), dtype)[0], np.frombuffer(bytes(tot), dtype)[0]


def tree_sum(v):
    """THE TREE of csrc/aeth_reduce.h over f64 values: lane t adds values t, t + 256, ... from -0.0, the xor butterfly
    inside each wave of 64, the waves as (w0 + w1) + (w2 + w3)"""
    lanes = np.full(256, -0.0)
    for k in range(0, v.size, 256):
        part = v[k:k + 256]
        lanes[:part.size] = lanes[:part.size] + part
    lane = np.arange(256)
    for mask in (32, 16, 8, 4, 2, 1):
        lanes = lanes + lanes[lane ^ mask]
    return (lanes[0] + lanes[64]) + (lanes[128] + lanes[192])


def check_sync(ctx, call, n, block):
    nb = sync.n_blocks(n, block)
    rec_only, rec_both, tot_only, tot_both = flavours(ctx, call, st.RECORD_DTYPE, nb)
    assert rec_only.tobytes() == rec_both.tobytes(), block
    assert tot_only.tobytes() == tot_both.tobytes(), block
    for f in ("n", "n_nonfinite"):
        assert tot_both[f] == rec_both[f].sum(), (block, f)
    assert tot_both["reserved"] == 0 and tot_both["n"] > 0
    for f in ("re", "im", "mass"):
        want = st.fsum(rec_both[f])
        bound = nb * EPS * st.fsum(np.abs(rec_both[f]))
        print(f"block {block} {f}: total - fsum {tot_both[f] - want:.3e}, bound {bound:.3e}")
        assert abs(tot_both[f] - want) <= bound, (block, f)
        assert st.same_f64_bits(tot_both[f], tree_sum(rec_both[f])), (block, f)


def test_line_flavours(ctx):
    n = 3 * sync.chunk() + 17
    xd = ctx.vec(signal(n, 41))
    for block in blocks_of(sync.chunk()):
        check_sync(ctx, lambda rec, total: sync.line_into(ctx, xd, st.POW4, rec, WORDS, N0, block, total=total), n, block)


def test_lag_flavours(ctx):
    n = 3 * sync.chunk() + 17
    xd = ctx.vec(signal(n, 42))
    for block in blocks_of(sync.chunk()):
        check_sync(ctx, lambda rec, total: sync.lag_into(ctx, xd, 4, 5, rec, None, block, total=total), n, block)


@pytest.mark.parametrize("kind,W,L", ((mov.LAG, 16, 64), (mov.POWER, 33, 0)))
def test_search_flavours(ctx, kind, W, L):
    n = 3 * MOV_CHUNK + 17
    xd = ctx.vec(signal(n, 43))
    for block in blocks_of(MOV_CHUNK):
        nb = mov.n_blocks(n, block)
        rec_only, rec_both, tot_only, tot_both = flavours(
            ctx, lambda rec, total: mov.search_into(ctx, xd, kind, W, L, 1e-9, 0.5, rec, None, block, best=total), mt.PEAK_DTYPE, nb)
        assert rec_only.tobytes() == rec_both.tobytes(), block
        assert tot_only.tobytes() == tot_both.tobytes(), block
        fold = mt.fold_records(rec_both, n)
        assert tot_both["index"] < n, block
        for f in ("index", "first", "n_nan", "reserved"):
            assert tot_both[f] == fold[f], (block, f, tot_both[f], fold[f])
        for f in ("p_re", "p_im", "r", "r_lag", "metric"):
            assert mt.same_bits(tot_both[f], fold[f]), (block, f)
