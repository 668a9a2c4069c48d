"""GPU: the host-slice entry points (aeth_host_*, the numpy / HostVec flavours) on BOTH sides of zero-copy.

Every host-slice call takes one of two paths that share no code after HostIO::open (csrc/aeth_runtime.hip):

  pinned   every buffer of the call <= kZeroCopyMax: memcpy into the context's two pinned bounce buffers, the kernel reads
           and writes host memory, one wait, memcpy out
  staged   any buffer larger: hipMemcpyAsync into the context's staging slots stage[0] / stage[1] (grown on demand with
           25 % slack), kernel on device memory, hipMemcpyAsync out

The two limits, from the source lines

  csrc/aeth_internal.h   constexpr size_t kZeroCopyMax = (size_t)256 << 10;
                         pinned = bytes0 <= kZeroCopyMax && bytes1 <= kZeroCopyMax;        (HostIO::open)
  csrc/aeth_fft.hip      static constexpr size_t kFftZeroCopyMax = (size_t)64 << 10;
                         if (bytes <= kFftZeroCopyMax) { ... }                             (aeth_fft_exec_host, _tmp_host)

are stated once below (ZC, FZC); every shape in this file is written relative to them, and the one CPU test at the end
fails when the library's constants move away from them.

Every comparison is bit equality against the oracle or against the device flavour of the same call; the only bound is
the FFT tests' own (-120 dB EVM against f64 truth, within 8 dB of the f32 oracle: test_gpu_fft._check)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import aether_primitives_amd as ap
from aether_primitives_amd import Fir, HipFft, HostVec, Scale, _lib, sampling
from helpers import bits_equal, rand_c64
from test_gpu_fft import _check

# The module holds one test that must run without a GPU, so the mark is put on each GPU test, not on the module.
gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aether_primitives_amd", "csrc")

ZC = 256 << 10      # bytes, so 32768 cf32
FZC = 64 << 10      # bytes, so 8192 points
ZS = ZC // 8        # the largest cf32 slice that stays pinned
FP = FZC // 8       # the longest frame aeth_fft_exec_host transforms on pinned memory
FFT_CACHE_MAX = 8   # kFftCacheMax, csrc/aeth_fft.hip

GUARD = np.complex64(-7.25 + 3.5j)
NMAX = 120000                                       # the longest slice any test takes


def bytes_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(np.uint8) == b.view(np.uint8)).all())


@functools.lru_cache(maxsize=None)
def _operands():
    """two seeded vectors of the longest size; every test takes prefixes, nothing writes to them"""
    a, b = rand_c64(4101, NMAX + 1), rand_c64(4102, NMAX + 1)
    a.flags.writeable = False
    b.flags.writeable = False
    return a, b


# ---- 1. the nine vec ops -------------------------------------------------------------------------------------------------
UNARY = ("vec_scale", "vec_conj", "vec_zero", "vec_mirror")
BINARY = ("vec_add", "vec_sub", "vec_mul", "vec_div", "vec_clone")
FACTOR = 0.37


def _host_op(ctx, op, arr, other):
    v = HostVec(ctx, arr)
    if op == "vec_scale":
        v.vec_scale(FACTOR)
    elif op in BINARY:
        getattr(v, op)(other)
    else:
        getattr(v, op)()


def _oracle_op(oracle, op, a, b):
    if op == "vec_scale":
        return oracle.vec_scale(a, FACTOR)
    if op in BINARY:
        return getattr(oracle, op)(a, b)
    return getattr(oracle, op)(a)


def _slice8(n, fill):
    """(buf, start): self = buf[start:start + n] is 8- but not 16-byte aligned and has a guard sample on either side"""
    buf = np.full(n + 3, GUARD, np.complex64)
    start = 1 if buf.ctypes.data % 16 == 0 else 2
    buf[start:start + n] = fill
    assert buf[start:].ctypes.data % 16 == 8
    return buf, start


def _slice4(n, fill):
    """(floats, view): view is a complex64 slice whose pointer is only 4-byte aligned, one guard float on either side"""
    fb = np.full(2 * n + 2, np.float32(-99.5), np.float32)
    view = fb[1:1 + 2 * n].view(np.complex64)
    view[:] = fill
    assert view.ctypes.data % 8 == 4 and view.size == n
    return fb, view


@gpu
@pytest.mark.parametrize("n", [1, 2, 3, ZS - 1, ZS, ZS + 1, 2 * ZS + 1, 100003])
@pytest.mark.parametrize("op", UNARY + BINARY)
def test_vec_op_both_paths(ctx, oracle, op, n):
    """bit for bit the oracle's; `other` and the samples around `self` in the same allocation are untouched"""
    a, b = (v[:n] for v in _operands())
    exp = _oracle_op(oracle, op, a, b)
    # 8- but not 16-byte aligned, inside a larger array
    buf, st = _slice8(n, a)
    other = b.copy()
    _host_op(ctx, op, buf[st:st + n], other)
    assert bits_equal(buf[st:st + n], exp)
    assert bits_equal(other, b)
    assert bits_equal(buf[:st], np.full(st, GUARD)) and bits_equal(buf[st + n:], np.full(3 - st, GUARD))
    # only 4-byte aligned, both operands: the host entry points check no alignment and both paths copy
    fa, va = _slice4(n, a)
    fo, vo = _slice4(n, b)
    _host_op(ctx, op, va, vo)
    assert bits_equal(va, exp)
    assert bits_equal(vo, b)
    assert fa[0] == fa[-1] == fo[0] == fo[-1] == np.float32(-99.5)


@gpu
@pytest.mark.parametrize("n", [3001, 40000])
@pytest.mark.parametrize("op", BINARY)
def test_vec_op_overlapping_host_operands(ctx, oracle, op, n):
    """both operands are copied before the kernel runs: the result is the oracle's on the ORIGINAL values"""
    orig = _operands()[0][:n + 1]
    h = orig.copy()
    getattr(HostVec(ctx, h[0:n]), op)(h[1:n + 1])
    assert bits_equal(h[:n], getattr(oracle, op)(orig[:n], orig[1:n + 1]))
    assert bits_equal(h[n:], orig[n:])
    s = orig[:n].copy()
    getattr(HostVec(ctx, s), op)(s)                                    # other is self
    assert bits_equal(s, getattr(oracle, op)(orig[:n], orig[:n]))


@gpu
@pytest.mark.parametrize("n", [3001, 40000])
@pytest.mark.parametrize("op", BINARY)
def test_vec_op_refusal_leaves_self_unchanged(ctx, op, n):
    a, b = (v[:n + 1] for v in _operands())
    for other in (b[:n - 1], b[:n + 1]):
        h = a[:n].copy()
        with pytest.raises(ap.LengthMismatch, match="Vectors must have same length"):
            getattr(HostVec(ctx, h), op)(other)
        assert bits_equal(h, a[:n])


@gpu
@pytest.mark.parametrize("op", UNARY + BINARY)
def test_vec_op_on_an_empty_slice_is_a_no_op(ctx, op):
    buf = np.full(2, GUARD, np.complex64)
    _host_op(ctx, op, buf[1:1], np.empty(0, np.complex64))
    assert bits_equal(buf, np.full(2, GUARD))


# ---- 2. the staging slots ------------------------------------------------------------------------------------------------
def _mul_against_oracle(c, oracle, n):
    a, b = (v[:n] for v in _operands())
    h = a.copy()
    HostVec(c, h).vec_mul(b)
    assert bits_equal(h, oracle.vec_mul(a, b)), n


@gpu
def test_staging_slots_regrow_shrink_and_trim(oracle, ctx):
    """a context of its own: its bounce buffers and slots are allocated by these calls.  40000 allocates the slots
    (50000 samples with the slack), 3001 is back on the pinned path, 120000 regrows both, 40001 is smaller than the slot,
    trim gives everything back, 32768 is the largest pinned size"""
    del ctx                                                            # only here so that a CPU machine skips
    c = ap.Context(0)
    try:
        for n in (40000, 3001, 120000, 40001):
            _mul_against_oracle(c, oracle, n)
        c.trim()
        for n in (40000, ZS):
            _mul_against_oracle(c, oracle, n)
    finally:
        c.close()


@gpu
def test_host_slice_calls_behind_unsynced_device_work(oracle, ctx):
    del ctx
    a, b = (v[:NMAX] for v in _operands())
    c = ap.Context(0)
    try:
        for n in (3001, 40000):                                        # pinned, staged
            da, db = c.vec(a), c.vec(b)
            h = a[:n].copy()
            da.vec_add(db)                                             # in flight: nothing waits for it ...
            HostVec(c, h).vec_mul(b[:n])                               # ... before the host-slice call starts
            assert bits_equal(h, oracle.vec_mul(a[:n], b[:n])), n
            assert bits_equal(da.to_host(), oracle.vec_add(a, b)), n
            assert bits_equal(db.to_host(), b)
    finally:
        c.close()


@gpu
def test_host_slice_calls_behind_the_overlap_lane(oracle, ctx):
    """two FIR launches side by side on the two queues, then a host-slice call on each path: the call joins the lane"""
    del ctx
    taps = oracle.synth_lowpass_taps(64, 0.25)
    n = 1 << 16
    xs = [rand_c64(4110 + i, n) for i in range(2)]
    a = _operands()[0]
    plain, ov = ap.Context(0), ap.Context(0)
    try:
        f = Fir(plain, taps, 2048)
        want = [f.filter(plain.vec(x)).to_host() for x in xs]
        ov.set_overlap(True)
        assert ov.overlap
        f = Fir(ov, taps, 2048)
        ins = [ov.vec(x) for x in xs]
        outs = [ov.empty(n) for _ in xs]
        h1, h2 = a[:3001].copy(), a[:40000].copy()
        f.filter(ins[0], out=outs[0])
        f.filter(ins[1], out=outs[1])                                  # no hazard with the first: beside it
        HostVec(ov, h1).vec_conj()
        HostVec(ov, h2).vec_conj()
        ov.sync()
        assert bits_equal(h1, oracle.vec_conj(a[:3001])) and bits_equal(h2, oracle.vec_conj(a[:40000]))
        for got, exp in zip(outs, want):
            assert bits_equal(got.to_host(), exp)
    finally:
        ov.close()
        plain.close()


# ---- 3. interpolate ------------------------------------------------------------------------------------------------------
# n_src, n_between -> Lo = n + (n - 1) * nb
INTERP = [(1, 5),              # Lo = 1       pinned
          (2, 0),              # Lo = 2       pinned
          (4681, 6),           # Lo = 32761   pinned
          (2, ZS - 2),         # Lo = 32768   pinned, dst exactly at the limit
          (2, ZS - 1),         # Lo = 32769   staged because of dst alone (src is 16 bytes)
          (4097, 7),           # Lo = 32769   staged
          (40000, 1)]          # Lo = 79999   staged, src above the limit too


@gpu
@pytest.mark.parametrize("compat", [True, False])
@pytest.mark.parametrize("n_src,nb", INTERP)
def test_interpolate_host_both_paths(ctx, oracle, n_src, nb, compat):
    src = _operands()[0][:n_src]
    Lo = n_src + (n_src - 1) * nb
    sentinel = 4 - 9j
    dst = [sentinel]                                                   # the reference APPENDS (sampling.rs:17,23)
    assert sampling.interpolate(ctx, src.copy(), dst, nb, compat_im=compat) == Lo
    assert len(dst) == Lo + 1 and dst[0] == sentinel
    assert bits_equal(np.array(dst[1:], np.complex64), oracle.interpolate(src, nb, compat_im=compat))


def _host_interpolate(ctx, src, dst, cap, nb):
    nw = C.c_size_t(77)
    rc = _lib.load().aeth_host_interpolate(ctx.h, src.ctypes.data_as(C.c_void_p), src.size, dst.ctypes.data_as(C.c_void_p),
                                           cap, nb, 1, C.byref(nw))
    return rc, nw.value


@gpu
@pytest.mark.parametrize("n_src,nb", [(4681, 6), (4097, 7)])           # pinned, staged
def test_interpolate_host_capacity(ctx, oracle, n_src, nb):
    src = _operands()[0][:n_src].copy()
    Lo = n_src + (n_src - 1) * nb
    dst = np.full(Lo + 5, GUARD, np.complex64)
    rc, nw = _host_interpolate(ctx, src, dst, Lo + 5, nb)              # cap > Lo: nothing past Lo is written
    assert rc == 0 and nw == Lo
    assert bits_equal(dst[:Lo], oracle.interpolate(src, nb)) and bits_equal(dst[Lo:], np.full(5, GUARD))
    dst[:] = GUARD
    rc, nw = _host_interpolate(ctx, src, dst, Lo - 1, nb)              # cap < Lo: refused before anything moves
    assert nw == 0 and bits_equal(dst, np.full(Lo + 5, GUARD))
    with pytest.raises(ap.LengthMismatch):
        _lib.check(rc)


# ---- 4. downsample, every element size -----------------------------------------------------------------------------------
DTYPES = [np.uint8, np.int16, np.float32, np.float64, np.complex128]          # elem 1, 2, 4, 8, 16
# the smallest src above ZC bytes, ZC / elem + k elements, that some 1 < n_dst < n_src divides: (k, n_dst).  ZC / elem + 1 is
# 262145 = 5 * 52429, 131073 = 3 * 43691, 65537 (prime, so k = 2: 65538 = 2 * 32769), 32769 = 3 * 10923, 16385 = 5 * 3277
STAGED_EVEN = {1: (1, 52429), 2: (1, 43691), 4: (2, 32769), 8: (1, 10923), 16: (1, 3277)}
BOTH = (sampling.downsample, sampling.downsample_sb)


def _elems(dtype, n, seed=7):
    rng = np.random.default_rng(seed + n)
    return (rng.standard_normal(n) * 100).astype(dtype)


def _carve(dtype, n, fill=None):
    """n elements of dtype that start at byte offset 1 of a uint8 allocation"""
    e = np.dtype(dtype).itemsize
    raw = np.full(n * e + 2, 0xA5, np.uint8)
    v = raw[1:1 + n * e].view(dtype)
    if fill is not None:
        v[:] = fill
    assert v.ctypes.data % 2 == 1
    return raw, v


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_downsample_host_debug_build_both_paths(ctx, oracle, dtype):
    e = np.dtype(dtype).itemsize
    k, n_dst = STAGED_EVEN[e]
    for n_src, nd in ((ZC // e, ZC // e // 16),                        # a src of exactly ZC bytes: pinned
                      (ZC // e + k, n_dst)):                           # the smallest even decimation above it: staged
        src = _elems(dtype, n_src)
        exp = oracle.downsample(src, nd)
        for fn in BOTH:
            keep = src.copy()
            dst = np.zeros(nd, dtype)
            fn(ctx, src, dst)
            assert bytes_equal(dst, exp) and bytes_equal(src, keep), (fn.__name__, n_src)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_downsample_host_release_build_staged(ctx, oracle, dtype):
    e = np.dtype(dtype).itemsize
    n = ZC // e + 1
    src = _elems(dtype, n)
    for sb, fn in enumerate(BOTH):                                     # one element past the limit into 5: the ratio floors
        dst = np.zeros(5, dtype)
        fn(ctx, src, dst, release=True)
        assert bytes_equal(dst, oracle.downsample(src, 5, release=True, step_by=bool(sb)))
    # src shorter than dst: dec = 0 broadcasts src[0]; staged because of dst alone
    short = src[:3].copy()
    dst = np.zeros(n, dtype)
    sampling.downsample(ctx, short, dst, release=True)
    assert bytes_equal(dst, oracle.downsample(short, n, release=True))
    assert bytes_equal(dst, np.full(n, short[0], dtype))
    raw, d = _carve(dtype, n)                                          # downsample_sb panics there (step_by(0)), staged or not
    with pytest.raises(ap.LengthMismatch, match="step_by"):
        sampling.downsample_sb(ctx, short, d, release=True)
    assert (raw == 0xA5).all()


@gpu
@pytest.mark.parametrize("dtype", DTYPES[1:])                          # elem > 1
def test_downsample_host_takes_any_host_address(ctx, oracle, dtype):
    """src and dst start at an odd byte offset: the host entry points copy, so nothing asks for element alignment"""
    e = np.dtype(dtype).itemsize
    k, n_dst = STAGED_EVEN[e]
    for n_src, nd in ((6000, 300), (ZC // e + k, n_dst)):              # pinned, staged
        vals = _elems(dtype, n_src)
        _, src = _carve(dtype, n_src, vals)
        exp = oracle.downsample(vals, nd)
        for fn in BOTH:
            raw, dst = _carve(dtype, nd)
            fn(ctx, src, dst)
            assert bytes_equal(dst.copy(), exp), (fn.__name__, n_src)
            assert raw[0] == 0xA5 and raw[-1] == 0xA5
        assert bytes_equal(src.copy(), vals)


@gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_downsample_host_refusals_at_a_staged_size(ctx, dtype):
    e = np.dtype(dtype).itemsize
    src = _elems(dtype, ZC // e + 1)                                   # an odd count
    for fn in BOTH:
        raw, dst = _carve(dtype, 2)
        with pytest.raises(ap.LengthMismatch, match="Only even decimations are supported"):
            fn(ctx, src, dst)                                          # the debug build: uneven sizes panic
        assert (raw == 0xA5).all()
        for release in (False, True):
            with pytest.raises(ap.LengthMismatch):
                fn(ctx, src, raw[1:1].view(dtype), release=release)    # empty dst: division by zero in the reference
            assert (raw == 0xA5).all()


# ---- 5. FFT --------------------------------------------------------------------------------------------------------------
# length, algorithm, and for the chirp-z routes whether the plan runs in one launch or several (aeth_fft_route)
FFT_PINNED = [(1, "identity", None), (2, "stockham_pow2", None), (4096, "stockham_pow2", None),
              (FP, "stockham_mixed_ragged", None),                                             # exactly 64 KiB
              (29, "bluestein", "one"), (263, "bluestein", "one"), (1031, "bluestein", "one"),
              (578, "bluestein", "one"), (437, "bluestein", "one"),
              (4099, "bluestein", "multi"),                                                    # too long for the one-launch kernel
              (1331, "stockham_mixed", None), (4114, "stockham_mixed", None),
              (323, "stockham_mixed_ragged", None), (1700, "stockham_mixed_ragged", None),     # register radix 17 and 19
              (1000, "stockham_mixed_ragged", None), (6000, "stockham_mixed_ragged", None), (7500, "stockham_mixed_ragged", None),
              (8190, "stockham_mixed", None)]                                                  # LDS ping-pong
FFT_STAGED = [(8232, "fourstep_mixed", None),                                                  # 40 points over the limit
              (10000, "stockham_mixed_ragged", None), (16384, "stockham_mixed_ragged", None),
              (10007, "bluestein", "multi"),                                                   # odd: tmp_dev + len is only 8-byte aligned
              (20014, "bluestein", "multi"), (30000, "fourstep_mixed", None), (32768, "fourstep_pow2", None)]


@gpu
@pytest.mark.parametrize("n,algo,launches", FFT_PINNED + FFT_STAGED)
def test_fft_host_flavours_are_the_device_flavour(ctx, oracle, n, algo, launches):
    """fwd / ifwd / tfwd / vec_fft on host slices (and bwd / ibwd / tbwd / vec_ifft): the bits of exec on device vectors"""
    f = HipFft(ctx, n)
    assert f.algorithm == algo, f.route
    if launches:
        assert f"({launches} launch" in f.route, f.route
    x = rand_c64(5000 + n, n)
    for sign in (+1, -1):
        oop, inpl, tmp = (f.fwd, f.ifwd, f.tfwd) if sign > 0 else (f.bwd, f.ibwd, f.tbwd)
        for s in (Scale.NONE, Scale.SN):
            ref = f.exec(ctx.vec(x), ctx.empty(n), sign, s).to_host()
            inp, out = x.copy(), np.zeros(n, np.complex64)
            oop(inp, out, s)
            assert bits_equal(inp, x), (sign, s)
            assert bits_equal(out, ref), (sign, s)
            io = x.copy(); inpl(io, s)
            assert bits_equal(io, ref), (sign, s)
            assert bits_equal(np.array(tmp(x, s)), ref), (sign, s)
            h = HostVec(ctx, x.copy())
            (h.vec_fft if sign > 0 else h.vec_ifft)(s)
            assert bits_equal(h.a, ref), (sign, s)
            _check(oracle, out, x, n, sign, s.factor(n))


@gpu
@pytest.mark.parametrize("n", [2048, 10000])                           # pinned, staged
def test_fft_lent_view_survives_other_host_slice_calls(ctx, oracle, n):
    """the view tfwd lends is the plan's own pinned temp: only a call on THAT plan may reuse it"""
    s = Scale.SN
    x, y = rand_c64(5100 + n, n), rand_c64(5200 + n, n)
    f, g = HipFft(ctx, n), HipFft(ctx, n)
    want_x = f.exec(ctx.vec(x), ctx.empty(n), +1, s).to_host()
    want_y = f.exec(ctx.vec(y), ctx.empty(n), +1, s).to_host()
    v = f.tfwd(x, s)
    assert bits_equal(np.array(v), want_x)
    _mul_against_oracle(ctx, oracle, 3001)
    out = np.zeros(n, np.complex64)
    g.fwd(y, out, s)
    assert bits_equal(out, want_y)
    dst = []
    sampling.interpolate(ctx, x[:500], dst, 3)
    assert bits_equal(np.array(dst, np.complex64), oracle.interpolate(x[:500], 3))
    assert bits_equal(np.array(v), want_x)                             # still the first result
    w = f.tfwd(y, s)
    assert bits_equal(np.array(w), want_y)


@gpu
def test_one_shot_vec_fft_on_host_slices_through_plan_eviction(ctx):
    lengths = (100, 128, 10000, 2048, 8232, 17, 1000, 16384, 960, 4099)
    assert len(set(lengths)) > FFT_CACHE_MAX and any(n > FP for n in lengths) and any(n <= FP for n in lengths)
    for n in lengths + lengths[:1]:                                    # the first length again: its plan has been evicted
        x = rand_c64(5300 + n, n)
        d = ctx.vec(x); HipFft(ctx, n).ifwd(d, Scale.SN)
        h = HostVec(ctx, x.copy()); h.vec_fft(Scale.SN)
        assert bits_equal(h.a, d.to_host()), n


# ---- 6. stats, FIR, sequences: the limit itself --------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("n", [ZS, ZS + 1])
def test_stats_at_the_limit(ctx, n):
    x = _operands()[0][:n].copy()
    assert HostVec(ctx, x).stats().raw == ctx.vec(x).stats().raw


@gpu
@pytest.mark.parametrize("n", [ZS, ZS + 1])
def test_fir_host_at_the_limit(ctx, oracle, n):
    taps = oracle.synth_lowpass_taps(64, 0.25)
    f = Fir(ctx, taps, 2048)
    a, b = _operands()
    x, hist = a[:n].copy(), b[:f.ntaps - 1].copy()
    assert bits_equal(f.filter(x), f.filter(ctx.vec(x)).to_host())
    assert bits_equal(f.filter(x, hist=hist), f.filter(ctx.vec(x), hist=ctx.vec(hist)).to_host())


@gpu
@pytest.mark.parametrize("n", [ZC, ZC + 1])                            # output bytes
def test_seq_bits_host_at_the_limit(ctx, n):
    seq = ap.Sequence(ctx, (28, 31), (28, 29, 30, 31))
    init = (1, 0x12345)
    host = seq.bits(init, n, skip=1600, host=True)
    assert host.size == n and (host == seq.bits(init, n, skip=1600).to_host()).all()


# ---- 7. CPU: the limits this file assumes are the library's --------------------------------------------------------------
def _shifted_constant(path, name):
    text = open(os.path.join(CSRC, path)).read()
    m = re.search(r"constexpr\s+size_t\s+" + name + r"\s*=\s*\(size_t\)\s*(\d+)\s*<<\s*(\d+)\s*;", text)
    assert m, f"{name} is no longer written as (size_t)A << B in {path}"
    return int(m.group(1)) << int(m.group(2))


def test_the_limits_are_the_librarys():
    """If a limit moves, move ZC / FZC and with them every boundary shape above (they are all written relative to the two)"""
    assert _shifted_constant("aeth_internal.h", "kZeroCopyMax") == ZC == 256 << 10
    assert _shifted_constant("aeth_fft.hip", "kFftZeroCopyMax") == FZC == 64 << 10
    fft = open(os.path.join(CSRC, "aeth_fft.hip")).read()
    assert re.search(r"kFftCacheMax\s*=\s*%d\b" % FFT_CACHE_MAX, fft)
    # both comparisons are inclusive: a buffer of exactly the limit stays pinned
    moved = "the comparison with the limit changed: the cases at exactly ZC / FZC no longer run the pinned path"
    assert "bytes0 <= kZeroCopyMax && bytes1 <= kZeroCopyMax" in open(os.path.join(CSRC, "aeth_runtime.hip")).read(), moved
    assert fft.count("bytes <= kFftZeroCopyMax") == 2, moved
    # ... and the shapes sit on the sides their comments name
    assert [n + (n - 1) * nb for n, nb in INTERP] == [1, 2, ZS - 7, ZS, ZS + 1, ZS + 1, 79999]
    assert all(n * 8 <= FZC for n, _, _ in FFT_PINNED) and all(n * 8 > FZC for n, _, _ in FFT_STAGED)
    assert max(n for n, _, _ in FFT_PINNED) == FP

    def has_proper_divisor(m):
        return any(m % d == 0 for d in range(2, int(m ** 0.5) + 1))
    for e, (k, n_dst) in STAGED_EVEN.items():
        n = ZC // e + k
        assert n * e > ZC and n % n_dst == 0 and 1 < n_dst < n
        assert not any(has_proper_divisor(ZC // e + j) for j in range(1, k))
