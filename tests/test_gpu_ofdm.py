"""GPU: the OFDM calls (aeth_ofdm_*, csrc/aeth_ofdm.hip).

1. the fused demod equals, byte for byte, the chain of existing calls: windows sliced on the host and uploaded
   contiguously, aeth_fft_exec, bins picked on the host, aeth_vec_mul_frames by the same eq;
2. the fused mod equals the host-placed grid, aeth_fft_exec with the backward sign and the host-made prefix;
3. the object created with general=True gives the same bytes, the general-only lengths equal the chain as well, and
   `route` says which is which;
4. the aggregate EVM against the complex128 restatement (tests/ofdm_truth.py) is within -80 dB, the figure of assert_evm's
   default (the macro itself compares every element at 10^(-80/10) = 1e-8 of its magnitude, below f32's own rounding, so
   it is the 20 log10 ratio of the error's to the truth's norm that is bounded; the figures are printed);
5. estimate equals estimate_truth bit for bit (a NaN equals any NaN: IEEE 754 leaves its sign and payload open);
6. calls over halves of the symbols, sentinels around the output, overlapping ranges, repeated calls, aeth_ctx_trim and
   both cache policies.

Shapes: every fused length, G in {0, 1, N/4, N}, n_sym in {1, 2, F-1, F, F+1, 3F+2} with F the symbols per workgroup, five
carrier sets, both 8-byte parities of every sample pointer (views one sample into an allocation), with and without eq,
all four Scale kinds -- every value of each, rotated against the others rather than fully crossed."""
import itertools
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
from aether_primitives_amd import Ofdm, Scale         # noqa: E402
from aether_primitives_amd.ofdm import EQ_KINDS       # noqa: E402
import ofdm_truth as ot                               # noqa: E402

pytestmark = pytest.mark.gpu

FUSED = (64, 128, 256, 512, 1024, 2048, 4096)
GENERAL_ONLY = (12, 600, 1536, 8192)
FRAMES = {64: 8, 128: 8, 256: 4}                      # symbols per workgroup (CfgFor<N>::F); 1 from 512 up
SCALES = (Scale.NONE, Scale.SN, Scale.N, Scale.X(0.37))
SENT = np.complex64(complex(-7.25, 1234.5))
PAD = 6


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def signal(n, seed):
    r = np.random.default_rng(seed)
    return ((r.standard_normal(n) + 1j * r.standard_normal(n)) * 0.7).astype(np.complex64)


def n_syms(n):
    f = FRAMES.get(n, 1)
    return sorted({s for s in (1, 2, f - 1, f, f + 1, 3 * f + 2) if s > 0})


def carrier_sets(n):
    k = 3 * n // 4
    occ = np.array(list(range(n - k // 2, n)) + list(range(1, k // 2 + 1)))
    r = np.random.default_rng(n)
    rnd = r.permutation(n)[: max(1, n // 3 + 1)]
    return [np.arange(n), occ, occ[::-1].copy(), np.array([n // 2 + 1]), rnd]


def shapes(n):
    """(G, n_sym, carrier set index): G x n_sym with the sets rotated, then every set at two more shapes"""
    gs = sorted({0, 1, n // 4, n})
    out = [(g, s, i % 5) for i, (g, s) in enumerate(itertools.product(gs, n_syms(n)))]
    f = FRAMES.get(n, 1)
    out += [(n // 4, f + 1, c) for c in range(5)] + [(1, 3 * f + 2, c) for c in range(5)]
    return list(dict.fromkeys(out))


class Dev:
    """n samples on the device, PAD + off samples into an allocation filled with a sentinel"""

    def __init__(self, ctx, n, off, data=None):
        self.n, self.off = n, PAD + off
        host = np.full(n + 2 * PAD + 1, SENT, np.complex64)
        if data is not None:
            host[self.off: self.off + n] = data
        self.all = ctx.vec(host)
        self.v = self.all.slice(self.off, self.off + n)

    def get(self):
        """the n samples; the sentinels around them have to be intact"""
        h = self.all.to_host()
        sent = np.array([SENT]).view(np.uint64)[0]
        assert (h[: self.off].view(np.uint64) == sent).all(), "wrote in front of the output"
        assert (h[self.off + self.n:].view(np.uint64) == sent).all(), "wrote behind the output"
        return h[self.off: self.off + self.n].copy()


_PLANS = {}


def plan(ctx, n):
    if n not in _PLANS:
        _PLANS[n] = ap.HipFft(ctx, n)
    return _PLANS[n]


def chain_demod(ctx, x, n, g, bins_, n_sym, eq, scale):
    """the existing calls: host windows -> aeth_fft_exec -> host pick -> aeth_vec_mul_frames"""
    w = ctx.vec(ot.windows(x, n, g, n_sym).reshape(-1))
    plan(ctx, n).fwd(w, w, scale)
    picked = w.to_host().reshape(n_sym, n)[:, bins_].reshape(-1)
    if eq is None:
        return picked
    d = ctx.vec(picked)
    d.vec_mul_frames(ctx.vec(eq), len(bins_))
    return d.to_host()


def chain_mod(ctx, car, n, g, bins_, n_sym, scale):
    """host-placed grid (zeros included) -> aeth_fft_exec with the backward sign -> host-made prefix"""
    d = ctx.vec(ot.grid(car, n, bins_, n_sym).reshape(-1))
    plan(ctx, n).bwd(d, d, scale)
    return ot.add_prefix(d.to_host().reshape(n_sym, n), g)


def scale_of(s, n):
    return float(s.factor(n))


def run_shape(ctx, n, g, n_sym, bins_, i, evms, bad, general_only=False):
    """one shape through both routes; mismatches are collected in `bad` so that one run reports them all"""
    k, L = len(bins_), n + g
    scale = SCALES[(i + i // 4) % 4]                      # rotated against the pointer parities (i & 1, i >> 1 & 1)
    fused = None if general_only else Ofdm(ctx, n, g, bins_)
    general = Ofdm(ctx, n, g, bins_, max_symbols=(n_sym if (i // 3) % 2 else 0), general=not general_only)
    if fused is not None:
        assert fused.route == "fused", fused.route
    assert general.route.startswith("general: ") and general.route[9:] == plan(ctx, n).route, general.route
    for o in (fused, general):
        if o is not None:
            assert (o.len, o.cp, o.symbol, o.carriers) == (n, g, L, k)
            assert [o.span(s) for s in (0, 1, 3)] == [0, n, 2 * L + n]
    span = (n_sym - 1) * L + n
    x = signal(span, 1000 * n + i)
    eq = signal(k, 7 + i)
    what = f"N={n} G={g} n_sym={n_sym} K={k} bins={bins_[:3]}.. scale={scale} case {i}"
    # ---- demod ----
    xin = Dev(ctx, span, i & 1, x)
    for e in (None, eq):
        want = chain_demod(ctx, x, n, g, bins_, n_sym, e, scale)
        got = {}
        for name, o in (("fused", fused), ("general", general)):
            if o is None:
                continue
            out = Dev(ctx, n_sym * k, (i >> 1) & 1)
            o.demod(xin.v, n_sym, eq=e, scale=scale, out=out.v)
            got[name] = out.get()
            if not same(got[name], want):
                bad.append(f"demod {name} != chain: {what} eq={e is not None}")
        truth = ot.demod_truth(x, n, g, bins_, n_sym, e, scale_of(scale, n)).reshape(-1)
        evms.append(ap.evm_db(next(iter(got.values())), truth))
    # ---- mod ----
    car = signal(n_sym * k, 2000 * n + i)
    cin = Dev(ctx, n_sym * k, (i >> 1) & 1, car)
    want = chain_mod(ctx, car, n, g, bins_, n_sym, scale)
    for name, o in (("fused", fused), ("general", general)):
        if o is None:
            continue
        out = Dev(ctx, n_sym * L, i & 1)
        o.mod(cin.v, n_sym, scale=scale, out=out.v)
        got = out.get()
        if not same(got, want):
            bad.append(f"mod {name} != chain: {what}")
    evms.append(ap.evm_db(got, ot.mod_truth(car, n, g, bins_, n_sym, scale_of(scale, n))))
    for o in (fused, general):
        if o is not None:
            o.close()


@pytest.mark.parametrize("n", FUSED)
def test_fused_equals_the_chain_and_the_general_route(ctx, n):
    evms, bad = [], []
    sets = carrier_sets(n)
    for i, (g, n_sym, c) in enumerate(shapes(n)):
        run_shape(ctx, n, g, n_sym, sets[c], i, evms, bad)
    print(f"N={n}: {len(evms)} EVMs against f64 truth, worst {max(evms):.1f} dB")
    assert not bad, (len(bad), bad[:6])
    assert max(evms) <= -80.0


@pytest.mark.parametrize("n", GENERAL_ONLY)
def test_general_only_lengths_equal_the_chain(ctx, n):
    evms, bad = [], []
    r = np.random.default_rng(n)
    sets = [np.arange(n), r.permutation(n)[: max(1, (3 * n) // 4)], np.array([n - 1])]
    for i, (g, n_sym) in enumerate([(0, 1), (n // 4, 3), (n, 2), (1, 5)]):
        run_shape(ctx, n, g, n_sym, sets[i % 3], i, evms, bad, general_only=True)
    print(f"N={n} (general): worst EVM {max(evms):.1f} dB")
    assert not bad, (len(bad), bad[:6])
    assert max(evms) <= -80.0


def test_more_symbols_than_the_resident_grid(ctx):
    """the fused kernel launches at most 8 workgroups per CU and walks the rest: 256 CUs on an MI355X"""
    n, g = 512, 128
    n_sym = 256 * 8 + 3
    bins_ = carrier_sets(n)[1]
    k, L = len(bins_), n + g
    x = signal((n_sym - 1) * L + n, 99)
    eq = signal(k, 98)
    o = Ofdm(ctx, n, g, bins_)
    got = o.demod(ctx.vec(x), n_sym, eq=eq, scale=Scale.SN).to_host()
    assert same(got, chain_demod(ctx, x, n, g, bins_, n_sym, eq, Scale.SN))
    car = signal(n_sym * k, 97)
    got = o.mod(ctx.vec(car), n_sym, scale=Scale.N).to_host()
    assert same(got, chain_mod(ctx, car, n, g, bins_, n_sym, Scale.N))


def test_mod_then_demod_returns_the_carriers(ctx):
    n, g = 256, 64
    bins_ = carrier_sets(n)[4]
    o = Ofdm(ctx, n, g, bins_)
    car = signal(9 * len(bins_), 5)
    t = o.mod(ctx.vec(car), 9, scale=Scale.N)
    back = o.demod(t.slice(g, t.n), 9).to_host()
    assert ap.evm_db(back, car) <= -120.0


# ---- 5: estimate ---------------------------------------------------------------------------------------------------------
def same_or_nan(got, want):
    g, w = np.ascontiguousarray(got).view(np.float32), np.ascontiguousarray(want).view(np.float32)
    both_nan = np.isnan(g) & np.isnan(w)
    return g.shape == w.shape and bool(((g.view(np.uint32) == w.view(np.uint32)) | both_nan).all())


def training(k, n_sym, x_sym, seed):
    y, x = signal(n_sym * k, seed).reshape(n_sym, k), signal(x_sym * k, seed + 1).reshape(x_sym, k)
    if k >= 52:
        sp = np.array([0.0, -0.0, 1e-40, -1e-42, 3e19, -3e19, np.inf, -np.inf, np.nan], np.float32)
        for j, v in enumerate(sp):                          # carriers 0 .. 8: the special value in y, 9 .. 17: in x
            y.real[:, j] = v
            y.imag[-1, j] = -v
            x.imag[:, 9 + j] = v
            x.real[0, 9 + j] = -v
        x[:, 20] = 0                                        # all-zero training
        x[:, 21] = np.complex64(complex(0.0, -0.0))
        y[:, 22] = 0                                        # a dead carrier: H = 0
        x[:, 23], y[:, 23] = np.complex64(3e19 + 3e19j), np.complex64(3e19 - 1e19j)     # squares overflow f32, not f64
    return y, x


@pytest.mark.parametrize("k,n", [(1, 64), (52, 64), (1200, 2048)])
def test_estimate_equals_the_definition_bit_for_bit(ctx, k, n):
    bins_ = np.arange(1, k + 1) if k > 1 else np.array([5])
    o = Ofdm(ctx, n, n // 4, bins_, general=(k == 52))       # the estimator does not care about the route
    count = 0
    for n_sym, one_x in itertools.product((1, 2, 7), (True, False)):
        x_sym = 1 if one_x else n_sym
        y, x = training(k, n_sym, x_sym, 31 * n_sym + k)
        yd, xd = ctx.vec(y.reshape(-1)), ctx.vec(x.reshape(-1))
        for kind, nv in itertools.product(("zf", "mmse", "matched"), (0.0, 0.1)):
            hw, ww, cw = ot.estimate_truth(y, x, n_sym, x_sym, k, nv, EQ_KINDS[kind])
            h, w, csi = o.estimate(yd, xd, nv=nv, kind=kind)
            what = f"K={k} n_sym={n_sym} x_sym={x_sym} {kind} nv={nv}"
            assert same_or_nan(h.to_host(), hw), "h " + what
            assert same_or_nan(w.to_host(), ww), "eq " + what
            assert same_or_nan(csi.to_host(), cw), "csi " + what
            count += 1
        # any one or two of the outputs absent: the others are the same bytes
        hw, ww, cw = ot.estimate_truth(y, x, n_sym, x_sym, k, 0.1, ot.MMSE)
        for mask in range(1, 7):
            bufs = [ap.DeviceVec(ctx, k) if mask & 1 else None, ap.DeviceVec(ctx, k) if mask & 2 else None,
                    ap.DeviceF32(ctx, k) if mask & 4 else None]
            o.estimate_into(yd, xd, n_sym, 0.1, "mmse", *bufs)
            for b, want in zip(bufs, (hw, ww, cw)):
                assert b is None or same_or_nan(b.to_host(), want), (mask, k, n_sym, x_sym)
    assert count == 36
    with pytest.raises(ap.AetherError):
        o.estimate_into(yd, xd, 7, 0.0, "zf", None, None, None)


# ---- 6: streams and hygiene --------------------------------------------------------------------------------------------
HYG = [(64, 16, 19), (256, 1, 9), (1024, 256, 5), (600, 150, 4)]


def repro_calls(ctx):
    """demod (with eq) and mod at a few shapes -> the bytes of all outputs"""
    b = b""
    for n, g, n_sym in HYG:
        bins_ = np.random.default_rng(n + 1).permutation(n)[: (3 * n) // 4]
        k, L = len(bins_), n + g
        o = Ofdm(ctx, n, g, bins_)
        x, eq, car = signal((n_sym - 1) * L + n, n), signal(k, n + 2), signal(n_sym * k, n + 3)
        b += o.demod(ctx.vec(x), n_sym, eq=eq, scale=Scale.SN).to_host().tobytes()
        b += o.mod(ctx.vec(car), n_sym, scale=Scale.SN).to_host().tobytes()
        o.close()
    return b


def test_same_bytes_twice_and_after_trim(ctx):
    a = repro_calls(ctx)
    assert repro_calls(ctx) == a, "the same calls gave other bytes"
    ctx.trim()
    assert repro_calls(ctx) == a


def _child(outdir):
    ctx = ap.Context(0)
    for nt in ("0", "1"):
        os.environ["AETH_NT"] = nt
        with open(os.path.join(outdir, f"nt{nt}.bin"), "wb") as f:
            f.write(repro_calls(ctx))
    ctx.close()
    print("ofdm child ok")


def test_bytes_do_not_depend_on_the_cache_policy(ctx, tmp_path):
    """AETH_TUNING=1 with AETH_NT=0 and AETH_NT=1 in a fresh child process: the bytes of this process"""
    env = dict(os.environ, AETH_TUNING="1")
    env.pop("AETH_NT", None)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child", str(tmp_path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    want = repro_calls(ctx)
    for nt in ("0", "1"):
        assert open(tmp_path / f"nt{nt}.bin", "rb").read() == want, f"AETH_NT={nt} changed the bytes"


@pytest.mark.parametrize("n,g,n_sym", HYG)
def test_two_calls_over_halves_equal_one(ctx, n, g, n_sym):
    bins_ = carrier_sets(n)[1] if n != 600 else np.arange(10, 400)
    k, L = len(bins_), n + g
    o = Ofdm(ctx, n, g, bins_)
    x, eq, car = signal((n_sym - 1) * L + n, 3), signal(k, 4), signal(n_sym * k, 5)
    h = n_sym // 2
    xd, cd = ctx.vec(x), ctx.vec(car)
    whole = o.demod(xd, n_sym, eq=eq).to_host()
    out = Dev(ctx, n_sym * k, 1)
    o.demod(xd.slice(0, o.span(h)), h, eq=eq, out=out.v.slice(0, h * k))
    o.demod(xd.slice(h * L, xd.n), n_sym - h, eq=eq, out=out.v.slice(h * k, n_sym * k))
    assert same(out.get(), whole)
    whole = o.mod(cd, n_sym).to_host()
    out = Dev(ctx, n_sym * L, 0)
    o.mod(cd.slice(0, h * k), h, out=out.v.slice(0, h * L))
    o.mod(cd.slice(h * k, n_sym * k), n_sym - h, out=out.v.slice(h * L, n_sym * L))
    assert same(out.get(), whole)
    # sentinels right around ONE symbol: in front of its prefix and behind its tail
    out = Dev(ctx, L, 1)
    o.mod(cd.slice(0, k), 1, out=out.v)
    assert same(out.get(), whole[:L])


def test_overlapping_ranges_and_bounds_are_refused_on_a_real_object(ctx):
    n, g = 128, 32
    o = Ofdm(ctx, n, g, np.arange(1, 97), max_symbols=4)
    L, k = n + g, 96
    buf = ctx.vec(signal(8 * L, 1))
    with pytest.raises(ap.AetherError, match="overlap"):
        o.demod(buf, 2, out=buf.slice(L, L + 2 * k))
    with pytest.raises(ap.AetherError, match="overlap"):
        o.mod(buf.slice(0, 2 * k), 2, out=buf.slice(k, k + 2 * L))
    with pytest.raises(ap.AetherError, match="5 symbols"):
        o.demod(buf, 5)
    with pytest.raises(ap.LengthMismatch):
        o.demod(buf.slice(0, o.span(3) - 1), 3)
    assert o.demod(buf, 0).n == 0 and o.mod(ctx.empty(0), 0).n == 0


if __name__ == "__main__" and len(sys.argv) > 2 and sys.argv[1] == "--child":
    _child(sys.argv[2])
