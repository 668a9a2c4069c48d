"""GPU parity per kernel VARIANT, not per operation.

Most hot-path kernels are templates whose instantiation the host picks at run time: by size (the non-temporal `NT`
builds above 128 MiB), by alignment (float4 / float2 bodies), by frames per workgroup (`F > 1` for transforms of up to
256 points), by scale (the `SCALED` build of the fused FFT*H*IFFT kernel), by store kind (plain, decimating,
demodulating: BPSK, separable QPSK, any other table), by prefetch form (`V_SPREAD`) and by the overlap lane's grid.
Each is its own machine code.  The tests here reach them on purpose:

  * the fused correlator chain at every power of two 2 ... 4096, batches around F, four scale pairs: f64 truth, the
    three unfused calls, and a guard band on both sides;
  * the fused correlate + demod for every store kind, scale form and compat mode: the bits of mul_chain + demod_naive;
  * the decimating FIR at fft_len 1024 and 4096 (2048: tests/test_gpu_fir.py): the bits of filter + downsample;
  * the one-launch chirp-z transform with an Inf in every odd frame: the even frames stay finite and exact;
  * a fixed battery run in ONE child process under AETH_TUNING=1 with the shipped knobs forced (AETH_NT=0 / 1,
    AETH_FIR_SPREAD=0 / 1, AETH_FIR_GRID_FIRST / _CHAINED = 1 / 32): every forced form gives the bits of the default
    form in this process, and the default form meets its oracle.

tools/variant_coverage.py lists which instantiations of the library a run of the suite dispatched
(profiles/r05_variant_coverage_*.txt)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import aether_primitives_amd as ap                                        # noqa: E402
from aether_primitives_amd import Fir, HipFft, Scale, modulation, noise, sampling  # noqa: E402
from helpers import bits_equal, rand_c64                                   # noqa: E402

pytestmark = pytest.mark.gpu
TOL_DB = -120.0
GUARD = 7 - 7j

# frames per workgroup of the fused kernel (aeth_fft_core.h: CfgFor -> Cfg::F = WG / T)
FRAMES_PER_WG = {2: 64, 4: 64, 8: 64, 16: 64, 32: 16, 64: 8, 128: 8, 256: 4, 512: 1, 1024: 1, 2048: 1, 4096: 1}
SCALE_PAIRS = [(Scale.NONE, Scale.NONE), (Scale.SN, Scale.SN), (Scale.NONE, Scale.N), (Scale.X(0.37), Scale.X(2.5))]


def chain_truth(orc, x, sig, n, s_fwd, s_bwd):
    """bwd_f64(fwd_f64(x) * s_fwd * sig) * s_bwd per frame (the sign conventions of oracle.correlate_frames)"""
    b = x.size // n
    X = orc.fft_f64_frames(x.astype(np.complex128), n, ap.SIGN_REF_FWD).reshape(b, n)
    X *= float(s_fwd.factor(n))
    X *= sig.astype(np.complex128)
    return orc.fft_f64_frames(X.reshape(-1), n, ap.SIGN_REF_BWD) * float(s_bwd.factor(n))


def guarded(ctx, x, front, back):
    """x on the device with `front` / `back` guard samples around it: (whole buffer, view of x)"""
    buf = ctx.vec(np.concatenate([np.full(front, GUARD, np.complex64), x, np.full(back, GUARD, np.complex64)]))
    return buf, buf.slice(front, front + x.size)


def _batches(n):
    f = FRAMES_PER_WG[n]
    return sorted({1, max(f - 1, 2), f + 1, 301})


@pytest.mark.parametrize("n,batch", [(n, b) for n in FRAMES_PER_WG for b in _batches(n)])
def test_mul_chain_every_length_batch_and_scale(ctx, oracle, n, batch):
    """aeth_fft_mul_ifft at every fused length, batches that fill a last workgroup of F frames partly (the generic load
    path, aeth_fir_kernel.h: load_window with ov == 0), under each scale pair (the SCALED build beside the plain one):
    f64 truth, the unfused vec_rfft -> vec_mul -> vec_rifft per frame, and nothing outside the frames written"""
    x = rand_c64(n * 7 + batch, n * batch)
    sig = rand_c64(n + 3, n)
    f = HipFft(ctx, n, max_batch=batch)
    sigd = ctx.vec(sig)
    back = FRAMES_PER_WG[n] * n + 5                                  # a whole workgroup's frames past the end
    for s_fwd, s_bwd in SCALE_PAIRS:
        buf, d = guarded(ctx, x, 2, back)
        f.mul_chain(d, sigd, s_fwd, s_bwd)
        h = buf.to_host()
        got = h[2:2 + x.size]
        assert (h[:2] == GUARD).all() and (h[2 + x.size:] == GUARD).all(), (s_fwd, s_bwd, "wrote outside the frames")
        e = oracle.evm_db(got, chain_truth(oracle, x, sig, n, s_fwd, s_bwd))
        assert e <= TOL_DB, (s_fwd, s_bwd, e)
        u = ctx.vec(x)
        for k in range(batch):
            u.slice(k * n, (k + 1) * n).vec_rfft(f, s_fwd).vec_mul(sigd).vec_rifft(f, s_bwd)
        e = oracle.evm_db(got, u.to_host())
        assert e <= TOL_DB, (s_fwd, s_bwd, "against the unfused calls", e)


CUSTOM_QPSK = np.array([1 + 0j, 0 + 1j, 0 - 1j, -1 + 0j], np.complex64)          # rotated: not separable


def _demod_input(n, frames, seed):
    x = rand_c64(seed, n * frames, scale=1.5)
    x[::97] = 0                                                        # near-ties after the chain (see below)
    x[5] = complex(1.0, 1.0)
    x[7] = complex(-0.5, 0.5)
    return x


def _plant_ties(sym):
    """symbols on the decision boundaries, exactly: 0 (all candidates of every table), 1+1j and -0.5+0.5j (two of the
    rotated QPSK table's), 1j and -1 (BPSK's)"""
    sym = sym.copy()
    for k, v in enumerate((0, 1 + 1j, -0.5 + 0.5j, 1j, -1)):
        sym[k::61] = v
    return sym


@pytest.mark.parametrize("n", [1024, 2048, 4096])
@pytest.mark.parametrize("kind", ["bpsk", "qpsk", "qpsk_custom"])
def test_correlate_demod_every_store_kind(ctx, n, kind):
    """aeth_fft_mul_ifft_demod: every demodulating build (BPSK, separable QPSK, generic table) x scale (plain, (SN, SN),
    (X, X)) x compat: the bits of mul_chain + demod_naive, input untouched.  sig = 1/N everywhere returns the frames
    themselves up to rounding, so the values planted on the decision boundaries reach the decision as near-ties (the
    FFT round trip perturbs them; exact ties go through demod_naive in the battery below, against the oracle)"""
    frames = 5
    mod = {"bpsk": modulation.bpsk, "qpsk": modulation.qpsk}[kind](ctx) if kind != "qpsk_custom" else modulation.table(ctx, CUSTOM_QPSK)
    f = HipFft(ctx, n, max_batch=frames)
    x = _demod_input(n, frames, n + len(kind))
    ident = np.full(n, 1.0 / n, np.complex64)
    for sig in (ctx.vec(rand_c64(9, n)), ctx.vec(ident)):
        for s_fwd, s_bwd in ((Scale.NONE, Scale.NONE), (Scale.SN, Scale.SN), (Scale.X(0.37), Scale.X(2.5))):
            tx = ctx.vec(x)
            ref = ctx.vec(x); f.mul_chain(ref, sig, s_fwd, s_bwd)
            for compat in (True, False):
                want = mod.demod_naive(ref, compat=compat).to_host()
                got = mod.correlate_demod(f, tx, sig, s_fwd, s_bwd, compat=compat).to_host()
                assert (got == want).all(), (kind, s_fwd, s_bwd, compat, int((got != want).sum()))
            assert bits_equal(tx.to_host(), x)


@pytest.mark.parametrize("fft_len", [1024, 4096])
@pytest.mark.parametrize("dec", [2, 3, 16, 30])
@pytest.mark.parametrize("with_hist", [False, True])
def test_fir_decimating_store_other_lengths(ctx, oracle, fft_len, dec, with_hist):
    """aeth_fir_exec_decim at the other one-block-per-workgroup lengths: the bits of filter + sampling::downsample, with
    and without history, nothing written past the decimated output"""
    taps = oracle.synth_lowpass_taps(64, 0.25)
    n = (fft_len * 9 + 123) // dec * dec
    x = rand_c64(fft_len + dec, n)
    f = Fir(ctx, taps, fft_len)
    d = ctx.vec(x)
    hist = ctx.vec(rand_c64(dec, 63)) if with_hist else None
    full = f.filter(d, hist=hist)
    ref = ctx.empty(n // dec)
    sampling.downsample(ctx, full, ref)
    buf, out = guarded(ctx, np.zeros(n // dec, np.complex64), 0, 64)
    f.filter_decim(d, dec, out=out, hist=hist)
    h = buf.to_host()
    assert bits_equal(h[:n // dec], ref.to_host())
    assert (h[n // dec:] == GUARD).all()


def test_fir_decimating_store_refuses_short_windows(ctx, oracle):
    """fft_len 512 has no decimating build: the documented error, nothing launched"""
    f = Fir(ctx, oracle.synth_lowpass_taps(64, 0.25), 512)
    with pytest.raises(ap.AetherError, match="decimating store"):
        f.filter_decim(ctx.vec(rand_c64(1, 4096)), 4)


@pytest.mark.parametrize("n,frames_per_wg", [(29, 8), (97, 4), (263, 1), (1031, 1)])
def test_chirp_z_frames_stay_independent(ctx, oracle, n, frames_per_wg):
    """The one-launch chirp-z transform (fmi_bluestein) zero-pads each frame of n samples to M: nothing of the next
    frame may enter its window (the `e < frame_n` bound of the F > 1 load paths, the frame_n clamp of the F == 1 buffer
    descriptor).  For finite input the chirp's zero tail would hide such a read; an Inf at the first sample of every odd
    frame turns it into NaN.  Every even frame must stay finite and meet f64 truth, both directions.  F > 1: batch F + 2,
    so the last workgroup holds two frames (the generic load path) behind a full one (the chirp-z path)."""
    batch = frames_per_wg + 2 if frames_per_wg > 1 else 6
    x = rand_c64(n + 17, n * batch)
    x.reshape(batch, n)[1::2, 0] = np.inf
    f = HipFft(ctx, n, max_batch=batch)
    assert f.algorithm == "bluestein"
    even = x.reshape(batch, n)[0::2].reshape(-1).astype(np.complex128)
    for sign, call in ((ap.SIGN_REF_FWD, f.ifwd), (ap.SIGN_REF_BWD, f.ibwd)):
        d = ctx.vec(x)
        call(d, Scale.SN)
        got = d.to_host().reshape(batch, n)[0::2].reshape(-1)
        assert np.isfinite(got).all(), (sign, "a neighbouring frame leaked into an even frame")
        e = oracle.evm_db(got, oracle.fft_f64_frames(even, n, sign) / np.sqrt(n))
        assert e <= TOL_DB, (sign, e)


# ---- the forced-variant battery --------------------------------------------------------------------------------
# One fixed set of calls, run (i) in this process with the defaults and (ii) in one child process under AETH_TUNING=1
# with the shipped knobs forced.  Sizes stay at a few MiB: the NT builds are reached through AETH_NT=1.

N_EW = 4099                                   # odd: a head, a 16-byte body and a tail
OPS = ("scale", "mul", "div", "conj", "add", "sub", "clone", "zero", "mirror")
FFT_POW2 = (2, 16, 64, 256, 512, 1024, 2048, 4096, 8192)
# chirp-z: one length per convolution length M = 64 ... 4096 of the one-launch kernel (29, 37, 97, 131, 263, 601, 1031)
FFT_OTHER = ((1000, "stockham_mixed_ragged"), (1331, "stockham_mixed"), (32768, "fourstep_pow2"), (29, "bluestein"),
             (37, "bluestein"), (97, "bluestein"), (131, "bluestein"), (263, "bluestein"), (601, "bluestein"),
             (1031, "bluestein"))
MUL_CHAIN_LENS = tuple(FRAMES_PER_WG)
FIR_LENS = (16, 32, 64, 128, 256, 512, 1024, 2048, 4096)
DEMOD_KINDS = ("bpsk", "qpsk", "qpsk_custom")


def _ew_inputs():
    return rand_c64(11, N_EW + 2), rand_c64(12, N_EW + 2) + 0.5          # + 0.5: no division by a tiny number


def _vec_at(ctx, host, off, n):
    """host[off:off+n] on the device at element offset `off` of its allocation (off = 1: an odd 8-byte slot)"""
    return ctx.vec(host).slice(off, off + n)


def _fft_batch(n):
    """frames per FFT call of the battery: up to 64 Ki samples; three more for the short lengths, so that the last
    workgroup of several frames (pow2 kernel, one-launch chirp-z of 29 and 97 points) holds more than one frame"""
    return (max(3, min(64, (1 << 16) // n)) if n <= 8192 else 2) + (3 if n <= 256 else 0)


def _fir_taps(orc, fft_len):
    return orc.synth_lowpass_taps(min(64, fft_len // 2), 0.25)


def battery(ctx, orc):
    """[(key, result)] of every call of the battery, in a fixed order"""
    out = []
    a, b = _ew_inputs()
    # VecOps: self / other in phase at 16-byte and odd 8-byte slots, and out of phase (the float2-only path)
    for so, oo in ((0, 0), (1, 1), (0, 1)):
        for op in OPS:
            v = _vec_at(ctx, a, so, N_EW)
            o = _vec_at(ctx, b, oo, N_EW)
            {"scale": lambda: v.vec_scale(0.37), "mul": lambda: v.vec_mul(o), "div": lambda: v.vec_div(o),
             "conj": lambda: v.vec_conj(), "add": lambda: v.vec_add(o), "sub": lambda: v.vec_sub(o),
             "clone": lambda: v.vec_clone(o), "zero": lambda: v.vec_zero(), "mirror": lambda: v.vec_mirror()}[op]()
            out.append((f"ew_{op}_{so}{oo}", v.to_host()))
        # the fused chain, reading self and not (a leading clone)
        v = _vec_at(ctx, a, so, N_EW)
        o, p = _vec_at(ctx, b, oo, N_EW), _vec_at(ctx, a[::-1].copy(), oo, N_EW)
        v.fused().vec_add(o).vec_mul(p).vec_conj().vec_scale(0.5).vec_sub(o).vec_div(p).run()
        out.append((f"chain_{so}{oo}", v.to_host()))
        v = _vec_at(ctx, a, so, N_EW)
        v.fused().vec_clone(o).vec_mul(p).vec_add(o).run()
        out.append((f"chain_clone_{so}{oo}", v.to_host()))
    # frames: even frame length at a 16-byte slot (float4 path), odd frame length / odd slot (float2 path)
    for L, off in ((256, 0), (255, 0), (256, 1)):
        fr = _vec_at(ctx, a, off, L * 16)
        fr.vec_mul_frames(_vec_at(ctx, b, off, L), frame_len=L)
        out.append((f"mul_frames_{L}_{off}", fr.to_host()))
        fr = _vec_at(ctx, a, off, L * 16)
        fr.vec_mirror_frames(L)
        out.append((f"mirror_frames_{L}_{off}", fr.to_host()))
    # sampling
    for nb in (1, 4):
        d = ctx.empty(N_EW + (N_EW - 1) * nb)
        sampling.interpolate(ctx, ctx.vec(a[:N_EW]), d, nb)
        out.append((f"interpolate_{nb}", d.to_host()))
    d = ctx.empty(4 * (250 + 249 * 3))
    sampling.interpolate(ctx, ctx.vec(a[:4 * 250]), d, 3, frame_len=250)
    out.append(("interpolate_frames", d.to_host()))
    for dec in (2, 5):
        n = N_EW // dec * dec
        d = ctx.empty(n // dec)
        sampling.downsample(ctx, ctx.vec(a[:n]), d)
        out.append((f"downsample_{dec}", d.to_host()))
    # modulation and noise
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2, 2 * 8 * 1024, dtype=np.uint8)
    mods = {"bpsk": modulation.bpsk(ctx), "qpsk": modulation.qpsk(ctx), "qpsk_custom": modulation.table(ctx, CUSTOM_QPSK),
            "psk8": modulation.table(ctx, np.exp(2j * np.pi * np.arange(8) / 8).astype(np.complex64))}
    for name, mod in mods.items():
        k = mod.bits_per_symbol()
        bb = bits[:len(bits) // k * k]
        nsym = len(bb) // k
        sym = mod.modulate(bb)
        out.append((f"modulate_{name}", sym.to_host()))
        buf = ctx.empty(nsym + 1)                                           # symbols to an odd 8-byte slot
        mod.modulate(bb, out=buf.slice(1, nsym + 1))
        out.append((f"modulate_odd_{name}", buf.to_host()[1:]))
        noisy_h = _plant_ties(orc.awgn_apply(sym.to_host(), 0.4, 77))
        noisy = ctx.vec(noisy_h)
        for compat in (True, False):
            out.append((f"demod_{name}_{int(compat)}", mod.demod_naive(noisy, compat=compat).to_host()))
        odd = ctx.vec(np.concatenate([noisy_h[:1], noisy_h])).slice(1, nsym + 1)
        out.append((f"demod_odd_{name}", mod.demod_naive(odd).to_host()))
        if k <= 2:                                                          # modulate_awgn: BPSK / QPSK tables only
            out.append((f"modulate_awgn_{name}", mod.modulate_awgn(bb, noise.new(ctx, 0.3, 815)).to_host()))
            buf = ctx.empty(nsym + 1)
            mod.modulate_awgn(bb, noise.new(ctx, 0.3, 815), out=buf.slice(1, nsym + 1))
            out.append((f"modulate_awgn_odd_{name}", buf.to_host()[1:]))
    t = ctx.empty(N_EW); noise.new(ctx, 0.25, 99).fill(t)
    out.append(("awgn_fill", t.to_host()))
    t = ctx.vec(a[:N_EW]); noise.new(ctx, 0.25, 99).apply(t)
    out.append(("awgn_apply", t.to_host()))
    # FFT: every fused-stream power of two both ways, small ones, the other algorithms, the two epilogues
    for n in FFT_POW2 + tuple(n for n, _ in FFT_OTHER):
        batch = _fft_batch(n)
        x = rand_c64(n, n * batch)
        f = HipFft(ctx, n, max_batch=batch)
        for s, sg in ((Scale.SN, "f"), (Scale.X(0.5), "b")):
            d = ctx.vec(x)
            (f.ifwd if sg == "f" else f.ibwd)(d, s)
            out.append((f"fft_{n}_{sg}", d.to_host()))
        if n in (64, 1024, 1000):
            d = ctx.vec(x); f.rfft_mirror(d, Scale.SN)
            out.append((f"fft_mirror_{n}", d.to_host()))
            Lo = n + (n - 1) * 3
            d = ctx.empty(Lo * batch); f.rfft_interpolate(ctx.vec(x), d, 3, Scale.SN)
            out.append((f"fft_interp_{n}", d.to_host()))
    # the FIR at every fused length
    for L in FIR_LENS:
        x = rand_c64(L + 1, 20011)
        fir = Fir(ctx, _fir_taps(orc, L), L)
        out.append((f"fir_{L}", fir.filter(ctx.vec(x)).to_host()))
    # the correlator chain, plain and scaled
    for n in MUL_CHAIN_LENS:
        x = rand_c64(n + 2, n * 9); sig = ctx.vec(rand_c64(n + 3, n))
        f = HipFft(ctx, n, max_batch=9)
        for tag, s in (("plain", (Scale.NONE, Scale.NONE)), ("scaled", (Scale.SN, Scale.X(0.37)))):
            d = ctx.vec(x); f.mul_chain(d, sig, *s)
            out.append((f"mul_chain_{n}_{tag}", d.to_host()))
    # correlate + demod, every store kind
    for n in (1024, 2048, 4096):
        x = _demod_input(n, 4, n)
        f = HipFft(ctx, n, max_batch=4)
        sig = ctx.vec(rand_c64(9, n))
        for kind in DEMOD_KINDS:
            for tag, s in (("plain", (Scale.NONE, Scale.NONE)), ("scaled", (Scale.SN, Scale.SN))):
                out.append((f"corr_demod_{n}_{kind}_{tag}", mods[kind].correlate_demod(f, ctx.vec(x), sig, *s).to_host()))
    # decimating FIR
    for L in (1024, 2048, 4096):
        n = L * 6 // 4 * 4
        fir = Fir(ctx, _fir_taps(orc, L), L)
        out.append((f"fir_decim_{L}", fir.filter_decim(ctx.vec(rand_c64(L + 5, n)), 4).to_host()))
    return out


FIR_LONE = (512, 1024, 2048, 4096)          # the one-block-per-workgroup lengths: burst / spread prefetch, persistent grid


def _lone_input(L):
    """1 Mi samples: enough blocks for a grid of 1/16 of the resident one to wrap many times.  N = 2048 (128-lane
    workgroups, the only configuration the AETH_FIR_GRID_* knobs act on) gets 4 Mi: 2115 blocks, more than the 2048
    workgroups of 32/16 of the resident grid (1024 on 256 CUs), so that form is oversubscribed rather than clamped to
    the block count, and the default forms (16/16 alone, 12/16 beside) run yet other grids."""
    return rand_c64(L + 2, (1 << 22) if L == 2048 else (1 << 20))


def fir_forms(ctx, orc):
    """the one-block-per-workgroup FIR lengths as lone launches: [(key, result)]"""
    return [(f"fir_{L}", Fir(ctx, _fir_taps(orc, L), L).filter(ctx.vec(_lone_input(L))).to_host()) for L in FIR_LONE]


def fir_overlap_pairs(ctx, orc):
    """two back-to-back FIR launches on a context with the overlap lane on (the first alone, the second beside it).
    The grid knobs change the grid at N = 2048 only; at the other lengths the pair checks the lane itself."""
    out = []
    ctx.set_overlap(True)
    for L in FIR_LONE:
        fir = Fir(ctx, _fir_taps(orc, L), L)
        x = _lone_input(L)
        xs = [ctx.vec(x), ctx.vec(x)]
        ys = [ctx.empty(x.size), ctx.empty(x.size)]
        for i in (0, 1):
            fir.filter(xs[i], out=ys[i])
        ctx.sync()
        out += [(f"fir_{L}", ys[0].to_host()), (f"fir_{L}", ys[1].to_host())]
    ctx.set_overlap(False)
    return out


def _child(outdir):
    """the battery under every forced form; every result to outdir/<form>__<key>.npy.  Stops at the first error."""
    from oracle import pyoracle as orc
    ctx = ap.Context(0)

    def save(form, items):
        for i, (k, v) in enumerate(items):
            np.save(os.path.join(outdir, f"{form}__{i:03d}__{k}.npy"), v)

    for nt in ("0", "1"):
        os.environ["AETH_NT"] = nt
        save(f"nt{nt}", battery(ctx, orc))
        for sp in ("0", "1"):
            os.environ["AETH_FIR_SPREAD"] = sp
            save(f"nt{nt}_spread{sp}", fir_forms(ctx, orc))
        del os.environ["AETH_FIR_SPREAD"]
    del os.environ["AETH_NT"]
    for g in ("1", "32"):
        os.environ["AETH_FIR_GRID_FIRST"] = g
        os.environ["AETH_FIR_GRID_CHAINED"] = g
        save(f"grid{g}", fir_overlap_pairs(ctx, orc))
    ctx.close()
    print("battery ok")


def _oracle_check(orc, key, got):
    """the default battery result `key` against its oracle (bit-exact ops; transforms against f64 truth)"""
    a, b = _ew_inputs()
    if key.startswith("ew_"):
        _, op, ph = key.split("_")
        so, oo = int(ph[0]), int(ph[1])
        x, o = a[so:so + N_EW], b[oo:oo + N_EW]
        exp = {"scale": lambda: orc.vec_scale(x, np.float32(0.37)), "mul": lambda: orc.vec_mul(x, o),
               "div": lambda: orc.vec_div(x, o), "conj": lambda: orc.vec_conj(x), "add": lambda: orc.vec_add(x, o),
               "sub": lambda: orc.vec_sub(x, o), "clone": lambda: orc.vec_clone(x, o), "zero": lambda: orc.vec_zero(x),
               "mirror": lambda: orc.vec_mirror(x)}[op]()
        return bits_equal(got, exp)
    if key.startswith("chain_"):
        ph = key[-2:]
        so, oo = int(ph[0]), int(ph[1])
        x, o, p = a[so:so + N_EW], b[oo:oo + N_EW], a[::-1].copy()[oo:oo + N_EW]
        if key.startswith("chain_clone"):
            exp = orc.vec_add(orc.vec_mul(orc.vec_clone(x, o), p), o)
        else:
            exp = orc.vec_div(orc.vec_sub(orc.vec_scale(orc.vec_conj(orc.vec_mul(orc.vec_add(x, o), p)), np.float32(0.5)), o), p)
        return bits_equal(got, exp)
    if key.startswith("mul_frames_") or key.startswith("mirror_frames_"):
        L, off = (int(t) for t in key.split("_")[-2:])
        fr = a[off:off + L * 16].reshape(16, L)
        if key.startswith("mul"):
            exp = np.concatenate([orc.vec_mul(r, b[off:off + L]) for r in fr])
        else:
            exp = np.concatenate([orc.vec_mirror(r) for r in fr])
        return bits_equal(got, exp)
    if key.startswith("interpolate_frames"):
        return bits_equal(got, np.concatenate([orc.interpolate(f, 3) for f in a[:1000].reshape(4, 250)]))
    if key.startswith("interpolate_"):
        return bits_equal(got, orc.interpolate(a[:N_EW], int(key.split("_")[1])))
    if key.startswith("downsample_"):
        dec = int(key.split("_")[1]); n = N_EW // dec * dec
        return bits_equal(got, orc.downsample(a[:n], n // dec))
    if key == "awgn_fill":
        return bits_equal(got, orc.awgn_fill(N_EW, 0.25, 99))
    if key == "awgn_apply":
        return bits_equal(got, orc.awgn_apply(a[:N_EW], 0.25, 99))
    return None                                   # checked where the battery's inputs are at hand (test below)


@pytest.fixture(scope="module")
def defaults(ctx, oracle):
    """the battery and the lone FIR launches in this process, with the defaults, once: (battery, lone)"""
    return battery(ctx, oracle), fir_forms(ctx, oracle)


@pytest.fixture(scope="module")
def forced(tmp_path_factory):
    """run the child once; {form: [(key, array)]}"""
    d = tmp_path_factory.mktemp("variants")
    env = dict(os.environ, AETH_TUNING="1")
    for k in ("AETH_NT", "AETH_FIR_SPREAD", "AETH_FIR_GRID_FIRST", "AETH_FIR_GRID_CHAINED"):
        env.pop(k, None)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--battery", str(d)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    if r.returncode != 0:
        pytest.fail(f"battery child exited {r.returncode}:\n{r.stderr[-4000:]}")
    forms = {}
    for f in sorted(os.listdir(d)):
        form, _, key = f[:-4].split("__", 2)
        forms.setdefault(form, []).append((key, np.load(d / f)))
    return forms


def _same(a, b):
    if a.dtype == np.complex64:
        return bits_equal(a, b)
    return a.shape == b.shape and bool((a == b).all())


def test_forced_variants_give_the_default_bits(defaults, forced):
    """(a) cache policy, prefetch form and grid size change no bit: every forced form == the default in this process"""
    base, lone = defaults
    assert set(forced) == {"nt0", "nt1", "nt0_spread0", "nt0_spread1", "nt1_spread0", "nt1_spread1", "grid1", "grid32"}
    for nt in ("nt0", "nt1"):
        assert [k for k, _ in forced[nt]] == [k for k, _ in base]
        bad = [k for (k, v), (_, w) in zip(forced[nt], base) if not _same(v, w)]
        assert not bad, f"AETH_NT={nt[-1]} changed {bad}"
        for sp in ("0", "1"):
            got = forced[f"{nt}_spread{sp}"]
            assert [k for k, _ in got] == [k for k, _ in lone]
            bad = [k for (k, v), (_, w) in zip(got, lone) if not _same(v, w)]
            assert not bad, f"AETH_NT={nt[-1]} AETH_FIR_SPREAD={sp} changed {bad}"
    lone_d = dict(lone)
    for g in ("grid1", "grid32"):
        got = forced[g]
        assert len(got) == 2 * len(lone)
        bad = [k for k, v in got if not _same(v, lone_d[k])]
        assert not bad, f"{g}: overlap-lane launches changed {bad}"


def test_battery_defaults_meet_their_oracles(oracle, defaults):
    """(b) the default form of every battery call against its oracle (the forced forms equal it bit for bit, test above)"""
    base, lone = defaults
    res = dict(base)
    a, _ = _ew_inputs()
    checked = 0
    for k, v in base:
        ok = _oracle_check(oracle, k, v)
        if ok is not None:
            assert ok, k
            checked += 1
    # modulation / demod / noise, bit-exact
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2, 2 * 8 * 1024, dtype=np.uint8)
    tabs = {"bpsk": (1, None), "qpsk": (2, None), "qpsk_custom": (2, CUSTOM_QPSK),
            "psk8": (3, np.exp(2j * np.pi * np.arange(8) / 8).astype(np.complex64))}
    for name, (k, tab) in tabs.items():
        bb = bits[:len(bits) // k * k]
        sym = oracle.modulate(bb, k, tab)
        assert bits_equal(res[f"modulate_{name}"], sym) and bits_equal(res[f"modulate_odd_{name}"], sym), name
        noisy = _plant_ties(oracle.awgn_apply(sym, 0.4, 77))
        for compat in (True, False):
            assert (res[f"demod_{name}_{int(compat)}"] == oracle.demod_naive(noisy, k, tab, compat=compat)).all(), (name, compat)
        assert (res[f"demod_odd_{name}"] == oracle.demod_naive(noisy, k, tab)).all(), name
        checked += 5
        if k <= 2:
            want = oracle.awgn_apply(sym, 0.3, 815, 0)
            assert bits_equal(res[f"modulate_awgn_{name}"], want) and bits_equal(res[f"modulate_awgn_odd_{name}"], want), name
            checked += 2
    # transforms against f64 truth
    for n in FFT_POW2 + tuple(n for n, _ in FFT_OTHER):
        batch = _fft_batch(n)
        x = rand_c64(n, n * batch).astype(np.complex128)
        for sg, sign, s in (("f", ap.SIGN_REF_FWD, 1 / np.sqrt(n)), ("b", ap.SIGN_REF_BWD, 0.5)):
            e = oracle.evm_db(res[f"fft_{n}_{sg}"], oracle.fft_f64_frames(x, n, sign) * s)
            assert e <= TOL_DB, (n, sg, e)
            checked += 1
        if n in (64, 1024, 1000):
            X = (oracle.fft_f64_frames(x, n, ap.SIGN_REF_FWD) / np.sqrt(n)).reshape(batch, n)
            Xf = X.astype(np.complex64)
            e = oracle.evm_db(res[f"fft_mirror_{n}"], np.concatenate([oracle.vec_mirror(r) for r in Xf]))
            assert e <= TOL_DB, (n, "mirror", e)
            e = oracle.evm_db(res[f"fft_interp_{n}"], np.concatenate([oracle.interpolate(r, 3) for r in Xf]))
            assert e <= TOL_DB, (n, "interpolate", e)
            checked += 2
    for L in FIR_LENS:
        x = rand_c64(L + 1, 20011)
        e = oracle.evm_db(res[f"fir_{L}"], oracle.fir_direct_f64(_fir_taps(oracle, L), x))
        assert e <= TOL_DB, (L, e)
        checked += 1
    for n in MUL_CHAIN_LENS:
        x = rand_c64(n + 2, n * 9); sig = rand_c64(n + 3, n)
        for tag, s in (("plain", (Scale.NONE, Scale.NONE)), ("scaled", (Scale.SN, Scale.X(0.37)))):
            e = oracle.evm_db(res[f"mul_chain_{n}_{tag}"], chain_truth(oracle, x, sig, n, *s))
            assert e <= TOL_DB, (n, tag, e)
            checked += 1
    for n in (1024, 2048, 4096):
        x = _demod_input(n, 4, n)
        sig = rand_c64(9, n)
        for tag, s in (("plain", (Scale.NONE, Scale.NONE)), ("scaled", (Scale.SN, Scale.SN))):
            y = chain_truth(oracle, x, sig, n, *s)
            for kind in DEMOD_KINDS:
                k, tab = tabs[kind]
                want = oracle.demod_naive(y.astype(np.complex64), k, tab)
                got = res[f"corr_demod_{n}_{kind}_{tag}"]
                # decisions against the f64 chain: equal except where the f32 chain lands on the other side of a boundary
                assert (got != want).mean() < 2e-3, (n, kind, tag, float((got != want).mean()))
                checked += 1
    for L in (1024, 2048, 4096):
        n = L * 6 // 4 * 4
        x = rand_c64(L + 5, n)
        e = oracle.evm_db(res[f"fir_decim_{L}"], oracle.fir_direct_f64(_fir_taps(oracle, L), x)[::4])
        assert e <= TOL_DB, (L, "decim", e)
        checked += 1
    assert checked == len(base), (checked, len(base))
    for k, v in lone:
        L = int(k.split("_")[1])
        e = oracle.evm_db(v, oracle.fir_direct_f64(_fir_taps(oracle, L), _lone_input(L)))
        assert e <= TOL_DB, (k, "lone launch", e)


def test_battery_lengths_take_their_routes(ctx):
    """the battery's transform lengths reach the algorithms they stand for"""
    for n, algo in FFT_OTHER:
        assert HipFft(ctx, n).algorithm == algo, n
    for n in FFT_POW2:                             # 8192 has a row of its own in the ragged table
        assert HipFft(ctx, n).algorithm == ("stockham_mixed_ragged" if n == 8192 else "stockham_pow2"), n


if __name__ == "__main__" and len(sys.argv) == 3 and sys.argv[1] == "--battery":
    _child(sys.argv[2])
