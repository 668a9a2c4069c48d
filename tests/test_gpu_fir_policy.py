"""GPU parity: the cache policy of the fused overlap-save kernel's stream accesses changes no bit.

The streaming builds of the kernel (AETH_NT = 1) pick a cache policy per access -- window body, window halo, sample
store -- by compile-time rules on the slot index (aeth_fir_kernel.h: StreamPolicy); the plain builds (AETH_NT = 0)
carry no policy at all.  A policy is a hint on where a line is kept, so per case:

  1. the AETH_NT = 0 output agrees with the f64 direct convolution at the bound of tests/test_gpu_fir_head.py
     (aggregate EVM <= -120 dB; streams shorter than ntaps - 1 samples: its absolute bound);
  2. the AETH_NT = 1 output equals the AETH_NT = 0 output byte for byte, in both forms of the window prefetch
     (AETH_FIR_SPREAD = 0: one burst; 1: four instalments, where the plan has that build).

The library reads the knobs only under AETH_TUNING=1, so the cases run in ONE child process.

Cases, the smallest that reach every path the rules touch:
  * FFT length 2048 with 64 and 65 taps (ov = 64: the halo is half of slot 0 and half of slot 15), 100 taps (ov = 128:
    exactly those two slots), 200 taps (ov = 256: slots 0, 1, 14 and 15, the four this length loads without the hint);
    FFT length 1024 with 64 taps (T = 64: one wave per workgroup, every slot is one wave's, the first and the last
    without the hint);
  * n in {1, hop - 1, hop + 1, 5 hop + 17, 13 hop + 3}, with and without a history of ntaps - 1 samples (k = hop);
  * a grid these streams do not fill runs every block in its workgroup's prologue, and the persistent loop's prefetch
    (the branch-free descriptor path, the one the steady state consists of) fetches only blocks past the end.  The
    smallest grid the library can be told to launch is 1/16 of the resident one (AETH_FIR_GRID_FIRST = 1 on a context
    with the overlap lane on: 64 workgroups of 128 lanes on 256 CUs); n = (cap/16 + 3) hop + 3 on such a context wraps
    that grid, so its last blocks are loaded by the loop.  The 1024-point plan (64-lane workgroups, on which the knob
    does not act) gets n = (8 CUs' worth more than its resident grid) instead;
  * one correlator-frame case (ov = 0: three 2048-sample frames through mul_chain), one decimating case and one
    demodulating case, whose stores use the same policy constant at other widths."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import aether_primitives_amd as ap                      # noqa: E402
from helpers import rand_c64                            # noqa: E402

pytestmark = pytest.mark.gpu
TOL_DB = -120.0                                         # tests/test_gpu_fir_head.py, tests/test_gpu_fir.py

# plan -> (ntaps, fft_len, hop); hop = floor64(fft_len - ntaps + 1), asserted against the library in the child
PLANS = {"t64": (64, 2048, 1984), "t65": (65, 2048, 1984), "t100": (100, 2048, 1920), "t200": (200, 2048, 1792),
         "t64n1024": (64, 1024, 960)}
DECIM = 29
CUS = 256                                               # MI355X; a device with fewer wraps the grid all the more
NT1 = ("nt1_spread0", "nt1_spread1")


def n_set(hop):
    return (1, hop - 1, hop + 1, 5 * hop + 17, 13 * hop + 3)


def case_list():
    """(plan, with_history, n, form); form None = the sample store, "wrap" = the sample store on a grid the stream wraps
    (n = the number of blocks beyond the grid; the child turns it into samples once it knows the grid)"""
    out = []
    for plan, (_, _, hop) in PLANS.items():
        for n in n_set(hop):
            out += [(plan, False, n, None), (plan, True, n, None)]
        out += [(plan, False, 3, "wrap"), (plan, True, 3, "wrap")]
    out += [("t64", True, 2 * 1984 + 5, "decim"), ("t64", False, 3 * 2048, "frames"), ("t64", False, 3 * 2048, "demod")]
    return out


def case_id(plan, hist, n, form):
    return f"{plan}-h{PLANS[plan][0] - 1 if hist else 0}-n{n}" + (f"-{form}" if form else "")


CASES = case_list()
IDS = [case_id(*c) for c in CASES]


def _taps(orc, plan):
    return orc.synth_lowpass_taps(PLANS[plan][0], 0.25)


def _closeness(orc, y, truth, taps, x_all):
    if y.size >= taps.size - 1:
        return {"evm": float(orc.evm_db(y, truth))}
    return {"abs": float(np.abs(y - truth).max()),
            "bound": 4 * 2.0 ** -23 * float(np.abs(x_all).max()) * float(np.abs(taps).sum())}


def _forms(fn):
    """fn() under AETH_NT = 0, then under AETH_NT = 1 with either prefetch form -> (plain result, {form: bytes equal})"""
    os.environ["AETH_NT"] = "0"
    y0 = fn()
    same = {}
    os.environ["AETH_NT"] = "1"
    for sp in ("0", "1"):
        os.environ["AETH_FIR_SPREAD"] = sp
        y = fn()
        same[f"nt1_spread{sp}"] = bool(y.dtype == y0.dtype and y.shape == y0.shape and y.tobytes() == y0.tobytes())
    del os.environ["AETH_FIR_SPREAD"], os.environ["AETH_NT"]
    return y0, same


def run_case(ctx, orc, plan, hist, n, form, objs):
    ntaps, fft_len, hop = PLANS[plan]
    seed = 9000 + 100 * list(PLANS).index(plan) + (50 if hist else 0) + n % 47
    if form in ("frames", "demod"):
        return _run_frames(ctx, orc, fft_len, seed, form)
    taps = _taps(orc, plan)
    if plan not in objs:
        objs[plan] = ap.Fir(ctx, taps, fft_len)
    fir = objs[plan]
    assert (fir.ntaps, fir.hop) == (ntaps, hop)
    rec = {}
    if form == "wrap":
        # the resident grid is 8 waves per CU; 128-lane workgroups can be held to 1/16 of it, 64-lane ones cannot
        cap = CUS * 8 // (2 if fft_len == 2048 else 1)
        grid = cap // 16 if fft_len == 2048 else cap
        n = (grid + n) * hop + 3
        rec["blocks"], rec["grid"] = -(-n // hop), grid
    k = hop if hist else 0
    xx = rand_c64(seed, k + n)
    d = ctx.vec(xx)
    x, h = d.slice(k, k + n), (d.slice(k - (ntaps - 1), k) if hist else None)
    truth = orc.fir_direct_f64(taps, xx)[k:]
    if form == "decim":
        y0, same = _forms(lambda: fir.filter_decim(x, DECIM, hist=h).to_host())
        rec["evm"] = float(orc.evm_db(y0, truth[::DECIM]))
    elif form == "wrap" and fft_len == 2048:
        ctx.set_overlap(True)
        os.environ["AETH_FIR_GRID_FIRST"] = os.environ["AETH_FIR_GRID_CHAINED"] = "1"

        def go():
            y = fir.filter(x, hist=h)
            ctx.sync()
            return y.to_host()
        y0, same = _forms(go)
        del os.environ["AETH_FIR_GRID_FIRST"], os.environ["AETH_FIR_GRID_CHAINED"]
        ctx.set_overlap(False)
        rec.update(_closeness(orc, y0, truth, taps, xx))
    else:
        y0, same = _forms(lambda: fir.filter(x, hist=h).to_host())
        rec.update(_closeness(orc, y0, truth, taps, xx))
    rec["same"] = same
    return rec


def _run_frames(ctx, orc, n, seed, form):
    """three n-sample frames through FFT * sig * IFFT (ov = 0), as samples or as demodulated bits"""
    frames = 3
    x, sig = rand_c64(seed, n * frames, scale=1.5), rand_c64(seed + 1, n)
    f, mod = ap.HipFft(ctx, n, max_batch=frames), ap.modulation.qpsk(ctx)
    sigd = ctx.vec(sig)

    def chain():
        v = ctx.vec(x); f.mul_chain(v, sigd)
        return v.to_host()
    y0, same = _forms(chain)
    X = orc.fft_f64_frames(x.astype(np.complex128), n, ap.SIGN_REF_FWD).reshape(frames, n) * sig.astype(np.complex128)
    rec = {"evm": float(orc.evm_db(y0, orc.fft_f64_frames(X.reshape(-1), n, ap.SIGN_REF_BWD)))}
    if form == "demod":
        b0, same_bits = _forms(lambda: mod.correlate_demod(f, ctx.vec(x), sigd).to_host())
        same = {k: same[k] and same_bits[k] for k in same}
        rec["bits_ok"] = bool((b0 == mod.demod_naive(ctx.vec(y0)).to_host()).all())
    rec["same"] = same
    return rec


def run_child(path):
    """every case in a fresh process under AETH_TUNING=1 -> {case id: record} (also left at `path` as JSON)"""
    env = dict(os.environ, AETH_TUNING="1")
    for key in ("AETH_NT", "AETH_FIR_SPREAD", "AETH_FIR_GRID_FIRST", "AETH_FIR_GRID_CHAINED"):
        env.pop(key, None)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child", str(path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    if r.returncode != 0:
        raise RuntimeError(f"fir-policy child exited {r.returncode}:\n{r.stderr[-4000:]}")
    with open(path) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def results(ctx, tmp_path_factory):
    return run_child(tmp_path_factory.mktemp("fir_policy") / "results.json")


def test_every_case_ran(results):
    assert sorted(results) == sorted(IDS)


@pytest.mark.parametrize("cid", [i for i in IDS if i.endswith("-wrap")])
def test_wrapping_streams_wrap_their_grid(results, cid):
    assert results[cid]["blocks"] > results[cid]["grid"]


@pytest.mark.parametrize("cid", IDS)
def test_plain_build_agrees_with_f64_direct_convolution(results, cid):
    r = results[cid]
    print(cid, {k: v for k, v in r.items() if k != "same"})
    assert "evm" in r or "abs" in r
    if "evm" in r:
        assert r["evm"] <= TOL_DB
    if "abs" in r:
        assert r["abs"] <= r["bound"]
    if "bits_ok" in r:
        assert r["bits_ok"]


@pytest.mark.parametrize("form", NT1)
@pytest.mark.parametrize("cid", IDS)
def test_streaming_build_gives_the_plain_builds_bytes(results, cid, form):
    assert results[cid]["same"][form] is True


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        from oracle import pyoracle
        c = ap.Context(0)
        objs = {}
        res = {case_id(*case): run_case(c, pyoracle, *case, objs) for case in CASES}
        c.close()
        with open(sys.argv[2], "w") as fh:
            json.dump(res, fh, indent=0, sort_keys=True)
        print("fir policy ok")
