"""GPU parity: the head of a stream in the fused overlap-save kernel, and the halo between its blocks.

Block 0 of a launch starts `ov` samples in front of the stream: its window is zeros, then the history (when one is
given), then the first `hop` samples.  Every later block's window starts with the last `ov` samples of its left
neighbour's.  The cases sit on the sizes at which those two paths can go wrong: streams of one sample, of one block
less / exactly / plus one sample, of three blocks; a history of none, of one sample (a 2-tap plan: the other 62 halo
elements of slot 0 stay zero) and of ntaps - 1 samples; 200 taps (ov = 256 > T = 128: the history spans slots 0 and 1);
a 1024-point plan (T = 64); the decimating, level, peak and demodulating stores; both cache builds (AETH_NT = 0 / 1,
which the library reads only under AETH_TUNING=1, so the cases run in ONE child process).

Per case:
  1. agreement with the f64 direct convolution at the tolerance of tests/test_gpu_fir.py (aggregate EVM <= -120 dB;
     streams shorter than ntaps - 1 samples, its 63: the absolute bound it uses there, because the transform's error
     scales with the block while those outputs are the filter's start-up, the small leading taps of a low-pass);
  2. with a history: filtering x[k:] behind x[k - (ntaps-1):k] gives the bits of filtering x whole, from output k on
     (k = hop);
  3. the SHA-256 of the output bytes is the one tests/golden/fir_head_parent.json records (written by
     tools/fir_head_golden.py from the kernel as it was before the halo slots lost the streaming hint: a change to how
     a window is loaded touches no arithmetic, so no bit may move).

The store forms: the decimated stream against every dec-th sample of f64 truth; levels against |truth| (||a| - |b|| <=
|a - b|, and the level's own rounding lies 24 dB below the bound, so the samples' -120 dB holds for the levels); the
peak's index against truth's argmax and its norm to 2^-20 (-120 dB); the demodulated frames (no overlap and no history
there: a window never starts in front of the stream) as the bits of demod_naive on the chain's samples, which meet f64
truth themselves."""
import hashlib
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
from helpers import bits_equal, rand_c64                # noqa: E402

pytestmark = pytest.mark.gpu
TOL_DB = -120.0
GOLDEN = os.path.join(HERE, "golden", "fir_head_parent.json")

# plan -> (ntaps, fft_len, hop); hop = floor64(fft_len - ntaps + 1), asserted against the library in the child
PLANS = {"t64": (64, 2048, 1984), "t2": (2, 2048, 1984), "t200": (200, 2048, 1792), "t64n1024": (64, 1024, 960)}
N_SET = (1, 63, 64, 65, 1983, 1984, 1985, 2 * 1984 + 5, 3 * 1984)
N_SET_200 = tuple(sorted(set(N_SET) | {1791, 1792, 1793, 2 * 1792 + 5, 3 * 1792}))     # ... and its own block edges
FORMS = ("decim", "level", "peak", "demod")
DECIM = 29                                              # 2 * 1984 + 5 = 29 * 137


def case_list():
    """(plan, with_history, n, form) of every case; form None = the sample store"""
    out = []
    for n in N_SET:
        out += [("t64", False, n, None), ("t64", True, n, None), ("t2", True, n, None)]
    for n in N_SET_200:
        out += [("t200", False, n, None), ("t200", True, n, None)]
    out += [("t64n1024", False, 2 * 960 + 5, None), ("t64n1024", True, 2 * 960 + 5, None)]
    out += [("t64", True, 2 * 1984 + 5, form) for form in FORMS if form != "demod"]
    out += [("t64", False, 3 * 2048, "demod")]              # three 2048-sample frames
    return out


def case_id(nt, plan, hist, n, form):
    h = PLANS[plan][0] - 1 if hist else 0
    return f"nt{nt}-{plan}-h{h}-n{n}" + (f"-{form}" if form else "")


CASES = case_list()
IDS = [case_id(nt, *c) for nt in (0, 1) for c in CASES]
IDS_HIST = [case_id(nt, *c) for nt in (0, 1) for c in CASES if c[1] and c[3] != "demod"]


def _taps(orc, plan):
    ntaps = PLANS[plan][0]
    if ntaps == 2:
        return np.array([0.6 + 0.2j, -0.3 + 0.5j], np.complex64)
    return orc.synth_lowpass_taps(ntaps, 0.25)


def _sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _db(err, ref):
    return 20.0 * np.log10(np.sqrt(np.mean(np.abs(err) ** 2)) / np.sqrt(np.mean(np.abs(ref) ** 2)))


def _closeness(orc, y, truth, taps, x_all):
    """assertion 1 in the form tests/test_gpu_fir.py uses: {'evm'} or {'abs', 'bound'}"""
    if y.size >= taps.size - 1:
        return {"evm": float(orc.evm_db(y, truth))}
    bound = 4 * 2.0 ** -23 * float(np.abs(x_all).max()) * float(np.abs(taps).sum())
    return {"abs": float(np.abs(y - truth).max()), "bound": bound}


def run_case(ctx, orc, plan, hist, n, form, objs):
    """one case -> {'sha', 'evm' | ('abs', 'bound'), 'hist_ok', ...}"""
    ntaps, fft_len, hop = PLANS[plan]
    taps = _taps(orc, plan)
    k = hop if hist else 0
    seed = 7000 + 100 * list(PLANS).index(plan) + (50 if hist else 0) + n % 47 + (FORMS.index(form) if form else 0)
    if form == "demod":
        return _run_demod(ctx, orc, fft_len, seed)
    xx = rand_c64(seed, k + n)
    d = ctx.vec(xx)
    x, h = d.slice(k, k + n), (d.slice(k - (ntaps - 1), k) if hist else None)
    rec = {}
    if form in ("level", "peak"):
        ref = np.conj(taps[::-1]).astype(np.complex64)          # c = the causal matched filter of ref: its taps are `taps`
        if ("corr", plan) not in objs:
            objs[("corr", plan)] = ap.Corr(ctx, ref, fft_len)
        corr = objs[("corr", plan)]
        assert (corr.nref, corr.hop) == (ntaps, hop)
    else:
        if ("fir", plan) not in objs:
            objs[("fir", plan)] = ap.Fir(ctx, taps, fft_len)
        fir = objs[("fir", plan)]
        assert (fir.ntaps, fir.hop) == (ntaps, hop)
    truth = orc.fir_direct_f64(taps, xx)[k:]
    if form is None:
        y = fir.filter(x, hist=h).to_host()
        rec.update(_closeness(orc, y, truth, taps, xx))
        if hist:
            rec["hist_ok"] = bits_equal(y, fir.filter(d).to_host()[k:])
        rec["sha"] = _sha(y)
    elif form == "decim":
        y = fir.filter_decim(x, DECIM, hist=h).to_host()
        rec["evm"] = float(orc.evm_db(y, truth[::DECIM]))
        rec["hist_ok"] = bits_equal(y, fir.filter(d).to_host()[k:][::DECIM])
        rec["sha"] = _sha(y)
    elif form == "level":
        y = corr.levels(x, hist=h).to_host()
        rec["evm"] = float(_db(y.astype(np.float64) - np.abs(truth), truth))
        whole = corr.levels(d).to_host()[k:]
        rec["hist_ok"] = bool((y.view(np.uint32) == whole.view(np.uint32)).all())
        rec["sha"] = _sha(y)
    else:
        best, blocks = corr.search(x, hist=h, blocks=True)
        want = int(np.argmax(np.abs(truth) ** 2))
        rec["index"], rec["want_index"] = best.index, want
        rec["norm_rel"] = abs(best.norm - abs(truth[want])) / abs(truth[want])
        _, wb = corr.search(d, blocks=True)
        wb = wb[1:]                                             # k = hop: the whole stream's block b + 1 is this one's b
        rec["hist_ok"] = bool(blocks.size == wb.size and (blocks["index"] + k == wb["index"]).all()
                              and (blocks["norm"].view(np.uint32) == wb["norm"].view(np.uint32)).all()
                              and (blocks["n_nan"] == wb["n_nan"]).all())
        rec["sha"] = _sha(blocks, np.array([best.index, best.n_nan], np.uint64), np.array([best.norm], np.float32))
    return rec


def _run_demod(ctx, orc, n, seed):
    frames = 3
    x, sig = rand_c64(seed, n * frames, scale=1.5), rand_c64(seed + 1, n)
    f, mod = ap.HipFft(ctx, n, max_batch=frames), ap.modulation.qpsk(ctx)
    sigd = ctx.vec(sig)
    got = mod.correlate_demod(f, ctx.vec(x), sigd).to_host()
    ref = ctx.vec(x); f.mul_chain(ref, sigd)
    X = orc.fft_f64_frames(x.astype(np.complex128), n, ap.SIGN_REF_FWD).reshape(frames, n) * sig.astype(np.complex128)
    truth = orc.fft_f64_frames(X.reshape(-1), n, ap.SIGN_REF_BWD)
    return {"evm": float(orc.evm_db(ref.to_host(), truth)), "bits_ok": bool((got == mod.demod_naive(ref).to_host()).all()),
            "sha": _sha(got)}


def run_all(ctx, orc):
    """every case under both cache builds (needs AETH_TUNING=1 in the environment of the process)"""
    out, objs = {}, {}
    for nt in (0, 1):
        os.environ["AETH_NT"] = str(nt)
        for c in CASES:
            out[case_id(nt, *c)] = run_case(ctx, orc, *c, objs)
    del os.environ["AETH_NT"]
    return out


def run_child(path):
    """run_all in a fresh process under AETH_TUNING=1 -> {case id: record} (also left at `path` as JSON)"""
    env = dict(os.environ, AETH_TUNING="1")
    for key in ("AETH_NT", "AETH_FIR_SPREAD", "AETH_FIR_GRID_FIRST", "AETH_FIR_GRID_CHAINED"):
        env.pop(key, None)
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "--child", str(path)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240, cwd=ROOT)
    if r.returncode != 0:
        raise RuntimeError(f"fir-head child exited {r.returncode}:\n{r.stderr[-4000:]}")
    with open(path) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def results(ctx, tmp_path_factory):
    return run_child(tmp_path_factory.mktemp("fir_head") / "results.json")


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_every_case_ran_and_has_a_golden_hash(results, golden):
    assert sorted(results) == sorted(IDS) and sorted(golden) == sorted(IDS)


@pytest.mark.parametrize("cid", IDS)
def test_agrees_with_f64_direct_convolution(results, cid):
    r = results[cid]
    print(cid, {k: v for k, v in r.items() if k != "sha"})
    if "evm" in r:
        assert r["evm"] <= TOL_DB
    if "abs" in r:
        assert r["abs"] <= r["bound"]
    if "index" in r:
        assert r["index"] == r["want_index"] and r["norm_rel"] <= 2.0 ** -20
    if "bits_ok" in r:
        assert r["bits_ok"]


@pytest.mark.parametrize("cid", IDS_HIST)
def test_history_continues_the_stream_bit_for_bit(results, cid):
    assert results[cid]["hist_ok"] is True


@pytest.mark.parametrize("cid", IDS)
def test_bits_are_the_parents(results, golden, cid):
    assert results[cid]["sha"] == golden[cid]


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        from oracle import pyoracle
        c = ap.Context(0)
        res = run_all(c, pyoracle)
        c.close()
        with open(sys.argv[2], "w") as fh:
            json.dump(res, fh, indent=0, sort_keys=True)
        print("fir head ok")
