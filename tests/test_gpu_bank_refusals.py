"""GPU: every refusal of the two filter banks (aeth_chan_*, aeth_synth_*) by return code, complete message and order.

tests/test_gpu_chan.py and tests/test_gpu_synth.py refuse one fault at a time and match words of the message.  Here one
table of bad calls is replayed against tests/golden/bank_refusals.json: per case the entry point, the case's name, the
return code and the whole aeth_last_error() string.  The two-fault cases fix which check comes first.  The messages
hold sizes and kinds, never an address, so the file does not depend on where the buffers lie.

Shapes: M = 16, P = 2, D = 4 (STREAM; the general kernels) and M = 16, P = 2, D = 16 (the ring kernel; for the synthesis
bank the fold route).  Every case is refused before any device work.

    python tests/test_gpu_bank_refusals.py --record [PATH]      writes the file (default: tests/golden/bank_refusals.json)

The committed file was recorded at the commit before the banks' shared host core (csrc/aeth_bank.h)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):                             # also run as a script: --record
    if _p not in sys.path:
        sys.path.insert(0, _p)

from helpers import bits_equal, rand_c64                                   # noqa: E402

import aether_primitives_amd as ap                                         # noqa: E402
from aether_primitives_amd import _lib                                     # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(ROOT, "tests", "golden", "bank_refusals.json")
M, P, FRAMES = 16, 2, 5
HOPS = (4, 16)
NO_ROUTE = 8388609                                # a transform length the planner refuses: tests/test_gpu_chan.py:312
p = C.c_void_p


def create_cases(lib, ctx, bank):
    """[(entry, case, thunk -> rc)] for aeth_<bank>_create"""
    create, destroy = getattr(lib, f"aeth_{bank}_create"), getattr(lib, f"aeth_{bank}_destroy")
    w = np.ones(130, np.float32)
    big = np.ones(NO_ROUTE, np.float32)
    W, BIG = w.ctypes.data, big.ctypes.data

    def mk(ctxh=ctx.h, proto=W, ntaps=64, channels=16, hop=16, phase=0, out=True, keep=(w, big)):
        def thunk():
            h = C.c_void_p(0x55)
            rc = create(ctxh, p(proto), ntaps, channels, hop, phase, 0, C.byref(h) if out else None)
            if out:
                assert (rc == 0) == bool(h.value), "a refused create must clear *out"
                if h.value:
                    destroy(h)
            return rc
        return thunk

    cases = [
        ("taps_not_a_multiple", mk(channels=5, hop=5)),
        ("zero_channels", mk(channels=0, hop=0)),
        ("hop_zero", mk(hop=0)),
        ("hop_above_channels", mk(hop=17)),
        ("bad_phase", mk(phase=2)),
        ("65_taps_per_channel", mk(ntaps=130, channels=2, hop=2)),
        ("prototype_null", mk(proto=None)),
        ("zero_taps", mk(ntaps=0)),
        ("out_null", mk(out=False)),
        ("ctx_null", mk(ctxh=None)),
        ("length_without_a_route", mk(proto=BIG, ntaps=NO_ROUTE, channels=NO_ROUTE, hop=NO_ROUTE)),
        # two faults: the first check wins
        ("out_null+ctx_null", mk(ctxh=None, out=False)),
        ("prototype_null+zero_channels", mk(proto=None, channels=0, hop=0)),
        ("taps_not_a_multiple+hop_zero", mk(channels=5, hop=0)),
        ("65_taps_per_channel+hop_above_channels", mk(ntaps=130, channels=2, hop=3)),
        ("bad_phase+length_without_a_route", mk(proto=BIG, ntaps=NO_ROUTE, channels=NO_ROUTE, hop=NO_ROUTE, phase=2)),
    ]
    if bank == "synth":
        cases += [
            ("512_frames_overlap", mk(proto=BIG, ntaps=512, channels=512, hop=1)),
            ("1024_frames_overlap", mk(proto=BIG, ntaps=1024, channels=1024, hop=1)),
            # ... before the plan is touched
            ("frames_overlap+length_without_a_route", mk(proto=BIG, ntaps=NO_ROUTE, channels=NO_ROUTE, hop=1)),
        ]
    return [(f"aeth_{bank}_create", name, t) for name, t in cases]


class Bank:
    """one bank object of hop D with its buffers: `n` input samples make `no` output elements"""

    def __init__(self, ctx, bank, D):
        self.bank, self.D = bank, D
        w = np.random.default_rng(1000 * M + P).standard_normal(M * P).astype(np.float32)
        if bank == "chan":
            self.obj = ap.Channelizer(ctx, w, M, D, "stream")
            self.n, self.no, nhist = FRAMES * D, FRAMES * M, M * P - D
        else:
            self.obj = ap.Synthesizer(ctx, w, M, D, "stream")
            self.n, self.no, nhist = FRAMES * M, FRAMES * D, self.obj.history * M
        self.nhist = nhist
        self.x, self.hist = ctx.vec(rand_c64(1, self.n + 2)), ctx.vec(rand_c64(2, nhist))
        self.sentinel = np.full(self.no + 2, 1.5 - 2.5j, np.complex64)
        self.out = ctx.vec(self.sentinel)
        self.lev = ap.DeviceF32(ctx, self.no + 2)


def call_cases(lib, b):
    """[(entry, case, thunk -> rc)] for the exec-like calls of one bank object"""
    X, H, O, LV, n, no, h = b.x.ptr, b.hist.ptr, b.out.ptr, b.lev.ptr, b.n, b.no, b.obj.h
    if b.bank == "chan":
        def fold(c=h, h=H, i=X, nn=n, o=O, no=no):
            return lib.aeth_chan_fold(c, p(h), p(i), nn, 0, p(o), no)

        def ex(c=h, h=H, i=X, nn=n, o=O, no=no, sign=1, kind=0):
            return lib.aeth_chan_exec(c, p(h), p(i), nn, 0, sign, kind, 0.0, p(o), no)

        def lv(c=h, h=H, i=X, nn=n, o=LV, no=no, sign=1, kind=0, lk=0):
            return lib.aeth_chan_exec_levels(c, p(h), p(i), nn, 0, sign, kind, 0.0, 0, lk, p(o), no)

        entries = [("aeth_chan_fold", fold, O, 8, False), ("aeth_chan_exec", ex, O, 8, True), ("aeth_chan_exec_levels", lv, LV, 4, True)]
    else:
        def unfold(c=h, h=H, i=X, nn=n, o=O, no=no):
            return lib.aeth_synth_unfold(c, p(h), p(i), nn, 0, p(o), no)

        def ex(c=h, h=H, i=X, nn=n, o=O, no=no, sign=1, kind=0):
            return lib.aeth_synth_exec(c, p(h), p(i), nn, 0, sign, kind, 0.0, p(o), no)

        entries = [("aeth_synth_unfold", unfold, O, 8, False), ("aeth_synth_exec", ex, O, 8, True)]
    out = []
    for entry, f, o, esz, transforms in entries:
        levels = esz == 4
        cases = [
            ("handle_null", dict(c=None)),
            ("in_null", dict(i=None)),
            ("out_null", dict(o=None)),
            ("zero_samples", dict(nn=0, no=0)),
            ("one_sample_more", dict(nn=n + 1)),
            ("one_output_less", dict(no=no - 1)),
            ("one_output_more", dict(no=no + 1)),
            ("in_misaligned", dict(i=X + 4)),
            ("hist_misaligned", dict(h=H + 4)),
            ("out_misaligned", dict(o=o + esz // 2)),
            # the output range must be clear of the input and of the history
            ("out_is_in", dict(o=X)),
            ("out_on_last_of_in", dict(o=X + 8 * (n - 1))),
            ("in_on_last_of_out", dict(i=o + esz * (no - 1) // 8 * 8)),
            ("hist_on_last_of_out", dict(h=o + esz * (no - 1) // 8 * 8)),
            ("out_is_hist", dict(o=H)),
            ("out_on_last_of_hist", dict(o=H + 8 * (b.nhist - 1))),
            # two faults: the first check wins
            ("zero_samples+in_null", dict(nn=0, no=0, i=None)),
            ("one_output_less+out_misaligned", dict(no=no - 1, o=o + esz // 2)),
            ("in_null+hist_misaligned", dict(i=None, h=H + 4)),
            ("in_misaligned+out_is_in", dict(i=X + 4, o=X)),
        ]
        if transforms:
            cases += [
                ("sign_zero", dict(sign=0)),
                ("sign_two", dict(sign=2)),
                ("scale_kind_4", dict(kind=4)),
                ("scale_kind_-1", dict(kind=-1)),
                ("out_is_in+sign_zero", dict(o=X, sign=0)),
                ("sign_zero+scale_kind_4", dict(sign=0, kind=4)),
            ]
        if levels:
            cases += [
                ("level_kind_3", dict(lk=3)),
                ("scale_kind_4+level_kind_3", dict(kind=4, lk=3)),
            ]
        out += [(entry, f"D{b.D}:{name}", (lambda f=f, kw=kw: f(**kw))) for name, kw in cases]
        out.append((entry, f"D{b.D}:right", f))                     # replayed last, see run()
    return out


def run(ctx):
    """every case of the table -> [{"entry", "case", "rc", "error"}]; then nothing was written and the right calls run"""
    lib = _lib.load()
    banks = [Bank(ctx, bank, D) for bank in ("chan", "synth") for D in HOPS]
    table = create_cases(lib, ctx, "chan") + create_cases(lib, ctx, "synth")
    right = []
    for b in banks:
        for row in call_cases(lib, b):
            (right if row[1].endswith(":right") else table).append(row)
    assert len({(e, c) for e, c, _ in table}) == len(table), "case names must be unique"
    got = []
    for entry, case, thunk in table:
        rc = thunk()
        assert rc != 0, f"{entry} {case}: the call was not refused"
        got.append({"entry": entry, "case": case, "rc": rc, "error": lib.aeth_last_error().decode()})
    ctx.sync()
    for b in banks:
        assert bits_equal(b.out.to_host(), b.sentinel), f"{b.bank} D = {b.D}: a refused call wrote to its output"
    for entry, case, thunk in right:                                # the same arguments, made right, run
        assert thunk() == 0, (entry, case, lib.aeth_last_error().decode())
    ctx.sync()
    return got


def test_every_refusal_by_code_text_and_order(ctx):
    want = json.load(open(GOLDEN))["cases"]
    got = run(ctx)
    assert [(g["entry"], g["case"]) for g in got] == [(w["entry"], w["case"]) for w in want], "the table and the recorded file differ in their cases"
    wrong = [(g, w) for g, w in zip(got, want) if g != w]
    for g, w in wrong:
        print(f"{g['entry']} {g['case']}:\n  recorded [{w['rc']}] {w['error']}\n  now      [{g['rc']}] {g['error']}")
    assert not wrong, f"{len(wrong)} of {len(want)} refusals changed their code or text"
    assert not any("0x" in w["error"] for w in want), "a recorded message holds an address"


if __name__ == "__main__" and len(sys.argv) >= 2 and sys.argv[1] == "--record":
    _ctx = ap.Context(0)
    _cases = run(_ctx)
    _ctx.close()
    _path = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    with open(_path, "w") as _f:
        json.dump({"comment": "tests/test_gpu_bank_refusals.py --record: every refusal of aeth_chan_* and aeth_synth_* by code and text",
                   "cases": _cases}, _f, indent=1)
        _f.write("\n")
    print(f"{len(_cases)} refusals recorded in {_path}")
