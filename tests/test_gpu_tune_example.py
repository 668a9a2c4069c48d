"""examples/tune.py end to end, in a child process: the tone lands within one bin of where the shift puts it, the chunks of
uneven length are the bits of one call, and the burst's EVM behind the mixer and the resampler is that of the same
composite signal planted without the offset and sent through the same resampler with no mixer, plus at most 3 dB.

The bound is measured in the same run, not chosen: both paths share the 16-tap filter, its stop band's leakage of the tone
and the f32 rounding of the resampler; only the shifter differs.  Its own error (below -140 dB, tests/test_gpu_nco.py) is
far under what the filter leaves, so the two figures agree closely.
Measured on an MI355X: burst EVM -50.41 dB with the mixer, -50.41 dB without it."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OFFSET, TONE, DOWN, N_BEFORE, N_AFTER = 0.2, -0.1, 4, 4096, 1024          # examples/tune.py


def test_tune_example_moves_the_tone_and_keeps_the_burst():
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "examples", "tune.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    print(r.stdout)
    assert "chunks equal one call: True" in r.stdout
    m = re.search(r"tone before ([-+][0-9.]+) cycles.*after ([-+][0-9.]+) cycles", r.stdout)
    f_in, f_out = float(m.group(1)), float(m.group(2))
    want = ((TONE - OFFSET) * DOWN + 0.5) % 1.0 - 0.5                     # -0.2 cycles per output sample
    assert abs(f_in - TONE) <= 1.0 / N_BEFORE, f_in
    assert abs(f_out - want) <= 1.0 / N_AFTER, (f_out, want)
    m = re.search(r"burst EVM ([-+]?[0-9.]+) dB; without the offset and without the mixer ([-+]?[0-9.]+) dB", r.stdout)
    evm, evm_plain = float(m.group(1)), float(m.group(2))
    assert evm <= evm_plain + 3.0, (evm, evm_plain)
