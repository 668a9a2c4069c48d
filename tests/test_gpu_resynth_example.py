"""examples/resynth.py runs end to end as a program: analysis followed by synthesis with the dual window returns the
stream within the round-trip bound of tests/test_gpu_synth.py, and zeroing the tone's bins takes the tone out.

The mask is five bins wide around a tone at a bin centre: the periodic Hann window puts such a tone into three bins, so
away from the stream's first frames nothing of it is left and the tone's bin of the long transform falls to what the
notched QPSK leaves there; 40 dB is far inside that (the tone alone stands 20 dB + 10 log10(32768) = 65 dB above the
QPSK's level per bin)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resynth_example_returns_the_stream_and_removes_the_tone(ctx):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "examples", "resynth.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    print(r.stdout)
    m = re.search(r"round trip of \d+ samples through \d+ frames: EVM (-?[\d.]+) dB", r.stdout)
    assert m, r.stdout
    assert float(m.group(1)) <= -114.0, r.stdout
    m = re.search(r"tone level before (-?[\d.]+) dB, after (-?[\d.]+) dB: (-?[\d.]+) dB down", r.stdout)
    assert m, r.stdout
    before, after, drop = (float(g) for g in m.groups())
    print(f"measured drop {drop:.1f} dB")
    assert before - after >= 40.0 and drop >= 40.0, r.stdout
