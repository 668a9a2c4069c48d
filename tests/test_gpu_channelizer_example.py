"""examples/channelizer.py runs end to end as a program: the two tone channels of the 16-channel bank stand out, and the
Hann-windowed, overlapped spectrogram leaks less three bins off the tone than the rectangular framing."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_channelizer_example_separates_the_tones_and_the_window_cuts_the_leakage(ctx):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "examples", "channelizer.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    print(r.stdout)
    rows = re.findall(r"^channel\s+(\d+):\s+(-?[\d.]+) dB(  <- tone)?$", r.stdout, re.M)
    assert [int(k) for k, _, _ in rows] == list(range(16))
    tones = [float(v) for _, v, t in rows if t]
    others = [float(v) for _, v, t in rows if not t]
    assert len(tones) == 2 and {int(k) for k, _, t in rows if t} == {3, 11}
    assert min(tones) >= max(others) + 20.0, r.stdout
    m = re.search(r"leakage three bins off the tone: hann (-?[\d.]+) dB, rectangular (-?[\d.]+) dB", r.stdout)
    assert m, r.stdout
    assert float(m.group(1)) < float(m.group(2)), r.stdout
