"""examples/psd.py runs end to end as a program: the averaged spectrum of 2048 frames shows the tone at bin 200 that a
single frame hides, some 4 dB over a noise floor of 3 M / 8."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_psd_example_finds_the_tone_in_the_average(ctx):
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "examples", "psd.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    print(r.stdout)
    assert "2048 frames of 1024 bins, route fused" in r.stdout
    m = re.search(r"largest bin of the averaged spectrum: (\d+)", r.stdout)
    assert m and int(m.group(1)) == 200, r.stdout
    m = re.search(r"largest bin of one frame alone: (\d+)", r.stdout)
    assert m and int(m.group(1)) != 200, r.stdout              # the seed of the example: one frame does not show it
    m = re.search(r"noise floor (-?[\d.]+) dB \(3 M / 8 is (-?[\d.]+) dB\), tone (-?[\d.]+) dB over it", r.stdout)
    assert m, r.stdout
    floor, ideal, over = (float(g) for g in m.groups())
    # 1 + 655 / 384 is 4.3 dB; the mean of 2048 half-overlapped frames is within a few per cent of its expectation
    assert abs(floor - ideal) < 0.3 and 3.5 < over < 5.0, r.stdout
