"""examples/fec.py end to end, in a child process: 2^16 bits through the K = 7 rate 1/2 code, QPSK with AWGN, the soft
demodulator and the Viterbi decoder.  The channel's raw hard-decision error share of the coded bits lies between 4 % and
7 % (about 4 dB Eb/N0), the noise-free pass decodes without an error, and the decoder leaves at most a hundredth of the
raw errors -- a condition with a wide margin, not a tuned number: the numpy restatement of the decoder left 0 errors in
65536 bits at this noise level for three seeds, against about 7300 raw errors."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fec_example_corrects_the_channel():
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "examples", "fec.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    print(r.stdout)
    m = re.search(r"raw errors (\d+) of (\d+) coded bits.*decoded errors (\d+), noise-free errors (\d+)", r.stdout)
    raw, ncoded, errors, quiet = (int(g) for g in m.groups())
    assert ncoded == 2 * 65536
    assert 0.04 <= raw / ncoded <= 0.07, raw / ncoded
    assert quiet == 0
    assert errors <= raw / 100, (errors, raw)
