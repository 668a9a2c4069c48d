"""examples/wifi.py end to end, in a child process: 2880 bits in 20 OFDM symbols through the scrambler, the K = 7 code, one
288 -> 192 rate-matching map (puncture 3/4, then the 802.11a interleaver), Gray 16-QAM and the OFDM framing, AWGN, and the
way back through the inverse map (erasures where bits were punctured) and the Viterbi decoder.

The noise-free pass decodes without an error: that follows from the definitions.  The noise power 0.144 was chosen on the
CPU with the restatements (tests/cc_truth.py for the code, the soft demodulator and the decoder at block 512, warm-up 64,
traceback 64; tests/remap_truth.py for the maps; numpy for the scrambler, the table and the noise, added per carrier: the
OFDM framing is unitary).  Raw errors of the 3840 bits on the air and decoded errors there, data seeds 815, 816, 817:

    power 0.144:  48 -> 0,   34 -> 0,   43 -> 0          (0.16: 75, 66, 64 -> 0;  0.18: 123, 114, 109 -> 0;
                                                           0.20: 172, 162, 161 -> 30, 2, 9)

so the decoder is two steps of noise away from its first error.  The raw share has the closed form 3/4 Q(1 / (sqrt(10)
0.144)) = 1.05 %, 40.5 of 3840; a binomial count of that mean has a deviation of 6.3, and the window below is five
deviations either side, 9 .. 72 errors (0.23 % .. 1.88 %), which a different noise generator stays inside.  With fewer
than 100 raw errors, `decoded <= raw / 100` means no decoded error at all."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_wifi_example_corrects_the_channel():
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.join(ROOT, "examples", "wifi.py")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    print(r.stdout)
    m = re.search(r"(\d+) bits in (\d+) OFDM symbols.*one (\d+) -> (\d+) map.*raw errors (\d+) of (\d+) bits on the air.*"
                  r"decoded errors (\d+), noise-free errors (\d+)", r.stdout)
    nbits, n_sym, r_in, r_out, raw, nair, errors, quiet = (int(g) for g in m.groups())
    assert (nbits, n_sym, r_in, r_out, nair) == (144 * 20, 20, 288, 192, 192 * 20)
    assert quiet == 0
    assert raw > 0
    assert 9 <= raw <= 72, raw / nair
    assert errors <= raw / 100, (errors, raw)
