"""examples/clock.py end to end: through the conversion from 48 kHz to 44.1 kHz * (1 + 20 ppm) the tone lands in the bin
its frequency and the new clock give, and the chunks of uneven length, with history and carried phase, are the bits of one
call.  The spur level is printed and recorded (profiles/arb_bw.txt), not asserted."""
import importlib.util
import os

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_clock_example_keeps_the_tone_and_its_chunks_are_one_call(ctx):
    spec = importlib.util.spec_from_file_location("example_clock", os.path.join(ROOT, "examples", "clock.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    f_in, f_out, k_out, spur_db, f_spur, same = ex.main()
    assert same
    n_out = ex.FS_NOMINAL // ex.BIN_HZ
    assert k_out == round(ex.TONE_HZ * n_out / ex.FS_OUT) == 1500     # 1499.97: the new clock moves the tone off the bin centre
    assert abs(f_in - ex.TONE_HZ) <= ex.BIN_HZ and abs(f_out - ex.TONE_HZ) <= ex.BIN_HZ
    print(f"strongest spur {spur_db:.1f} dB at {f_spur:.1f} Hz (recorded, not asserted)")
