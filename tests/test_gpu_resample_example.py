"""examples/resample.py end to end: the tone keeps its frequency in Hz through the 48 kHz -> 44.1 kHz conversion, the
chunks with history are the bits of one call, and the strongest image of the zero stuffing is no stronger than the
prototype's own stop-band says.

The bound is computed here, not chosen: zero stuffing by U puts copies of the tone at f0 + m * fs_in (m = 1 .. U - 1, or
-U/2 .. U/2 without 0) in the upsampled stream, each scaled like the tone itself; the filter H leaves |H(f0 + m fs_in)| /
|H(f0)| of copy m relative to the tone, and picking every Q-th sample moves it to (f0 + m fs_in) mod fs_out without
changing its level.  No two copies share a bin (U and Q are coprime).  H is evaluated in f64 from the f32 taps; 3 dB are
added for the finite-length estimate (4410 points of a stream whose rounding errors also land in that bin)."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_resample_example_keeps_the_tone_and_holds_the_stop_band(ctx):
    spec = importlib.util.spec_from_file_location("example_resample", os.path.join(ROOT, "examples", "resample.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    f_in, f_out, image_db, f_img, same = ex.main()
    assert same
    assert abs(f_in - ex.TONE_HZ) <= ex.BIN_HZ and abs(f_out - ex.TONE_HZ) <= ex.BIN_HZ and abs(f_out - f_in) <= ex.BIN_HZ

    from aether_primitives_amd import resamp
    h = resamp.prototype(ex.UP, ex.DOWN, ex.TAPS_PER_PHASE).astype(np.float64)
    fs_up = ex.FS_IN * ex.UP
    k = np.arange(h.size)

    def gain(f):
        return abs(np.sum(h * np.exp(-2j * np.pi * f * k / fs_up)))

    copies = [m for m in range(-(ex.UP // 2), ex.UP // 2 + 1) if m]
    levels = [20 * np.log10(gain(ex.TONE_HZ + m * ex.FS_IN) / gain(ex.TONE_HZ)) for m in copies]
    worst = int(np.argmax(levels))
    f_alias = (ex.TONE_HZ + copies[worst] * ex.FS_IN) % ex.FS_OUT
    f_alias = f_alias if f_alias < ex.FS_OUT / 2 else f_alias - ex.FS_OUT
    print(f"measured image {image_db:.1f} dB at {f_img:.1f} Hz; the prototype's stop-band gives {levels[worst]:.1f} dB at {f_alias:.1f} Hz "
          f"(copy m = {copies[worst]})")
    assert image_db <= levels[worst] + 3.0, (image_db, levels[worst])
    assert abs(f_img - f_alias) <= ex.BIN_HZ, (f_img, f_alias)
