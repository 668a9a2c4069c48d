"""examples/spectrum.py (the device counterpart of `spectrum` / `waterfall`, src/util/plot.rs:36-68, :102-130) runs end to
end: the planted tone is the peak the device reports, and the waterfall holds the reference's levels."""
import os
import runpy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
EX = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")


def test_spectrum_example(ctx):
    water, st, peak_bin = runpy.run_path(os.path.join(EX, "spectrum.py"))["main"](fft_len=2048, frames=64, tone_bin=300)
    assert water.shape == (64, 2048) and water.dtype == np.float32 and np.isfinite(water).all()
    # the tone: amplitude 4 * sqrt(2048) after Scale::SN, far above noise of power 2 per bin; mirrored to bin 300 + 1024
    assert peak_bin == 300 and st.max_index == 1324 and st.n == 2048 and st.n_nan == 0
    assert abs(st.max_norm / (4 * np.sqrt(2048)) - 1) < 0.05
    assert (water.argmax(axis=1) == 1324).all()
    # noise bins: 10 log10 of an amplitude whose square has mean 2 -> median 5 log10(2 ln 2) = 0.71 "dB" (the reference's quirk), not 3
    assert abs(np.median(water) - 5 * np.log10(2 * np.log(2))) < 0.3
    # power per bin: noise 2 + the tone's 16 * 2048 / 2048
    assert abs(st.power - 18) < 1.5
