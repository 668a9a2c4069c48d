"""examples/dsss.py runs end to end: 64 bits -> BPSK -> spread by the order-7 m-sequence -> AWGN -> correlator -> bits;
and the chips the device makes for the template are the m-sequence examples/sync.py builds on the host."""
import os
import runpy

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
EX = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples")


def test_dsss_example_recovers_every_bit(ctx):
    data, got, peaks, chips = runpy.run_path(os.path.join(EX, "dsss.py"))["main"]()
    assert data.size == 64 and 0 < data.sum() < 64
    assert (got == data).all()
    assert peaks.size == 64
    # a clean peak is 127 * (+-1); the noise (deviation `power` = 1 per component and chip, noise.rs:41-42,58) adds a real
    # part of deviation sqrt(127) = 11.3: six deviations either way
    assert (np.abs(peaks.real) > 127 - 68).all() and (np.abs(peaks.real) < 127 + 68).all()
    sync = runpy.run_path(os.path.join(EX, "sync.py"))
    assert chips.dtype == np.complex64 and (chips.view(np.uint32) == sync["m_sequence"]().view(np.uint32)).all()
