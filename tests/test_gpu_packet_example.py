"""examples/packet.py at a reduced size (48 frames of 64 bytes): payload bytes -> bits -> crc-32 attach -> scrambler ->
K = 7 code -> QPSK -> AWGN -> soft demodulation -> Viterbi -> descrambler -> one check with payload strip -> packed bytes.

At the clean level the summary counts no bad frame and every packed payload equals the sent bytes.  At the noisy level no
count is fixed in advance: frame by frame, the CRC calls a frame good exactly when its decoded bits -- payload and check
bits -- equal the sent ones (an undetected error would need a 2^-32 coincidence), a good frame's decoded payload equals
the sent one, the summary counts what the diff words show, and the good payloads that left the device equal the sent
bytes.  (A frame whose payload is intact and whose check bits took the errors is bad by any CRC: in the reduced run frame 8
has diff 0x2c0.  So "good exactly when the payload is intact" holds in one direction only, and the frame is compared.)"""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_packet_example_verdicts_match_the_decoded_payloads():
    spec = importlib.util.spec_from_file_location("packet_example", os.path.join(ROOT, "examples", "packet.py"))
    packet = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(packet)
    F, N = 48, 64
    clean, noisy = packet.main(n_frames=F, n_bytes=N)
    data = clean["data"]
    sent = lambda f: data[f * N:(f + 1) * N].tobytes()
    assert clean["summary"] == (0, F) and not clean["diff"].any() and not clean["differ"].any()
    assert sorted(clean["good"]) == list(range(F)) and all(clean["good"][f].tobytes() == sent(f) for f in range(F))
    for res in (clean, noisy):
        bad = np.flatnonzero(res["diff"])
        print(res["power"], "bad by CRC", bad.size, "decoded frame differs", int(res["differ"].sum()), "payload differs", int(res["differ_payload"].sum()))
        for f in range(F):
            assert (res["diff"][f] == 0) == (not res["differ"][f]), f
            assert res["diff"][f] != 0 or not res["differ_payload"][f], f
        assert res["summary"] == (bad.size, int(bad[0]) if bad.size else F)
        assert sorted(res["good"]) == [f for f in range(F) if res["diff"][f] == 0]
        assert all(p.tobytes() == sent(f) for f, p in res["good"].items())
