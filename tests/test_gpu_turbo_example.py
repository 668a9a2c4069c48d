"""examples/turbo.py as it ships (64 frames of 488 + 24 bits in the LTE code at K = 512): CRC attach -> encode -> QPSK -> AWGN
-> soft demodulation -> decode with early stop at max_iter = 1, 2, 4, 8 -> CRC check.

First the device's bytes are held against the restatement tests/turbo_truth.py on the soft values the device made: the
coded bits, and every round's decisions and records.  Then the link itself: in every round the frames the CRC calls good
are exactly those whose payload equals the sent one; and the two conditions the noise level was chosen for: at least one
frame fails the CRC after one iteration and passes after eight, and at least one frame stops before the eighth."""
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import turbo_truth as T                                # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(HERE)


def test_turbo_example_converges_frame_by_frame():
    spec = importlib.util.spec_from_file_location("turbo_example", os.path.join(ROOT, "examples", "turbo.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    res = example.main()
    F, L, K = 64, 488, 512
    code = T.named("lte")
    N = 3 * K + 4 * code.nu
    pi, sent, soft = res["pi"], res["sent"].reshape(F, L), res["soft"]
    assert res["sent"].size == F * L and soft.size == F * N
    assert pi.tolist() == T.qpp(K, 31, 64).tolist()
    frames = res["coded"].reshape(F, N)[:, :K]                        # the frames with their check bits: the systematic plane
    assert frames[:, :L].tobytes() == sent.tobytes()
    assert res["coded"].tobytes() == T.encode(code, pi, frames.ravel()).tobytes()

    history = []
    T.decode(code, pi, example.WINDOW, example.WARMUP, soft, 8, 0, None, history)
    rounds = res["rounds"]
    assert [rd["max_iter"] for rd in rounds] == [1, 2, 4, 8]
    for rd in rounds:
        bits, rec = T.from_history(history, rd["max_iter"], T.EARLY)
        assert rd["bits"].tobytes() == bits.tobytes(), rd["max_iter"]
        assert rd["records"].tobytes() == rec.tobytes(), rd["max_iter"]
        right = (rd["bits"].reshape(F, K)[:, :L] == sent).all(axis=1)
        assert (~rd["bad"]).tolist() == right.tolist(), f"max_iter {rd['max_iter']}: the CRC's verdict differs from the payload's"
    print("raw errors", res["raw"], "failed frames per round", res["failed"], "mean iterations", res["mean_iter"])
    assert res["raw"] > 0
    assert (rounds[0]["bad"] & ~rounds[-1]["bad"]).any(), "no frame fails after one iteration and passes after eight"
    assert (rounds[-1]["records"]["iterations"] < 8).any(), "no frame stops before the eighth iteration"
    assert res["wrong"] == 0
    good = ~rounds[-1]["bad"]
    assert res["payload"][good].tobytes() == sent[good].tobytes()
