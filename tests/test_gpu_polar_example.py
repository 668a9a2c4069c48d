"""examples/polar.py as it ships (256 frames of 240 + 16 bits in the (9, 256) code): CRC attach -> encode -> QPSK -> AWGN ->
soft demodulation -> decode with records -> CRC check, then the flip rounds.

First the device's bytes are held against the restatement tests/polar_truth.py on the soft values the device made: the
coded bits, and every round's decisions and records under that round's flips.  Then the link itself: after each round the
frames the CRC calls good are exactly those whose payload equals the sent one, and the set of failed frames never grows;
there are raw errors, at least one frame fails the first pass, and fewer fail after the last round."""
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import polar_truth as T                                # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(HERE)


def test_polar_example_repairs_frames_by_flipping():
    spec = importlib.util.spec_from_file_location("polar_example", os.path.join(ROOT, "examples", "polar.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    res = example.main()
    F, L, K, N = 256, 240, 256, 512
    msk, sent, soft = res["mask"], res["sent"].reshape(F, L), res["soft"]
    assert res["sent"].size == F * L and soft.size == F * N and int(msk.sum()) == K
    assert msk.tobytes() == T.mask(9, K).tobytes()
    frames = T.decode(msk, T.soft_of_bits(res["coded"]))[0]         # the frames with their check bits, from the noise-free codewords
    assert frames.reshape(F, K)[:, :L].tobytes() == sent.tobytes()
    assert res["coded"].tobytes() == T.encode(msk, frames).tobytes()

    rounds = res["rounds"]
    assert 2 <= len(rounds) <= example.ROUNDS + 1
    first = rounds[0]["records"]
    prev_bad = None
    for r, rd in enumerate(rounds):
        flip = rd["flip"]
        if r == 0:
            assert (flip == T.NONE).all()
        else:
            was_bad = rounds[r - 1]["bad"]
            assert (flip[was_bad] == first["index"][was_bad, r - 1]).all() and (flip[~was_bad] == rounds[r - 1]["flip"][~was_bad]).all()
        bits, rec = T.decode(msk, soft, flip)
        assert rd["bits"].tobytes() == bits.tobytes(), r
        assert rd["records"].tobytes() == rec.tobytes(), r
        right = (rd["bits"].reshape(F, K)[:, :L] == sent).all(axis=1)
        assert (~rd["bad"]).tolist() == right.tolist(), f"round {r}: the CRC's verdict differs from the payload's"
        if prev_bad is not None:
            assert not (rd["bad"] & ~prev_bad).any(), f"round {r}: a frame that was good fails"
        prev_bad = rd["bad"]
    print("raw errors", res["raw"], "failed frames per round", res["failed"], "wrong payloads", res["wrong"])
    assert res["raw"] > 0
    assert res["failed"][0] >= 1
    assert res["failed"][-1] < res["failed"][0]
    assert res["wrong"] == res["failed"][-1]
    good = ~rounds[-1]["bad"]
    assert res["payload"][good].tobytes() == sent[good].tobytes()
