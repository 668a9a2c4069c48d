"""examples/polar_list.py as it ships (256 frames of 240 + 16 bits in the (9, 256) code, the link of examples/polar.py):
for L = 1, 2, 4, 8 the device's rows, records and `which` are held against the restatement tests/polar_list_truth.py on
the soft values the device made, with crc-16/xmodem computed on the host (binascii.crc_hqx).  Then the link itself: the
L = 1 count equals the number of frames whose plain SC payload is wrong, every frame whose picked payload equals the sent
one was called good, and fewer frames are wrong at L = 8 than at L = 1.  The counts are printed."""
import binascii
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import polar_truth as T                                # noqa: E402
import polar_list_truth as LT                          # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(HERE)


def crc_passes(rows, payload):
    """[R] bool: the 16 check bits of a row (highest coefficient first) equal crc-16/xmodem of its payload bits"""
    ok = np.zeros(rows.shape[0], bool)
    weights = 1 << np.arange(15, -1, -1)
    for r in range(rows.shape[0]):
        ok[r] = binascii.crc_hqx(np.packbits(rows[r, :payload]).tobytes(), 0) == int((rows[r, payload:].astype(np.int64) * weights).sum())
    return ok


def test_polar_list_example_lets_the_crc_pick():
    spec = importlib.util.spec_from_file_location("polar_list_example", os.path.join(ROOT, "examples", "polar_list.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    res = example.main()
    F, P, K, N = 256, 240, 256, 512
    msk, sent, soft = res["mask"], res["sent"].reshape(F, P), res["soft"]
    assert soft.size == F * N and int(msk.sum()) == K and msk.tobytes() == T.mask(9, K).tobytes()
    assert sorted(res["lists"]) == [1, 2, 4, 8]
    for L, got in sorted(res["lists"].items()):
        rows, rec = LT.decode(msk, soft, L, LT.ALL)
        rows = rows.reshape(F, L, K)
        assert got["rows"].tobytes() == rows.tobytes(), L
        assert got["records"].tobytes() == rec.tobytes(), L
        ok = crc_passes(rows.reshape(F * L, K), P).reshape(F, L)
        payload, which = LT.pick(rows[:, :, :P], P, L, (~ok).astype(np.uint64))
        assert got["which"].tolist() == which.tolist(), L
        assert got["payload"].tobytes() == payload.tobytes(), L
        right = (got["payload"] == sent).all(axis=1)
        assert not (right & (got["which"] == LT.NONE)).any(), f"L = {L}: a frame with the sent payload that no row's CRC passed"
        assert got["none"] == int((which == LT.NONE).sum()) and got["wrong"] == int((~right).sum())
        assert got["wrong0"] == int((rows[:, 0, :P] != sent).any(axis=1).sum())
        print(f"L = {L}: no row passes {got['none']}, wrong after the pick {got['wrong']}, wrong if row 0 is taken {got['wrong0']}")
    print("plain SC wrong", res["sc_wrong"])
    assert res["lists"][1]["wrong"] == res["sc_wrong"] == res["lists"][1]["wrong0"]
    assert res["lists"][8]["wrong"] < res["lists"][1]["wrong"]
