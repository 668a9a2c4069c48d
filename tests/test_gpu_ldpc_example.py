"""examples/ldpc.py as it ships (64 codewords of staircase(12, 24, 81)): encode -> QPSK -> AWGN -> soft demodulation ->
decode with early stop.

First the device's bytes are held against the restatement tests/ldpc_truth.py on the soft values the device made: the
coded bits, the decoded payload and every record.  Then the link itself: the hard decisions in front of the decoder hold
errors, none is left behind it, and every record says unsatisfied = 0."""
import importlib.util
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import ldpc_truth as T                                # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(HERE)


def test_ldpc_example_decodes_every_codeword():
    spec = importlib.util.spec_from_file_location("ldpc_example", os.path.join(ROOT, "examples", "ldpc.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    res = example.main()
    shift, z = res["shift"], res["z"]
    F = 64
    assert res["sent"].size == F * 972 and res["soft"].size == F * 1944
    assert res["coded"].tobytes() == T.encode(shift, z, res["sent"]).tobytes()
    bits, rec = T.decode(shift, z, res["soft"], example.MAX_ITER, T.EARLY | T.PAYLOAD)
    assert res["bits"].tobytes() == bits.tobytes()
    assert res["records"]["iterations"].tolist() == rec[:, 0].tolist() and res["records"]["unsatisfied"].tolist() == rec[:, 1].tolist()
    print("raw errors", res["raw"], "after decoding", res["wrong"], "iterations", sorted(set(rec[:, 0].tolist())))
    assert res["raw"] > 0
    assert res["wrong"] == 0 and res["bits"].tobytes() == res["sent"].tobytes()
    assert not res["records"]["unsatisfied"].any()
