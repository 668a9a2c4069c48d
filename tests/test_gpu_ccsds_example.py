"""examples/ccsds.py as it ships: RS(255, 223) at depth 4 around the K = 7 convolutional code, QPSK and AWGN.

At the example's noise the Viterbi decoder leaves byte errors, every record says status = 0 and the payload equals the
sent bytes.  At a second, higher level (0.86: the CPU restatement of the inner code puts between 7 and 22 byte errors
into a codeword there) the failed codewords are exactly those in which the frames behind the Viterbi decoder differ from
the sent ones in more than 16 bytes, the others are repaired, and the summary counts both.  The byte errors are counted
here from the frames the example hands out with diagnose=True."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIGHER = 0.86


@pytest.fixture(scope="module")
def example():
    spec = importlib.util.spec_from_file_location("ccsds_example", os.path.join(ROOT, "examples", "ccsds.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def byte_errors(res, example):
    """per codeword, frame by frame: the bytes in which the frames behind the Viterbi decoder differ from the sent ones"""
    F = example.FRAMES
    diff = (res["received"] != res["coded"]).reshape(F, 255, example.DEPTH)
    return diff.sum(axis=1).ravel()


def test_the_outer_code_repairs_what_the_viterbi_decoder_leaves(example):
    res = example.main(diagnose=True)
    errs = byte_errors(res, example)
    print("byte errors per codeword", errs.tolist())
    assert errs.sum() >= 1, "the Viterbi decoder left nothing to repair: the example shows nothing"
    assert errs.max() <= 16
    assert not res["records"]["status"].any()
    assert res["records"]["corrected"].tolist() == errs.tolist()
    assert res["payload"].tobytes() == res["sent"].tobytes()
    assert (int(res["summary"]["n_failed"]), int(res["summary"]["n_corrected"])) == (0, int(errs.sum()))


def test_beyond_sixteen_byte_errors_a_codeword_fails_and_is_left_alone(example):
    res = example.main(power=HIGHER, diagnose=True)
    errs = byte_errors(res, example)
    print("byte errors per codeword", errs.tolist())
    failed = res["records"]["status"] != 0
    assert failed.tolist() == (errs > 16).tolist()
    assert int(res["summary"]["n_failed"]) == int((errs > 16).sum())
    assert res["records"]["corrected"].tolist() == np.where(errs > 16, 0, errs).tolist()
    assert int(res["summary"]["n_corrected"]) == int(errs[errs <= 16].sum())
    F, I = example.FRAMES, example.DEPTH
    got = res["payload"].reshape(F, 223, I)
    exp = np.where(failed.reshape(F, 1, I), res["received"].reshape(F, 255, I)[:, :223], res["sent"].reshape(F, 223, I))
    assert (got == exp).all(), "a repaired codeword is the sent one, a failed one comes through as received"
