"""CPU: the Reed-Solomon algebra without a device.

  1. The restatement against itself: Euclid's decoder (tests/rs_truth.py, truth b) equals the exhaustive search by the
     definition (truth a) on RS(7, 3) and the shortened (6, 2) over GF(8), for every error pattern of weight <= 2 and on
     random words with 0 .. 4 errors and 0 .. 5 erasures.
  2. aeth_rs_generator, aeth_rs_host_encode and aeth_rs_host_decode against the truth for the catalogue, (15, 11),
     (15, 9), (15, 14) with r = 1, (15, 8) with odd r = 7, (255, 191) with r = 64 and n = r + 1; every encoded word
     evaluates to 0 at all r roots (the truth's own loop evaluates).  Decode cases: errors r div 2 and r div 2 + 1,
     erasures r and r + 1, mixes exactly on and one past 2 e + f = r, at depth 1 and interleaved."""
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from aether_primitives_amd import rs                  # noqa: E402
import rs_truth as T                                  # noqa: E402

GF8 = {"rs-7-3": (3, 0xb, 1, 1, 4, 7), "rs-6-2": (3, 0xb, 1, 1, 4, 6), "rs-7-3-fcr3-prim5": (3, 0xb, 3, 5, 4, 7), "rs-7-4": (3, 0xd, 0, 2, 3, 7)}

CODES = {name: tuple(getattr(rs.named(name), f) for f in ("m", "poly", "fcr", "prim", "nroots", "n"))
         for name in ("ccsds-255-223", "ccsds-255-239", "dvb-204-188", "rs-15-11")}
CODES.update({
    "rs-15-9": (4, 0x13, 2, 7, 6, 15),
    "rs-15-14": (4, 0x13, 1, 1, 1, 15),
    "rs-15-8": (4, 0x13, 0, 2, 7, 15),
    "rs-255-191": (8, 0x11d, 3, 1, 64, 255),
    "rs-5-4": (4, 0x13, 1, 1, 4, 5),
    "rs-65-64": (8, 0x11d, 0, 1, 64, 65),
    "rs-2-1": (3, 0xb, 0, 1, 1, 2),
})


def test_the_catalogue():
    assert CODES["ccsds-255-223"] == (8, 0x187, 112, 11, 32, 255)
    assert CODES["ccsds-255-239"] == (8, 0x187, 120, 11, 16, 255)
    assert CODES["dvb-204-188"] == (8, 0x11d, 0, 1, 16, 204)
    assert CODES["rs-15-11"] == (4, 0x13, 1, 1, 4, 15)


# ---- 1 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GF8))
def test_euclid_equals_the_exhaustive_search_on_every_pattern_up_to_weight_2(name):
    tr = T.Truth(GF8[name])
    rng = np.random.default_rng(3)
    base = tr.encode(rng.integers(0, 8, tr.k).astype(np.uint8))
    for w in (0, 1, 2):
        for pos in itertools.combinations(range(tr.n), w):
            for vals in itertools.product(range(1, 8), repeat=w):
                word = base.copy()
                for j, v in zip(pos, vals):
                    word[j] ^= v
                a, b = tr.decode_exhaustive(word), tr.decode_euclid(word)
                assert (a[0] == b[0]).all() and a[1:] == b[1:], (pos, vals)
                if 2 * w <= tr.r:
                    assert (a[0] == base).all() and a[1:] == (w, 0)


@pytest.mark.parametrize("name", sorted(GF8))
def test_euclid_equals_the_exhaustive_search_on_random_words(name):
    tr = T.Truth(GF8[name])
    rng = np.random.default_rng(4)
    W = 1500
    words = tr.encode(rng.integers(0, 8, W * tr.k).astype(np.uint8)).reshape(W, tr.n)
    bad, era = T.damage(rng, tr, words, rng.integers(0, 5, W), rng.integers(0, 6, W) * (rng.random(W) < 0.6), overlap=False)
    bad2, era2 = T.damage(rng, tr, words[:200], rng.integers(0, 3, 200), rng.integers(1, 4, 200), overlap=True)
    bad, era = np.concatenate([bad, bad2]), np.concatenate([era, era2])
    failed = 0
    for w in range(bad.shape[0]):
        a, b = tr.decode_exhaustive(bad[w], era[w]), tr.decode_euclid(bad[w], era[w])
        assert (a[0] == b[0]).all() and a[1:] == b[1:], (w, bad[w], era[w])
        failed += a[2]
    assert 0.2 <= failed / bad.shape[0] <= 0.7, failed


# ---- 2 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CODES) + sorted(GF8))
def test_generator_and_host_encode(name):
    code = CODES.get(name) or GF8[name]
    tr = T.Truth(code)
    g = rs.generator(code)
    assert list(g) == tr.generator() and g[-1] == 1 and g.size == tr.r + 1
    for root in tr.roots:
        assert tr._eval([int(v) for v in g], root) == 0
    rng = np.random.default_rng(len(name))
    for depth in (1, 3):
        data = rng.integers(0, 256, 4 * depth * tr.k).astype(np.uint8)   # bits above m are masked
        enc = rs.host_encode(code, data, depth)
        assert (enc == tr.encode(data, depth)).all()
        assert (enc.reshape(4, tr.n, depth)[:, :tr.k, :].ravel() == data & tr.N0).all(), "the data part is the input frame in place"
        assert not tr.syndromes(enc.reshape(4, tr.n, depth).transpose(0, 2, 1).reshape(-1, tr.n)).any(), "an encoded word has a non-zero syndrome"


def cases(r):
    """(errors, erasures) on both sides of the bound"""
    t = r // 2
    out = [(0, 0), (t, 0), (t + 1, 0), (0, r), (0, r + 1), (1, 0)]
    for f in sorted({1, 2, r // 2, r - 1} - {0}):
        if f < r:
            out += [((r - f) // 2, f), ((r - f) // 2 + 1, f)]
    return out


@pytest.mark.parametrize("name", sorted(CODES) + sorted(GF8))
def test_host_decode_on_both_sides_of_the_bound(name):
    code = CODES.get(name) or GF8[name]
    tr = T.Truth(code)
    rng = np.random.default_rng(len(name) + 50)
    spec = [c for c in cases(tr.r) if c[0] + c[1] <= tr.n] * (1 if tr.r > 16 else 3)
    W = len(spec) + (-len(spec)) % 3
    spec += [(0, 0)] * (W - len(spec))
    words = tr.encode(rng.integers(0, tr.N0 + 1, W * tr.k).astype(np.uint8)).reshape(W, tr.n)
    bad, era = T.damage(rng, tr, words, [c[0] for c in spec], [c[1] for c in spec])
    exhaustive = (tr.N0 + 1) ** tr.k <= 4096
    exp, corrected, status = tr.decode(bad.ravel(), era.ravel(), exhaustive=exhaustive)
    for w, (e, f) in enumerate(spec):
        if 2 * e + f <= tr.r:
            assert status[w] == 0 and corrected[w] <= e + f and (exp.reshape(W, tr.n)[w] == words[w]).all(), (e, f)
        elif f > tr.r:
            assert status[w] == 1
    assert status.any() and not status.all()
    for payload in (False, True):
        got, rec, summ = rs.host_decode(code, bad.ravel(), era.ravel(), 1, payload)
        nb = tr.k if payload else tr.n
        assert (got.reshape(W, nb) == exp.reshape(W, tr.n)[:, :nb]).all()
        assert (rec["corrected"] == corrected).all() and (rec["status"] == status).all()
        assert (int(summ["n_failed"]), int(summ["n_corrected"])) == (int(status.sum()), int(corrected.sum()))
    # the same words interleaved to depth 3: the same verdicts in the frame layout
    fr = lambda a: np.ascontiguousarray(a.reshape(W // 3, 3, -1).transpose(0, 2, 1)).ravel()        # noqa: E731
    got, rec, summ = rs.host_decode(code, fr(bad), fr(era), 3)
    assert (got == fr(exp.reshape(W, tr.n))).all() and (rec["status"] == status).all() and (rec["corrected"] == corrected).all()
    if not era.any():
        return
    got2, rec2, _ = rs.host_decode(code, fr(bad), None, 3)               # no erasure array: the flags are gone, not the damage
    exp2, c2, s2 = tr.decode(bad.ravel(), None, exhaustive=exhaustive)
    assert (got2 == fr(exp2.reshape(W, tr.n))).all() and (rec2["status"] == s2).all() and (rec2["corrected"] == c2).all()
