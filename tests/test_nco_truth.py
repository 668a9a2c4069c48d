"""CPU: the numpy restatement of the oscillator (tests/nco_truth.py) against exp(2 pi j w / 2^64) in complex128 under the
bound of aeth_fft_exec (-120 dB, tests/test_gpu_fft.py), the cardinal words, the word arithmetic against Python integers
at positions up to 2^64 - 1, and chunks concatenating bit for bit."""
import numpy as np

import nco_truth
from helpers import bits_equal, rand_c64

TOL_DB = -120.0                                   # tests/test_gpu_fft.py:20

WORDS = (0x123456789abcdef0, 0xfedcba9876543211, 0x0f0f0f0f0f0f0f0f)
POSITIONS = (0, 1, 2, 3, 2 ** 31 + 5, 2 ** 40 + 7, 2 ** 63 + 1, 2 ** 64 - 1)


def db(got, want):
    return 20 * np.log10(np.linalg.norm(np.asarray(got).astype(np.complex128) - want) / np.linalg.norm(want))


def test_restatement_against_complex128():
    rng = np.random.default_rng(1)
    w = rng.integers(0, 2 ** 64, 1 << 14, dtype=np.uint64)
    c, d = nco_truth.phasor(w)
    assert c.dtype == np.float32 and d.dtype == np.float32
    truth = nco_truth.phasor_f64(w.tolist())
    got = c.astype(np.float64) + 1j * d.astype(np.float64)
    e_ph, worst = db(got, truth), float(np.abs(got - truth).max())
    # the mix of unit-variance data: every word of a chirp that wraps many times
    words = (WORDS[0], WORDS[1], 2 ** 50 + 12345)
    x = rand_c64(7, 1 << 14)
    n0 = 2 ** 40 + 7
    y = nco_truth.mix(words, n0, x)
    ytruth = x.astype(np.complex128) * nco_truth.phasor_f64([nco_truth.word_int(words, n0 + i) for i in range(x.size)])
    e_mix = db(y, ytruth)
    t = nco_truth.tone(words, n0, 0.75, 4096)
    e_tone = db(t, 0.75 * nco_truth.phasor_f64([nco_truth.word_int(words, n0 + i) for i in range(4096)]))
    print(f"phasor {e_ph:.1f} dB (largest error {worst:.3g}), mix {e_mix:.1f} dB, tone {e_tone:.1f} dB")
    assert e_ph <= TOL_DB and e_mix <= TOL_DB and e_tone <= TOL_DB, (e_ph, e_mix, e_tone)


def test_cardinal_words_are_exact():
    c, d = nco_truth.phasor(np.array([0, 1 << 62, 1 << 63, 3 << 62], np.uint64))
    want_c = np.array([1.0, -0.0, -1.0, 0.0], np.float32)
    want_d = np.array([0.0, 1.0, -0.0, -1.0], np.float32)
    assert c.view(np.uint32).tolist() == want_c.view(np.uint32).tolist()
    assert d.view(np.uint32).tolist() == want_d.view(np.uint32).tolist()


def test_words_equal_python_integers():
    for words in (WORDS, (0, 0, 0), (2 ** 64 - 1,) * 3, (5, 2 ** 63, 2 ** 63), (0, 1, 1)):
        got = nco_truth.words_at(words, np.array(POSITIONS, np.uint64))
        for n, g in zip(POSITIONS, got.tolist()):
            p, s, r = words
            assert g == (p + n * s + (n * (n - 1) // 2) * r) % 2 ** 64, (words, n)
            assert g == nco_truth.word_int(words, n)
    # consecutive positions: the first difference is step + n * rate
    w = nco_truth.words_at(WORDS, nco_truth.positions(2 ** 63 - 2, 5)).tolist()
    for i in range(4):
        n = 2 ** 63 - 2 + i
        assert (w[i + 1] - w[i]) % 2 ** 64 == (WORDS[1] + n * WORDS[2]) % 2 ** 64


def test_chunks_concatenate_bit_for_bit():
    x = rand_c64(3, 1500)
    for n0 in (0, 2 ** 32 - 100, 2 ** 64 - 1 - x.size):
        whole = nco_truth.mix(WORDS, n0, x)
        twhole = nco_truth.tone(WORDS, n0, 1.25, x.size)
        for cut in (1, 2, 255, 256, 257, 733):
            parts = np.concatenate([nco_truth.mix(WORDS, n0, x[:cut]), nco_truth.mix(WORDS, n0 + cut, x[cut:])])
            assert bits_equal(parts, whole), (n0, cut)
            tparts = np.concatenate([nco_truth.tone(WORDS, n0, 1.25, cut), nco_truth.tone(WORDS, n0 + cut, 1.25, x.size - cut)])
            assert bits_equal(tparts, twhole), (n0, cut)
