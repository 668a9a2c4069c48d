"""The definition of the averaged spectra (include/aether_hip.h, "averaged spectra") restated in numpy, for the tests of
aeth_vec_frame_sums and aeth_chan_exec_sums.  Every f64 addition is written out in the order of the contract: a chunk's
frames in ascending order, then a row's chunk sums in ascending order; the max skips NaN."""
import numpy as np


def level_q(frames):
    """q of every sample: (double)re * re + (double)im * im, both products exact, one rounding"""
    f = np.asarray(frames, np.complex64)
    re, im = f.real.astype(np.float64), f.imag.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        return re ** 2 + im ** 2


def rows_of(F, block):
    """[(first frame, one past the last)] of every row"""
    B = F if block == 0 or block > F else block
    return [(r, min(F, r + B)) for r in range(0, F, B)]


def frame_sums(frames, length, block, chunk):
    """frames: F * length complex64 -> (sum, max), float64 arrays of shape (rows, length)"""
    q = level_q(frames).reshape(-1, length)
    F = q.shape[0]
    assert F >= 1 and chunk >= 1
    sums, maxs = [], []
    with np.errstate(over="ignore", invalid="ignore"):
        for r0, r1 in rows_of(F, block):
            row = None
            for c0 in range(r0, r1, chunk):
                part = q[c0].copy()                              # a chunk's sum starts from its first frame
                for m in range(c0 + 1, min(c0 + chunk, r1)):
                    part = part + q[m]
                row = part if row is None else row + part       # the row's sum starts from chunk 0's sum
            best = np.full(length, -np.inf)
            for m in range(r0, r1):
                best = np.where(q[m] > best, q[m], best)         # a NaN q never enters
            sums.append(row)
            maxs.append(best)
    return np.array(sums), np.array(maxs)


def same_plane(got, want):
    """byte for byte, except that any NaN equals any NaN (the payload of a NaN is not part of the contract)"""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    if got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    return bool((gn == wn).all() and (got.view(np.uint64)[~gn] == want.view(np.uint64)[~wn]).all())


def burst_then_noise(seed, F, length, burst_at=(0, 9, 10)):
    """1e-3 noise in every frame and a burst of amplitude 3e9 in a few of them: sums whose low bits depend on the order"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((F, length)) + 1j * rng.standard_normal((F, length))) * 1e-3
    for m in burst_at:
        if m < F:
            x[m] += (rng.standard_normal(length) + 1j * rng.standard_normal(length)) * 3e9
    return x.astype(np.complex64).reshape(-1)
