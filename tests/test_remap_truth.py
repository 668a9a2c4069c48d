"""CPU: the library's host-only table builders (aeth_remap_puncture / _invert / _compose / _rows_cols / _bicm16) against
the plain loops of tests/remap_truth.py, and the properties that follow from the definitions."""
import numpy as np
import pytest

from aether_primitives_amd import remap
import remap_truth as rt


def same(got, want):
    assert got[1] == want[1], (got[1], want[1])
    assert got[0].dtype == np.int32 and np.array_equal(got[0], want[0])


@pytest.mark.parametrize("p", range(1, 13))
def test_puncture_equals_the_loop(p):
    rng = np.random.default_rng(100 + p)
    for _ in range(8):
        keep = rng.integers(0, 2, p, dtype=np.uint8)
        keep[rng.integers(0, p)] = 1                                  # never all zero
        keep = keep | (rng.integers(0, 2, p, dtype=np.uint8) << 1)    # only bit 0 counts
        same(remap.puncture_map(keep), rt.puncture(keep))


@pytest.mark.parametrize("rows,cols", ((1, 1), (1, 7), (7, 1), (3, 5), (32, 193)))
def test_rows_cols_equals_the_loop(rows, cols):
    same(remap.rows_cols_map(rows, cols), rt.rows_cols(rows, cols))
    m, r_in = remap.rows_cols_map(rows, cols)
    assert sorted(m.tolist()) == list(range(r_in))
    back, _ = remap.rows_cols_map(cols, rows)                         # the transpose undoes it
    same(remap.invert_map(m, r_in), (back, r_in))


@pytest.mark.parametrize("n_cbps,n_bpsc", ((48, 1), (96, 2), (192, 4), (288, 6)))
def test_bicm16_equals_the_loop_and_is_the_standards_interleaver(n_cbps, n_bpsc):
    same(remap.bicm16_map(n_cbps, n_bpsc), rt.bicm16(n_cbps, n_bpsc))
    m, r_in = remap.bicm16_map(n_cbps, n_bpsc)
    assert r_in == n_cbps and sorted(m.tolist()) == list(range(n_cbps)), "not a permutation"
    to, _ = remap.invert_map(m, n_cbps)                               # where coded bit k goes
    carrier = to // n_bpsc
    assert np.abs(np.diff(carrier)).min() >= 3, "adjacent coded bits on carriers less than 3 apart"
    if n_bpsc == 4:
        assert to[:4].tolist() == [0, 13, 24, 37]


def test_invert_twice_is_the_permutation():
    rng = np.random.default_rng(7)
    for n in (1, 2, 13, 192, 1000):
        perm = rng.permutation(n).astype(np.int32)
        inv, r = remap.invert_map(perm, n)
        same((inv, r), rt.invert(perm, n))
        same(remap.invert_map(inv, r), (perm, n))


def test_invert_takes_the_first_copy_and_marks_what_is_never_read():
    m = np.array([2, 2, 0, -1, 0, 4], np.int32)
    same(remap.invert_map(m, 6), (np.array([2, -1, 0, -1, 5, -1], np.int32), 6))
    same(remap.invert_map(m, 6), rt.invert(m, 6))


@pytest.mark.parametrize("keep", ([1, 1, 1, 0, 0, 1], [1, 1, 0, 1], [1, 0, 1, 1, 0, 1, 1, 0, 0, 1]))
def test_puncture_then_depuncture_is_the_identity_at_kept_positions(keep):
    pm, p = remap.puncture_map(keep)
    dm, d_in = remap.invert_map(pm, p)
    m, r_in = remap.compose_maps(pm, p, dm, d_in)
    assert r_in == p
    want = np.where(np.array(keep) & 1, np.arange(p), -1).astype(np.int32)
    assert np.array_equal(m, want)
    same((m, r_in), rt.compose(pm, p, dm, d_in))


def test_compose_of_6_to_4_and_192_to_192_has_periods_288_and_192():
    pm, p = remap.puncture_map([1, 1, 1, 0, 0, 1])
    im, i_in = remap.bicm16_map(192, 4)
    m, r_in = remap.compose_maps(pm, p, im, i_in)
    assert (r_in, m.size) == (288, 192)
    same((m, r_in), rt.compose(pm, p, im, i_in))
    # the composed map on data is one map after the other
    x = np.random.default_rng(3).integers(0, 256, 288 * 5, dtype=np.uint8)
    assert np.array_equal(rt.remap(x, m, r_in, 192 * 5), rt.remap(rt.remap(x, pm, p, 4 * 240), im, i_in, 192 * 5))


def test_compose_propagates_minus_one_and_repeats():
    rng = np.random.default_rng(11)
    for a_out, a_in, b_out, b_in in ((4, 6, 5, 3), (3, 5, 7, 2), (6, 4, 4, 9), (1, 1, 3, 2)):
        a = rng.integers(-1, a_in, a_out).astype(np.int32)
        b = rng.integers(-1, b_in, b_out).astype(np.int32)
        got = remap.compose_maps(a, a_in, b, b_in)
        same(got, rt.compose(a, a_in, b, b_in))
        m, r_in = got
        n_mid = 4 * a_out * b_in
        x = rng.integers(0, 256, n_mid // a_out * a_in, dtype=np.uint8)
        n_out = n_mid // b_in * b_out
        assert np.array_equal(rt.remap(x, m, r_in, n_out, 0x5a), rt.remap(rt.remap(x, a, a_in, n_mid, 0x5a), b, b_in, n_out, 0x5a))


def test_the_restatement_counts_its_inputs():
    m = np.array([3, -1, 0, 5, -1], np.int32)
    assert [rt.in_count(m, 7, n) for n in (0, 1, 2, 3, 4, 5, 6, 7)] == [0, 4, 4, 4, 6, 7, 11, 11]
    x = np.arange(14, dtype=np.uint8)
    assert rt.remap(x, m, 7, 7, 0xee).tolist() == [3, 0xee, 0, 5, 0xee, 10, 0xee]
