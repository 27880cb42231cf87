"""tests/isoforms_ref.py against hand-computed cases, and mmseq_amd.isoforms.switch_probability against a count over all pairs of
draws.  No device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isoforms_ref as R  # noqa: E402


def test_two_equal_members():
    tr = np.array([[2.0, 0.5, 7.0], [2.0, 0.5, 7.0]])
    r = R.isoforms_ref(tr, [[0, 1]], thresholds=[0.1], ranks=[0, 2])
    assert np.array_equal(r["H"][0], np.full(3, -(0.5 * np.log(0.5) + 0.5 * np.log(0.5)))) and np.allclose(r["H"][0], np.log(2.0), rtol=0, atol=1e-15)
    assert np.array_equal(r["top"][0], [0, 0, 0]) and np.array_equal(r["second"][0], [1, 1, 1])      # the first of equals is the top
    assert np.array_equal(r["P"][0], [0.5, 0.5, 0.5])
    assert np.array_equal(r["n_top"], [3, 0]) and np.array_equal(r["n_second"], [0, 3]) and np.array_equal(r["n_above"][:, 0], [3, 3])
    assert r["major"][0] == 0 and r["n_distinct"][0] == 1 and r["status"][0] == 0
    assert r["mean_P"][0] == 0.5 and r["ss_P"][0] == 0.0 and r["ss_H"][0] == 0.0
    assert np.array_equal(r["q_P"][0], [0.5, 0.5])


def test_single_member():
    tr = np.array([[3.0, 1e-9, 4.5, 100.0]])
    r = R.isoforms_ref(tr, [[0]], thresholds=[0.0, 0.5], ranks=[0, 3, 4])
    assert np.array_equal(r["H"][0], np.zeros(4)) and not np.signbit(r["H"][0]).any()               # +0.0, never -0.0
    assert np.array_equal(r["P"][0], np.ones(4))
    assert np.array_equal(r["top"][0], np.zeros(4)) and np.array_equal(r["second"][0], np.full(4, R.NONE))
    assert r["n_top"][0] == 4 and r["n_second"][0] == 0 and np.array_equal(r["n_above"][0], [4, 4])
    assert r["mean_H"][0] == 0.0 and r["mean_P"][0] == 1.0
    assert np.array_equal(r["q_P"][0], [1.0, 1.0, np.nan], equal_nan=True)                          # a rank = S gives NaN for that rank alone


def test_member_that_is_zero_everywhere():
    tr = np.array([[1.0, 3.0], [0.0, 0.0], [3.0, 1.0]])
    r = R.isoforms_ref(tr, [[0, 1, 2]], thresholds=[0.0])
    want = -(0.25 * np.log(0.25) + 0.75 * np.log(0.75))
    assert np.allclose(r["H"][0], want, rtol=0, atol=1e-15)                                          # the zero member contributes nothing
    assert np.array_equal(r["top"][0], [2, 0]) and np.array_equal(r["second"][0], [0, 2])
    assert np.array_equal(r["n_top"], [1, 0, 1]) and np.array_equal(r["n_second"], [1, 0, 1])        # it is never the top, nor the second
    assert np.array_equal(r["n_above"][:, 0], [2, 0, 2])                                             # 0 > 0 * T is false
    assert r["major"][0] == 0 and r["n_distinct"][0] == 2                                            # equal n_top: the smallest position
    two = R.isoforms_ref(tr, [[0, 2]])
    assert np.array_equal(two["H"][0], r["H"][0]) and np.array_equal(two["P"][0], r["P"][0])


def test_all_zero_sample_invalidates_the_group_alone():
    tr = np.array([[1.0, 0.0, 2.0], [2.0, 0.0, 1.0], [5.0, 6.0, 7.0]])
    r = R.isoforms_ref(tr, [[0, 1], [2, 0], [1]], thresholds=[0.1], ranks=[1])
    assert np.array_equal(r["status"], [1, 0, 1])
    for k in ("mean_H", "ss_H", "mean_P", "ss_P"):
        assert np.isnan(r[k][[0, 2]]).all() and np.isfinite(r[k][1])
    assert np.isnan(r["H"][[0, 2]]).all() and np.isnan(r["P"][[0, 2]]).all() and np.isnan(r["q_H"][[0, 2]]).all()
    assert (r["top"][[0, 2]] == R.NONE).all() and (r["second"][[0, 2]] == R.NONE).all()
    assert np.array_equal(r["n_top"], [0, 0, 3, 0, 0]) and np.array_equal(r["n_above"][:, 0], [0, 0, 3, 2, 0])
    assert np.array_equal(r["n_distinct"], [0, 1, 0]) and np.array_equal(r["major"], [0, 0, 0])
    alone = R.isoforms_ref(tr, [[2, 0]], thresholds=[0.1], ranks=[1])
    for k in ("H", "P", "top", "second", "mean_H", "ss_H", "mean_P", "ss_P", "q_H", "q_P"):
        assert np.array_equal(alone[k][0], r[k][1]), k
    for bad in (np.nan, np.inf, -1.0):
        t2 = tr.copy()
        t2[0, 1] = bad
        assert np.array_equal(R.isoforms_ref(t2, [[0, 2], [2]])["status"], [1, 0])


def test_thresholds_sit_at_the_comparison():
    # T = 8: x = 2 is exactly 0.25 T, so it is not above 0.25 and is above the next double below
    tr = np.array([[2.0], [6.0]])
    below = np.nextafter(0.25, 0.0)
    r = R.isoforms_ref(tr, [[0, 1]], thresholds=[0.25, below, 0.75, np.nextafter(0.75, 0.0)])
    assert np.array_equal(r["n_above"], [[0, 1, 0, 0], [1, 1, 0, 1]])
    # the product theta * T is what is compared, rounded once: 0.1 * 3 > 0.3 in doubles
    tr = np.array([[0.3], [2.7]])
    assert tr[:, 0].sum() == 3.0 and 0.1 * 3.0 > 0.3
    assert np.array_equal(R.isoforms_ref(tr, [[0, 1]], thresholds=[0.1])["n_above"][:, 0], [0, 1])


def test_reference_refuses_bad_descriptions():
    tr = np.ones((3, 2))
    for groups, th, rk in (([], (), ()), ([[]], (), ()), ([[0, 0]], (), ()), ([[3]], (), ()), ([[0]], (1.0,), ()), ([[0]], (np.nan,), ()),
                           ([[0]], (0.1,) * 9, ()), ([[0]], (), (0,) * 65)):
        with pytest.raises(ValueError):
            R.isoforms_ref(tr, groups, th, rk)


@pytest.mark.parametrize("Sa,Sb", [(7, 7), (5, 12)])
def test_switch_probability_counts_all_pairs(Sa, Sb):
    from mmseq_amd.isoforms import switch_probability
    rng = np.random.default_rng(Sa * 100 + Sb)
    groups = [[0, 1, 2], [3], [4, 5]]
    ptr = np.array([0, 3, 4, 6])
    tra = np.round(rng.gamma(2.0, 1.0, (6, Sa)), 1)
    trb = np.round(rng.gamma(2.0, 1.0, (6, Sb)), 1)
    a, b = R.isoforms_ref(tra, groups), R.isoforms_ref(trb, groups)
    got = switch_probability(ptr, a["n_top"], Sa, b["n_top"], Sb)
    for g in range(3):
        assert got[g] == R.switch_probability_brute(a["top"][g], b["top"][g]), g
    assert got[1] == 0.0 and 0.0 < got[0] < 1.0
    # a group that is not valid on one side has no counts: NaN
    trb[4, 0] = np.nan
    b = R.isoforms_ref(trb, groups)
    got = switch_probability(ptr, a["n_top"], Sa, b["n_top"], Sb)
    assert np.isnan(got[2]) and got[1] == 0.0
    with pytest.raises(ValueError):
        switch_probability(ptr, a["n_top"][:-1], Sa, b["n_top"], Sb)
