"""The restatement of the q-values (tests/qvalue_ref.py) against a case worked by hand and against its own definition in loops: ties,
infinities, NaN on either side, the two zeros, no nulls left; and the properties of a q-value."""
from fractions import Fraction

import numpy as np
import pytest

import qvalue_ref as Q

NAN, INF = float("nan"), float("inf")


def both(obs, null):
    a, b = Q.qvalues_loops(obs, null), Q.qvalues(obs, null)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1], equal_nan=True)
    return b


def test_five_observed_against_ten_nulls_by_hand():
    """m = 5, m0 = 10.  Descending: t = 3 has V = 1 (3.5), R = 1: 5/10; t = 2.5: V = 1, R = 2: 5/20; t = 2: V = 2 (3.5, 2.2), R = 3: 10/30;
    t = 1: V = 3 (and 1.5), R = 4: 15/40; t = 0.5: V = 6 (and 0.8, 0.7, 0.6), R = 5: 30/50.  The estimate at 3 is above the one at 2.5,
    so the feature at 3 takes 1/4 from the threshold below it."""
    obs = [3.0, 1.0, 2.5, 0.5, 2.0]
    null = [0.7, 3.5, 0.2, 2.2, -1.0, 1.5, 0.8, 0.4, 0.6, 0.3]
    ge, q = both(obs, null)
    assert list(ge) == [1, 3, 1, 6, 2]
    assert list(q) == [float(Fraction(n, d)) for n, d in ((1, 4), (3, 8), (1, 4), (3, 5), (1, 3))]


def test_ties_count_on_both_sides():
    """obs 2, 2, 1 against nulls 2, 1, 1, 0: at t = 2: V = 1, R = 2: 3/8; at t = 1: V = 3, R = 3: 9/12."""
    ge, q = both([2.0, 1.0, 2.0], [1.0, 2.0, 0.0, 1.0])
    assert list(ge) == [1, 3, 1] and list(q) == [0.375, 0.75, 0.375]


def test_infinities_order_like_numbers():
    """+inf is the most significant value and is matched by a null +inf; -inf has every value at or above it."""
    ge, q = both([INF, -INF, 0.0], [INF, -INF, 1.0, -1.0])
    assert list(ge) == [1, 4, 2]
    assert list(q) == [0.75, 1.0, 0.75]      # 3/4 at +inf; (2 * 3) / (4 * 2) at 0; (4 * 3) / (4 * 3) at -inf


def test_nan_counts_on_neither_side():
    ge, q = both([1.0, NAN, 2.0], [NAN, 2.5, NAN, 0.0])
    assert list(ge) == [1, 0, 1] and np.isnan(q[1])
    assert list(q[[0, 2]]) == [0.5, 0.5]     # m = 2, m0 = 2: (1 * 2) / (2 * 2) at t = 1; (1 * 2) / (2 * 1) = 1 at t = 2, lowered to 1/2
    ge, q = both([NAN, NAN], [1.0])
    assert list(ge) == [0, 0] and np.isnan(q).all()


def test_the_two_zeros_are_one_value():
    ge, q = both([-0.0, 0.0], [0.0, -0.0, -1.0])
    assert list(ge) == [2, 2] and list(q) == [float(Fraction(2, 3))] * 2
    ge, q = both([0.0], [-0.0])
    assert list(ge) == [1] and list(q) == [1.0]


def test_without_nulls_every_q_is_nan():
    ge, q = both([1.0, 2.0, NAN], [NAN, NAN])
    assert list(ge) == [0, 0, 0] and np.isnan(q).all()


@pytest.mark.parametrize("seed", range(4))
def test_q_is_in_the_unit_interval_and_non_increasing_in_the_statistic(seed):
    rng = np.random.default_rng(seed)
    obs = np.round(rng.normal(0.5, 1.5, 60), 1)      # (rounded: ties)
    null = np.round(rng.normal(0.0, 1.0, 170), 1)
    ge, q = both(obs, null)
    assert (q >= 0).all() and (q <= 1).all()
    up = np.argsort(obs, kind="stable")
    assert (np.diff(q[up]) <= 0).all() and (np.diff(ge[up].astype(np.int64)) <= 0).all()
    for v in np.unique(obs):
        assert len(set(q[obs == v])) == 1
