"""mmg_qvalues on the device against the restatement (tests/qvalue_ref.py).  Every quantity is an integer count or one IEEE division of
two exact products, so q is compared bitwise (NaN in the same places) and null_ge exactly."""
import ctypes as C

import numpy as np
import pytest

import qvalue_ref as Q

NAN, INF = float("nan"), float("inf")


def assert_is_the_restatement(obs, null):
    from mmseq_amd.diff import qvalues
    ge, q = qvalues(obs, null)
    want_ge, want_q = Q.qvalues(obs, null)
    assert ge.dtype == np.uint64 and np.array_equal(ge, want_ge)
    assert np.array_equal(q, want_q, equal_nan=True)
    return ge, q


@pytest.mark.gpu
@pytest.mark.parametrize("n_null", [1, 63, 4097])
@pytest.mark.parametrize("F", [1, 64, 65, 1000])
def test_shapes_around_a_wave_a_block_and_a_sort_tile(gpu, F, n_null):
    rng = np.random.default_rng(1000 * F + n_null)
    ge, q = assert_is_the_restatement(rng.normal(0.7, 2.0, F), rng.normal(0.0, 1.0, n_null))
    assert (q >= 0).all() and (q <= 1).all() and ge.max() <= n_null


@pytest.mark.gpu
def test_all_observed_values_equal(gpu):
    rng = np.random.default_rng(5)
    null = np.concatenate([rng.normal(0.25, 1.0, 500), [0.25] * 7])
    ge, q = assert_is_the_restatement(np.full(300, 0.25), null)
    assert len(set(q)) == 1 and len(set(ge)) == 1 and ge[0] == (null >= 0.25).sum()


@pytest.mark.gpu
def test_heavy_ties_eight_distinct_values_on_both_sides(gpu):
    rng = np.random.default_rng(6)
    vals = np.array([-2.0, -0.5, 0.0, 0.5, 1.0, 1.5, 3.0, 8.0])
    ge, q = assert_is_the_restatement(vals[rng.integers(0, 8, 777)], vals[rng.integers(0, 8, 3001)])
    assert len(set(q)) <= 8


@pytest.mark.gpu
@pytest.mark.parametrize("obs,null", [
    ([3.0, 1.0, 2.5, 0.5, 2.0], [0.7, 3.5, 0.2, 2.2, -1.0, 1.5, 0.8, 0.4, 0.6, 0.3]),
    ([2.0, 1.0, 2.0], [1.0, 2.0, 0.0, 1.0]),
    ([INF, -INF, 0.0], [INF, -INF, 1.0, -1.0]),
    ([1.0, NAN, 2.0], [NAN, 2.5, NAN, 0.0]),
    ([NAN, NAN], [1.0]),
    ([-0.0, 0.0], [0.0, -0.0, -1.0]),
    ([0.0], [-0.0]),
    ([1.0, 2.0, NAN], [NAN, NAN]),
], ids=["by_hand", "ties", "infinities", "nan", "all_observed_nan", "zeros", "zero_against_minus_zero", "no_nulls_left"])
def test_the_cases_of_the_cpu_test(gpu, obs, null):
    """tests/test_qvalue_ref.py writes out what each of these gives; here the device against the restatement that passed it."""
    ge, q = assert_is_the_restatement(obs, null)
    if obs == [3.0, 1.0, 2.5, 0.5, 2.0]:
        assert list(ge) == [1, 3, 1, 6, 2] and list(q) == [0.25, 0.375, 0.25, 0.6, 1.0 / 3.0]


@pytest.mark.gpu
def test_special_values_scattered_through_a_larger_case(gpu):
    rng = np.random.default_rng(7)
    obs, null = np.round(rng.normal(0.5, 2.0, 2000), 2), np.round(rng.normal(0.0, 1.0, 9000), 2)
    for a, n in ((obs, 40), (null, 200)):
        a[rng.choice(a.size, n, replace=False)] = rng.choice([NAN, INF, -INF, -0.0, 0.0], n)
    assert_is_the_restatement(obs, null)


@pytest.mark.gpu
def test_many_blocks_and_a_deep_search(gpu):
    """F = 100 003 against 1 000 003 nulls: several blocks in every kernel, 20 steps of the search, both sorts beyond one tile."""
    rng = np.random.default_rng(8)
    obs = rng.normal(0.3, 1.5, 100003)
    null = rng.normal(0.0, 1.0, 1000003)
    obs[::5000] = NAN
    null[::70001] = NAN
    ge, q = assert_is_the_restatement(obs, null)
    assert np.isnan(q).sum() == len(obs[::5000]) and 0.0 <= np.nanmin(q) < np.nanmax(q) == 1.0


@pytest.mark.gpu
def test_error_returns(gpu):
    from mmseq_amd import _lib
    lib = _lib.load()
    obs, null = np.zeros(4), np.zeros(4)
    ge, q = np.zeros(4, np.uint64), np.zeros(4)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.mmg_qvalues(0, 0, p(obs), 4, p(null), p(ge), p(q)) == 1
    assert lib.mmg_qvalues(0, 4, p(obs), 0, p(null), p(ge), p(q)) == 1
    assert lib.mmg_qvalues(0, 4, p(obs), 1 << 31, p(null), p(ge), p(q)) == 1
    for args in ((None, 4, p(null), p(ge), p(q)), (p(obs), 4, None, p(ge), p(q)), (p(obs), 4, p(null), None, p(q)), (p(obs), 4, p(null), p(ge), None)):
        assert lib.mmg_qvalues(0, 4, *args) == 1
        assert b"NULL" in lib.mmg_last_error()
    assert lib.mmg_qvalues(0, 4, p(obs), 4, p(null), p(ge), p(q)) == 0
    assert list(ge) == [4] * 4 and list(q) == [1.0] * 4
