"""tests/contrast_ref.py, the numpy specification of mmg_contrast_*, on its own (no device)."""
import numpy as np
import pytest

import contrast_ref as R


def _traces(seed, n, S):
    return np.exp(np.random.default_rng(seed).normal(0.0, 3.0, (n, S)))


def test_a_transcript_against_itself_is_exactly_zero():
    tr = _traces(1, 4, 64)
    o = R.contrast_ref(tr, [([2], [2]), ([0, 3], [0, 3])], [0, 63])
    assert (o["R"] == 0.0).all() and (o["p_gt"] == 0.0).all() and (o["var"] == 0.0).all() and (o["log_ratio"] == 0.0).all()
    assert (o["percentiles"] == 0.0).all() and (o["rc"] == 0).all()


def test_swapping_the_sides_negates_bit_for_bit():
    tr = _traces(2, 7, 128)
    a = R.contrast_ref(tr, [([0], [1]), ([2, 3, 4], [5, 6]), ([0], [0, 1, 2])], [3, 64])
    b = R.contrast_ref(tr, [([1], [0]), ([5, 6], [2, 3, 4]), ([0, 1, 2], [0])], [3, 64])
    assert np.array_equal(a["R"], -b["R"]) and np.array_equal(a["log_ratio"], -b["log_ratio"])
    assert np.array_equal(a["var"], b["var"])
    assert not (a["R"] == 0.0).any()                     # no N_s == D_s here
    assert np.array_equal(a["p_gt"], 1.0 - b["p_gt"])
    assert np.array_equal(a["percentiles"][:, 0], -np.sort(b["R"], axis=1)[:, 127 - 3])


def test_one_member_per_side_is_the_difference_of_the_log_means():
    tr = _traces(3, 5, 1024)
    o = R.contrast_ref(tr, [([0], [1]), ([4], [2])])
    lm = np.log(tr).mean(axis=1)
    np.testing.assert_allclose(o["log_ratio"], [lm[0] - lm[1], lm[4] - lm[2]], rtol=1e-12, atol=1e-12)
    assert np.array_equal(o["p_gt"], [(tr[0] > tr[1]).mean(), (tr[4] > tr[2]).mean()])


def test_the_difference_of_logs_is_finite_where_the_quotient_is_not():
    """values near 1e-300 against values near 1e+5: r is finite (the quotient, near 1e-305, is still a normal number there: the
    quotient form itself breaks a little further out, against 1e+30, where the quotient underflows to 0 and to inf)"""
    rng = np.random.default_rng(4)
    lo = 1e-300 * np.exp(rng.normal(0, 1, 64))
    tr = np.stack([lo, 1e5 * np.exp(rng.normal(0, 1, 64)), 1e30 * np.exp(rng.normal(0, 1, 64))])
    o = R.contrast_ref(tr, [([0], [1]), ([1], [0]), ([0], [2]), ([2], [0])])
    assert np.isfinite(o["R"]).all() and np.isfinite(o["log_ratio"]).all() and np.isfinite(o["var"]).all()
    assert abs(o["log_ratio"][0] - np.log(1e-305)) < 1.0 and abs(o["log_ratio"][2] + 330 * np.log(10.0)) < 1.0
    with np.errstate(all="ignore"):
        assert (tr[0] / tr[2] == 0.0).all() and np.isinf(np.log(tr[0] / tr[2])).all()   # the quotient form: underflow, -inf
        assert np.isinf(tr[2] / tr[0]).all()
    assert np.array_equal(o["p_gt"], [0.0, 1.0, 0.0, 1.0])


def test_non_finite_values_propagate():
    tr = _traces(5, 2, 8)
    tr[0, 3] = 0.0
    o = R.contrast_ref(tr, [([0], [1]), ([0], [0])], [0, 7])
    assert o["R"][0, 3] == -np.inf and o["log_ratio"][0] == -np.inf and o["percentiles"][0, 0] == -np.inf
    assert np.isnan(o["R"][1, 3]) and np.isnan(o["log_ratio"][1])       # -inf - -inf
    # the NaN x86 gives for inf - inf has its sign bit set: by the library's key such a NaN sorts first, a positive one last
    assert np.isnan(o["percentiles"][1]).sum() == 1 and (o["percentiles"][1] == 0.0).sum() == 1


def test_sokal_codes_and_the_pinned_oracle(orc):
    rng = np.random.default_rng(6)
    assert R.sokal(rng.normal(size=3))[0] == 200 and R.sokal(rng.normal(size=1000))[0] == 201
    x = np.cumsum(rng.normal(size=256)) * 0.1 + rng.normal(size=256)
    rc, var, tau, m = orc.sokal(x)
    got = R.sokal(x)
    assert rc == 0 and got[0] == 0
    np.testing.assert_allclose(got[1:], [var, tau], rtol=1e-9)


def test_sort_key_orders_like_the_values():
    x = np.array([3.0, -0.0, 0.0, -np.inf, np.inf, -2.5, 1e-310, -1e-310, np.nan])
    s = R.sorted_series(x)
    assert np.isnan(s[-1]) and np.array_equal(s[:-1], np.sort(x[:-1]))
    assert np.signbit(s[3]) and not np.signbit(s[4])      # -0.0 before +0.0


def test_bad_contrasts_are_refused():
    tr = _traces(7, 3, 4)
    for bad in ([], [([], [0])], [([0], [])], [([0, 0], [1])], [([0], [3])]):
        with pytest.raises(ValueError):
            R.contrast_ref(tr, bad)
