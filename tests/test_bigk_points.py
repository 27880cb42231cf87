"""The three shortcuts of the conditional-binomial chain's kernel at their decision boundaries, on the HOST instantiation of the library's
inline code (mmg_selftest_bigk_points with device = -1): no GPU needed.  tests/test_gpu_bigk_points.py runs the fp32 tests and compares the
fp64 outputs with these in kernels; the checks are tests/bigk_points_checks.py.

Here: the boundaries of the fp64 code are found by bisection over the (n, p) grid and the points placed around them; the STEP bound
binv_zero_bound settles x = 0 only where the fp64 search does, lies below (1 - p)^n at 80 digits, and the bound its comment derives holds
for the search's own r0; the fp64 search equals the exact CDF wherever rounding cannot matter; the BTRS candidate and the path it takes
equal a numpy restatement."""
import pytest

import bigk_points_checks as K


@pytest.fixture(scope="module")
def gibbs():
    from mmseq_amd import gibbs
    return gibbs


def test_inversion_points_meet_the_conditions_of_a_device_run(gibbs):
    I = K.check_inversion_inputs(gibbs)
    print("inversion: %d (n, p), %d boundaries of the fp64 search (k up to %d), %d points" % (len(I.grid), I.b_u.size, I.b_k.max(), I.p_u.size))


def test_step_bound_settles_x_0_only_where_the_search_does(gibbs):
    K.check_step_bound_settles_zero(gibbs)


def test_step_bound_is_below_the_exact_r0(gibbs):
    K.check_step_bound_below_exact_r0(gibbs)


def test_the_bound_the_step_comment_derives_holds_for_the_search(gibbs):
    gap, n, p = K.check_step_claim(gibbs)
    print("STEP: smallest u_0 - binv_zero_bound over the grid: %.6e at n = %d, p = %r" % (gap, n, p))


def test_fp64_search_equals_the_exact_cdf_away_from_its_boundaries(gibbs):
    far, far_b, pts, (shift, n, p) = K.check_inversion_truth(gibbs)
    print("inversion: %d of %d points farther than 2^-40 (k + 1) from every exact boundary of the search's sum, %d farther than that + n 2^-54 from "
          "every one of Binomial(n, p); the two CDFs differ by up to %.3e (n = %d, p = %r: %.2f n 2^-54)" % (far, pts, far_b, shift, n, p, shift / (n * 2.0 ** -54)))


def test_btrs_candidate_path_and_exact_test_equal_the_restatement(gibbs):
    K.check_btrs_host(gibbs)
    B = K.btrs(gibbs)
    print("BTRS: %d (n, p, u) with a threshold v* in (2^-32, 1), %d points" % (B.n.size, B.p_v.size))
