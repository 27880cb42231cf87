"""The three shortcuts of the conditional-binomial chain's kernel at their decision boundaries, on the device: the points of
tests/test_bigk_points.py (tests/bigk_points_checks.py) through mmg_selftest_bigk_points with device = 0.  Every fp64 output equals the host
instantiation's bit for bit; binv_pretest and btrs_pretest never decide differently from the fp64 code ON and AROUND its boundaries, the
estimate's error stays within its bound point by point, and the points the bounds leave room for are decided.  The measured margins are
printed (profiles/bigk_points.txt)."""
import pytest

import bigk_points_checks as K

pytestmark = pytest.mark.gpu


def test_fp64_outputs_equal_the_host_instantiation(gpu):
    K.check_device_fp64_equals_host(gpu, 0)


def test_binv_pretest_at_the_boundaries_of_the_fp64_search(gpu):
    decided, pts, room = K.check_device_binv_pretest(gpu, 0)
    print("binv_pretest: %d of %d points decided, none differently; all %d with 8 e_x of room decided" % (decided, pts, room))


def test_btrs_pretest_around_the_acceptance_threshold(gpu):
    for lo, hi, share, n2, decided, case in K.check_device_btrs_pretest(gpu, 0):
        print("btrs_pretest, %d <= n < %d: %d points reach the test, %d decided, none differently; largest |d32 - diff| / e32 = %.4f at %s"
              % (lo, hi, n2, decided, share, case))


def test_margins_of_the_inversion_bound(gpu):
    K.check_device_binv_pretest(gpu, 0)                          # slack 1 is the assertion; the rest is measured
    for slack, wrong, decided, first in K.check_device_margins(gpu, 0):
        print("binv_pretest at slack 1/%d: %d decided, %d differently%s" % (round(1 / slack), decided, wrong, "" if first is None else ", the first (n, p, u, pre, x): %s" % (first,)))


def test_reruns_are_identical(gpu):
    K.check_device_rerun(gpu, 0)
