"""CPU checks of the numpy restatement of mmdiff (tests/mmdiff_ref.py): its Philox against the oracle's, its samplers against the
oracle's keyed draws where they share a path, dlgamma against math.lgamma, the moment matching against its closed form."""
import math

import numpy as np
import pytest

import mmdiff_ref as R


def test_philox_matches_the_oracle(orc):
    rng = np.random.default_rng(3)
    for _ in range(50):
        c = rng.integers(0, 2 ** 32, 4, dtype=np.uint64)
        k = rng.integers(0, 2 ** 32, 2, dtype=np.uint64)
        got = np.array([int(w[()]) for w in R.philox(c[0], c[1], c[2], c[3], k[0], k[1])], np.uint32)
        assert np.array_equal(got, orc.philox(c.astype(np.uint32), k.astype(np.uint32)))


@pytest.mark.parametrize("shape", [0.3, 1.0, 2.6, 40.0])
def test_gamma_unit_matches_the_oracles_keyed_gamma(orc, shape):
    """simu_gamma_trace_keyed(seed, chain, tag, id, shape, scale, n)[row] is Gamma(shape) * scale on Stream(seed, chain, tag, id, row)."""
    seed, tag, sid, n = 99, 7, 5, 64
    want = orc.simu_gamma_trace_keyed(seed, 0, tag, sid, shape, 1.0, n)
    for row in range(n):
        rs = R.Streams(seed, tag, np.array([sid]), row)
        g = rs.gamma_unit(np.array([True]), shape)
        assert g[0] == want[row]


def test_normal_is_the_polar_method_on_the_stream():
    rs = R.Streams(1, R.TAG_DIFF, np.arange(4), 3)
    z = rs.normal(np.array([True, False, True, True]))
    assert np.isnan(z[1]) and np.all(np.isfinite(z[[0, 2, 3]]))
    assert rs.c3[1] == 0 and np.all(rs.c3[[0, 2, 3]] >= 1)
    # lane 0 alone gives the same draw: lanes never share blocks
    solo = R.Streams(1, R.TAG_DIFF, np.arange(4), 3).normal(np.array([True, False, False, False]))
    assert solo[0] == z[0]


def test_dlgamma_against_math_lgamma():
    xs = np.concatenate([np.linspace(0.1, 10, 997), np.geomspace(10, 1e6, 500), [0.5, 1.0, 1.5, 2.0, 3.0, 7.999, 8.0]])
    got = R.dlgamma(xs)
    for x, g in zip(xs, got):
        want = math.lgamma(x)
        # a few ulps of the larger of |lgamma| and the shift's logarithm (cancellation near the zeros at 1 and 2)
        assert abs(g - want) <= 8 * 2.0 ** -52 * max(1.0, abs(want), abs(math.lgamma(x + 8))), x
    assert R.dlgamma(1.0)[0] == pytest.approx(0.0, abs=4e-15) and R.dlgamma(2.0)[0] == pytest.approx(0.0, abs=4e-15)


def test_dlgamma_outside_its_domain_returns_at_once():
    """x <= 0, NaN and -inf give NaN, +inf gives +inf, without running the shift loop (which would never end for x <= -2^53)."""
    got = R.dlgamma(np.array([0.0, -0.0, -1.0, -1e12, -2.0 ** 60, -np.inf, np.nan, np.inf, 5e-324]))
    assert np.all(np.isnan(got[:7])) and got[7] == np.inf and np.isfinite(got[8])


def test_moment_matching_closed_form():
    rng = np.random.default_rng(1)
    for shape, scale in [(2.0, 0.5), (7.5, 3.0), (0.8, 10.0)]:
        x = rng.gamma(shape, scale, 200000)
        res, res2 = np.array([x.mean()]), np.array([np.log(x).mean()])
        got = R.shape_from(res, res2)[0]
        s = math.log(res[0]) - res2[0]
        assert got == pytest.approx((3 - s + math.sqrt((s - 3) ** 2 + 24 * s)) / (12 * s), rel=1e-14)
        assert got == pytest.approx(shape, rel=0.05)   # the approximation of the Gamma MLE it stands for


def test_keyed_permutation_is_a_permutation_and_depends_on_the_feature():
    perms = [R.permutation(1234, f, 6) for f in range(20)]
    assert all(sorted(p) == list(range(6)) for p in perms)
    assert len({tuple(p) for p in perms}) > 10
    assert R.permutation(1234, 3, 6) == R.permutation(1234, 3, 6)


def test_de_design_matches_the_reference_layout():
    M, P0, P1, C = R.de_design([2, 1])
    assert np.array_equal(P1[:, 0], [0.5, 0.5, -0.5]) and np.array_equal(C[:, 1], [0, 0, 1]) and R.is_nil(M) and R.is_nil(P0)
    M, P0, P1, C = R.de_design([1, 1, 2])
    assert np.array_equal(P1, [[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, 1]]) and np.array_equal(C[:, 1], [0, 1, 2, 2])


def test_restatement_is_deterministic_and_tunes():
    rng = np.random.default_rng(0)
    y = rng.normal(3, 0.2, (6, 4))
    e = np.full((6, 4), 0.2)
    M, P0, P1, C = R.de_design([2, 2])
    _, r1 = R.run_bms(y, e, M, P0, P1, C, burnin=1024, iters=1024, tune=False, seed=5)
    _, r2 = R.run_bms(y, e, M, P0, P1, C, burnin=1024, iters=1024, tune=False, seed=5)
    for k in r1:
        assert np.array_equal(r1[k], r2[k], equal_nan=True)
    assert np.all((r1["gamma_mean"] >= 0) & (r1["gamma_mean"] <= 1))
