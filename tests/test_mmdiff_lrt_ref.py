"""The numpy restatement of mmdiff -lrt (tests/mmdiff_lrt_ref.py) against independent optima: a closed form, and the grid-plus-polish
maximum of tests/lrt_optimum.py on fixtures whose profile likelihoods have a single local maximum.  No device.

The tolerance on l and on stat (TOL_LOGLIK).  The reference is run twice, the second time with the grid step halved (20 instead
of 10 points per decade) and the polish 100 times tighter (ftol = gtol = 1e-15 instead of 1e-13); the largest change of l over every
model of every fixture feature was 3.6e-15 when this file was written (test_reference_is_converged prints it and holds it to a
tenth of the tolerance).  Ten times that is 3.6e-14, below the floor of 1e-10 absolute, so the tolerance is the floor: 1e-10 on l,
and on stat = 2 (l_1 - l_0) the same bound applied to each l, 4e-10.  DESIGN.md section 10.5 carries the same derivation."""
import numpy as np
import pytest

import lrt_optimum as O
import mmdiff_lrt_ref as L
import mmdiff_ref as R

TOL_LOGLIK = 1e-10
TOL_STAT = 4.0 * TOL_LOGLIK


@pytest.fixture(scope="module")
def fitted():
    return {name: L.lrt(fx["y"], fx["e"], fx["M"], fx["P0"], fx["P1"], fx["C"], fx["fixalpha"])
            for name, fx in ((n, O.fixture(n)) for n in O.FIXTURES)}


# ----------------------------------------------------------------------------- closed form
@pytest.mark.parametrize("groups,fixalpha", [((3, 3), False), ((3, 4), False), ((2, 2, 2), False), ((3, 3), True)])
def test_closed_form_with_one_class_and_equal_e(groups, fixalpha):
    """One class and all e_i equal: the weights are equal, theta is ordinary least squares and sigma^2 = max(0, RSS / N - e^2).
    One scoring step from any start lands on it exactly, so what is left is the rounding of sums of N terms: 1e-12 relative to v."""
    M, P0, P1, C = R.de_design(groups)
    N = sum(groups)
    C = np.zeros((N, 2), np.int64)                  # one class in both models
    if len(groups) > 2:
        P1 = P1[:, 1:]                              # (with the intercept the three indicators are collinear: keep two)
    rng = np.random.default_rng(7)
    F = 10
    y = (0.0 if fixalpha else 2.0) + rng.normal(0.0, 0.4, (F, N))
    y[:4, :groups[0]] += 1.0
    e = np.repeat(rng.uniform(0.05, 0.6, (F, 1)), N, 1)
    y[0] = 0.0 if fixalpha else 3.25                # identical replicates: RSS = 0, the boundary
    e[1] = 2.0                                      # e^2 above RSS / N: the boundary again
    r = L.lrt(y, e, M, P0, P1, C, fixalpha)
    for m, P in enumerate((P0, P1)):
        X = L.design_matrix(M, P, fixalpha)
        if X.shape[1]:
            beta = np.linalg.lstsq(X, y.T, rcond=None)[0]
            rss = ((y.T - X @ beta) ** 2).sum(0)
        else:
            rss = (y ** 2).sum(1)
        esq = e[:, 0] ** 2
        sig = np.maximum(0.0, rss / N - esq)
        v = esq + sig
        ll = -0.5 * (N * np.log(2.0 * np.pi) + N * np.log(v) + rss / v)
        assert np.all(r["status"][m] & ~np.uint32(L.ST_BOUNDARY) == 0)
        assert np.array_equal((r["status"][m] & L.ST_BOUNDARY) != 0, sig == 0.0) and (sig == 0.0).sum() >= 2
        assert np.all(np.abs(r["sigmasq%d" % m][0] - sig) <= 1e-12 * v)
        assert np.all(np.abs(r["loglik"][m] - ll) <= TOL_LOGLIK)
    assert r["df"] == (2 if len(groups) > 2 else 1)


# ----------------------------------------------------------------------------- the global maximum
@pytest.mark.parametrize("name", O.FIXTURES)
def test_fixture_profiles_have_a_single_local_maximum(name):
    """Scoring finds a local maximum, so the comparison below is fair only where there is one: every feature of every fixture,
    on both grids."""
    for fine in (False, True):
        for m, opt in O.reference(name, fine).items():
            assert [o["modes"] for o in opt] == [1] * len(opt), (name, m, fine)


def test_reference_is_converged():
    change = max(abs(a["loglik"] - b["loglik"]) for name in O.FIXTURES for m in O.MODELS[name]
                 for a, b in zip(O.reference(name)[m], O.reference(name, True)[m]))
    print("largest change of l between the two runs of the reference: %.3g" % change)
    assert 10.0 * change <= TOL_LOGLIK


@pytest.mark.parametrize("name", O.FIXTURES)
def test_restatement_reaches_the_global_maximum(name, fitted):
    r, ref = fitted[name], O.reference(name, True)
    for m in O.MODELS[name]:
        want = np.array([o["loglik"] for o in ref[m]])
        diff = r["loglik"][m] - want
        print(name, "model", m, "l - reference:", diff)
        assert np.all(r["status"][m] & (L.ST_CAP | L.ST_SINGULAR) == 0)
        assert np.all(np.abs(diff) <= TOL_LOGLIK)
    if O.MODELS[name] == (0, 1):
        want = 2.0 * (np.array([o["loglik"] for o in ref[1]]) - np.array([o["loglik"] for o in ref[0]]))
        assert np.all(np.abs(r["stat"] - want) <= TOL_STAT)
        assert np.all(r["stat"] >= -TOL_STAT)       # nested models: the likelihood ratio is not negative


@pytest.mark.parametrize("name", O.FIXTURES)
def test_boundary_and_spread_features(name, fitted):
    """Features 0 and 1 have identical replicates: every sigma^2 is 0 and bit 4 is set; features 2 and 3 spread 100 e: model 0's
    variance is far above e^2."""
    r, fx = fitted[name], O.fixture(name)
    for m in O.MODELS[name]:
        assert np.all(r["sigmasq%d" % m][:, :2] == 0.0) and np.all(r["status"][m, :2] == L.ST_BOUNDARY)
    assert np.all(r["sigmasq0"][0, 2:4] > 100.0 * (fx["e"][2:4] ** 2).max(1)) and np.all(r["status"][0, 2:4] == 0)


def test_de_with_three_groups_has_no_maximum_likelihood_theta_in_model_1(fitted):
    """-de 2 2 2 without -fixalpha: the intercept and the three indicator columns are collinear, X'WX is not positive definite:
    status 2 and NaN for model 1 and for what is derived from it, model 0 untouched; df counts the columns as they are."""
    r = fitted["de222"]
    assert np.all(r["status"][1] == L.ST_SINGULAR) and np.all(r["iters"][1] == 0)
    assert np.isnan(r["loglik"][1]).all() and np.isnan(r["theta1"]).all() and np.isnan(r["sigmasq1"]).all()
    assert np.isnan(r["stat"]).all() and np.isnan(r["p_value"]).all() and np.isnan(r["q_value"]).all()
    assert r["df"] == (4 + 3) - (1 + 1) and np.isfinite(r["loglik"][0]).all()
    fx = O.fixture("de222")
    full = L.lrt(fx["y"], fx["e"], fx["M"], fx["P0"], fx["P1"], fx["C"], True)     # with -fixalpha the indicators are a basis
    assert np.all(full["status"][1] & L.ST_SINGULAR == 0) and np.isfinite(full["stat"]).all() and full["df"] == (3 + 3) - (0 + 1)


def test_max_iters_sets_the_cap_bit(fitted):
    """A cap of 2: the features on the boundary from the first step are done (one step to 0, one iteration that finds nothing to
    move), the others carry bit 1; a cap of 1 is reached by every feature."""
    fx = O.fixture("de33")
    full = fitted["de33"]
    for cap in (1, 2):
        capped = L.lrt(fx["y"], fx["e"], fx["M"], fx["P0"], fx["P1"], fx["C"], False, max_iters=cap)
        needs_more = full["iters"] > cap
        assert needs_more.any() and needs_more.all() == (cap == 1)
        assert np.array_equal((capped["status"] & L.ST_CAP) != 0, needs_more) and np.array_equal(capped["iters"], np.minimum(full["iters"], cap))
        assert np.all(capped["loglik"] <= full["loglik"] + TOL_LOGLIK)


def test_p_and_q_follow_from_stat(fitted):
    from scipy import stats
    r = fitted["covariate"]
    assert r["df"] == 2
    assert np.allclose(r["p_value"], stats.chi2.sf(np.maximum(r["stat"], 0.0), 2), rtol=1e-10, atol=0.0)
    assert np.array_equal(r["q_value"], L.bh_qvalues(r["p_value"]))


def test_file_text_names_the_terms_and_marks_missing_ones():
    fx = O.fixture("fixalpha")
    r = L.lrt(fx["y"][:3], fx["e"][:3], fx["M"], fx["P0"], fx["P1"], fx["C"], True)
    lines = L.lrt_file(["a", "b", "c"], r, fx["M"], fx["P0"], fx["P1"], True).split("\n")
    assert lines[0].split("\t") == ["feature_id", "loglik0", "loglik1", "lrt_stat", "df", "p_value", "q_value", "alpha0", "alpha1", "beta0_0",
                                    "beta1_0", "eta0_0", "eta1_0", "sigmasq0_0", "sigmasq1_0", "sigmasq1_1", "iters0", "iters1", "status0", "status1"]
    row = lines[3].split("\t")
    assert row[0] == "c" and row[4] == "2" and row[7:12] == ["NA"] * 5 and row[12] == R.fmt(r["theta1"][0, 2]) and len(lines) == 5
