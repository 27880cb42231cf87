"""The exact reference of tests/mmdiff_exact.py checked against closed forms, and the numpy restatement of mmdiff checked against it.

The fixture: three rows of y (no effect, a clear effect, an effect with unequal spread) under five designs, and the twelve-sample
rows under three designs of tests/wide_designs.py (cases f, g, h: three covariate columns; two with -fixalpha; a fitted model 0).
tests/golden/mmdiff_exact.json records the exact log Bayes factor and the within-model posterior means of every row and design on the
default grid (`python tests/test_mmdiff_exact.py` rewrites it); test_golden_file_is_the_quadrature recomputes it, and the device tests of
tests/test_gpu_mmdiff_exact.py read it, so the quadrature runs once.

What the first trial of this comparison got wrong.  It gave model 0 of `-de 3 3` an eta column, because `-de` writes P0 as a column
of ones.  A single constant column is nil (src/bms.cpp:1154-1156): model 0 has alpha, one sigma^2 and rho, nothing else.  With the
extra column the "exact" log BF of the three rows was -1.72509, 1.51756, 1.50481; without it -1.77839, 1.46819, 1.45902, lower by
0.053, 0.049 and 0.046.  The restatement's 32 x 2048 run of that trial (mean gamma 0.1411, 0.8003, 0.8100; s.e. 0.0037, 0.0047,
0.0027) was 2.7 to 4.2 s.e. below the first set and is 0.9, 2.6 and 0.5 s.e. below the second.  test_nil_design_column_is_no_column
is the check that would have caught it: it pins what a constant column means, and what it would cost to read it otherwise.
"""
import json
import math
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mmdiff_exact as X  # noqa: E402
import wide_designs  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mmdiff_exact.json")

E6 = (0.1, 0.2, 0.3, 0.15, 0.25, 0.2)
ROWS6 = ((2.0, 2.2, 1.9, 2.1, 2.3, 1.8),
         (2.0, 2.2, 1.9, 2.9, 3.1, 2.7),
         (2.0, 2.6, 1.5, 3.6, 2.9, 4.1))
# design (d), groups of 6 and 6: the three samples of each group above, then a second draw of three
E12 = E6[:3] + (0.2, 0.1, 0.25) + E6[3:] + (0.3, 0.15, 0.2)
ROWS12 = (ROWS6[0][:3] + (2.1, 1.7, 2.2) + ROWS6[0][3:] + (2.3, 2.5, 2.1),
          ROWS6[1][:3] + (2.3, 2.0, 2.4) + ROWS6[1][3:] + (2.4, 2.2, 2.6),
          ROWS6[2][:3] + (2.4, 1.8, 2.1) + ROWS6[2][3:] + (2.0, 2.9, 2.2))
M_COV = (0.3, 1.1, -0.4, 0.9, 0.0, -1.2)    # the covariate of test_gpu_mmdiff's "covariate" case

CASES = {
    "a_de33": dict(),
    "b_fixalpha": dict(fixalpha=True),
    "c_covariate": dict(cov=True),
    "d_de66": dict(n=12),
    "e_d3_s05": dict(d=3.0, s=0.5),
    "f_cov3": dict(wide="k3"),
    "g_cov2_fixalpha": dict(wide="k2", fixalpha=True),
    "h_batch": dict(wide="batch", classes1=1),
}
WIDE = tuple(c for c in CASES if "wide" in CASES[c])     # designs of tests/wide_designs.py on the rows of ROWS12


def design(case):
    """y (3, N), e (N,), M, P0, P1, classes (N, 2) and the keyword arguments d, s, fixalpha of a case."""
    c = CASES[case]
    if "wide" in c:
        M, P0, P1, classes = wide_designs.design(c["wide"])
        if c.get("classes1") == 1:      # one variance class in model 1: its grid then has the 2 lambdas and 1 sigma^2
            classes[:, 1] = 0
        return np.array(ROWS12), np.array(E12), M, P0, P1, classes, dict(d=1.4, s=2.0, fixalpha=c.get("fixalpha", False))
    n = c.get("n", 6)
    y = np.array(ROWS12 if n == 12 else ROWS6)
    e = np.array(E12 if n == 12 else E6)
    first = np.arange(n) < n // 2
    M = np.array(M_COV)[:, None] if c.get("cov") else np.zeros((n, 1))
    P0 = np.ones((n, 1))
    P1 = np.where(first, 0.5, -0.5)[:, None]
    classes = np.stack([np.zeros(n, np.int64), (~first).astype(np.int64)], 1)
    return y, e, M, P0, P1, classes, dict(d=c.get("d", 1.4), s=c.get("s", 2.0), fixalpha=c.get("fixalpha", False))


def compute_case(case, grid=None, rows=(0, 1, 2)):
    """The exact values of a case: per row log_bf and the posterior means mmdiff prints (None where the model has no such term)."""
    y, e, M, P0, P1, classes, kw = design(case)
    if grid is not None:
        kw["grid"] = grid
    out = dict(log_bf=[], alpha0=[], alpha1=[], beta0=[], beta1=[], eta1=[])
    for r in rows:
        pm = [X.posterior_mean(y[r], e, M, P, classes[:, m], **kw) for m, P in ((0, P0), (1, P1))]
        out["log_bf"].append(pm[1]["log_marginal"] - pm[0]["log_marginal"])
        for m in range(2):
            out["alpha%d" % m].append(pm[m]["alpha"])
            out["beta%d" % m].append(float(pm[m]["beta"][0]) if pm[m]["beta"].size else None)
        out["eta1"].append(float(pm[1]["eta"][0]))
        if case in WIDE:                # every column, under keys the five first cases do not have
            for m in range(2):
                out.setdefault("beta%d_cols" % m, []).append([float(v) for v in pm[m]["beta"]])
                out.setdefault("eta%d_cols" % m, []).append([float(v) for v in pm[m]["eta"]])
    return out


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _sigmoid(x):
    return 1.0 / (1.0 + math.exp(-x))


# ----------------------------------------------------------------------------- the reference against closed forms
def _refinement_job(job):
    case, r = job
    y, e, M, P0, P1, classes, kw = design(case)
    base = X.log_bf(y[r], e, M, P0, P1, classes, **kw)
    return base, X.log_bf(y[r], e, M, P0, P1, classes, grid=X.DEFAULT_GRID.refined(), **kw) - base


def test_grid_refinement_moves_log_bf_by_less_than_1e_5():
    """Half the step and both ranges wider by 5 at each end, for every row of the first five designs (the jobs run in a few processes,
    about five minutes on 8 cores with the three rows of the wide designs: the refined grid of model 1 has 20 times the points).  The
    default grid's values are also those of the golden file.
    Movements of log BF, rows 0, 1, 2:
        a_de33       -1.6e-09   2.0e-08   4.0e-12
        b_fixalpha    3.6e-15   7.1e-15   1.1e-14
        c_covariate  -2.0e-09   1.6e-08   1.0e-12
        d_de66        2.3e-09   2.0e-09   0.0e+00
        e_d3_s05      8.7e-10   1.5e-08   9.0e-13
    The designs of tests/wide_designs.py take one row each, the row test_golden_file_is_the_quadrature recomputes (their grids have
    three dimensions in one model or in both, and a refined run of one row takes minutes):
        f_cov3           row 2   3.6e-15
        g_cov2_fixalpha  row 0   2.8e-14
        h_batch          row 1   5.7e-10
    With log sigma^2 from -12 instead of -18 the second row of a_de33 moved by 2.7e-5, all of it from that end."""
    jobs = [(case, r) for i, case in enumerate(CASES) for r in range(3) if case not in WIDE or r == i % 3]
    with ProcessPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        got = list(ex.map(_refinement_job, jobs))
    g = golden()
    for (case, r), (base, mv) in zip(jobs, got):
        print("refinement %s row %d: log BF %.6f moves by %.2e" % (case, r, base, mv))
    for (case, r), (base, mv) in zip(jobs, got):
        assert abs(base - g[case]["log_bf"][r]) <= 1e-9, (case, r, base)
        assert abs(mv) < 1e-5, (case, r, mv)


def test_golden_file_is_the_quadrature():
    """The recorded posterior means and log BF, recomputed for one row of each design (the refinement test recomputes every log BF)."""
    g = golden()
    assert sorted(g) == sorted(CASES)
    for i, case in enumerate(CASES):
        r = i % 3
        want = compute_case(case, rows=(r,))
        for k, v in want.items():
            a, b = g[case][k][r], v[0]
            if isinstance(b, list):          # the keys of the wide cases that hold every column
                assert len(a) == len(b) and all(abs(x - y) <= 1e-9 * max(1.0, abs(y)) for x, y in zip(a, b)), (case, k, a, b)
                continue
            assert (a is None and b is None) or abs(a - b) <= 1e-9 * max(1.0, abs(b)), (case, k, a, b)


def test_fixture_rows_mix():
    """P(gamma = 1) at p' = 0.5 lies in [0.15, 0.85] for every row of designs b to e, so chains of a few thousand iterations visit
    both models; two rows of d_de66 were replaced to get there.  The three rows of a_de33 are the given fixture: its first row is at
    0.1445 (it was chosen at 0.1512, under the reading with an eta column in model 0), so that design is held to [0.14, 0.86]."""
    g = golden()
    for case in CASES:
        lo = 0.14 if case == "a_de33" else 0.15
        for b in g[case]["log_bf"]:
            assert lo <= _sigmoid(b) <= 1.0 - lo, (case, b)


def test_gaussian_only_model():
    """lambda and sigma^2 pinned: the grid is one point and the value is the multivariate normal density of y plus the log priors
    of lambda and sigma^2 there, the latter by numerical integration over rho."""
    from scipy.integrate import quad
    from scipy.stats import invgamma, multivariate_normal
    y, e, M, P0, P1, classes, _ = design("c_covariate")
    lam, sg = 0.7, 0.35
    for fixalpha in (False, True):
        Xd = np.concatenate(([] if fixalpha else [np.ones((6, 1))]) + [M, P1], 1)
        v0 = np.array(([] if fixalpha else [25.0]) + [25.0 if fixalpha else 4.0, lam])
        cov = np.diag(e * e + sg) + (Xd * v0) @ Xd.T
        want = multivariate_normal.logpdf(y[1], np.zeros(6), cov) + invgamma.logpdf(lam, 1.4, scale=2.0)
        want += math.log(quad(X.rho_integrand, 0, np.inf, args=(np.array([sg, sg]),), epsabs=0, epsrel=1e-12)[0])
        got = X.log_marginal(y[1], e, M, P1, classes[:, 1], 1.4, 2.0, fixalpha, X.Grid(pin=(lam, sg)))
        assert abs(got - want) < 1e-9, (fixalpha, got, want)


def test_rho_integrates_out_in_closed_form():
    from scipy.integrate import quad
    for sig in ([0.02], [0.5, 3.0], [40.0, 0.1]):
        sig = np.array(sig)
        num = quad(X.rho_integrand, 0, np.inf, args=(sig,), epsabs=0, epsrel=1e-13)[0]
        assert abs(math.exp(X.log_prior_sigmasq(sig)) / num - 1.0) < 1e-10, sig


def test_rho_integrand_is_the_product_of_the_priors():
    from scipy.stats import gamma, invgamma
    rho, sig = 0.37, np.array([0.5, 3.0])
    want = gamma.pdf(rho, 1.2, scale=0.5) * np.prod(invgamma.pdf(sig, 2.0, scale=2.0 * rho))
    assert abs(X.rho_integrand(rho, sig) / want - 1.0) < 1e-12


def test_eta_marginal_is_student_t():
    """eta | lambda ~ N(0, lambda), lambda ~ InvGamma(d, s): eta is Student t with 2 d degrees of freedom and scale sqrt(s / d)."""
    from scipy.stats import t
    for d, s in ((1.4, 2.0), (3.0, 0.5)):
        for eta in (0.0, 0.3, -1.0, 4.0, 25.0):
            want = t.pdf(eta, 2.0 * d, scale=math.sqrt(s / d))
            assert abs(X.eta_marginal(eta, d, s) / want - 1.0) < 1e-9, (d, s, eta)


def test_equal_models_have_log_bf_zero():
    y, e, M, P0, P1, classes, _ = design("c_covariate")
    same = np.stack([classes[:, 1], classes[:, 1]], 1)
    assert abs(X.log_bf(y[1], e, M, P1, P1, same, grid=X.DEFAULT_GRID.coarsened(0.5))) <= 1e-12


def test_swapping_the_models_flips_the_sign():
    y, e, M, P0, P1, classes, _ = design("a_de33")
    assert X.log_bf(y[1], e, M, P1, P0, classes[:, ::-1]) == -X.log_bf(y[1], e, M, P0, P1, classes)


def test_nil_design_column_is_no_column():
    """A single constant column of P is no eta at all: the marginal equals that of P = None and of a column of zeros.  Two equal
    constant columns are not nil and give another model (two more intercepts with t priors); so does one column that is not
    constant.  For the first fixture row, reading `-de`'s column of ones as an eta column lowers log m_0 by 0.0533."""
    y, e, M, P0, P1, classes, _ = design("a_de33")
    c0 = classes[:, 0]
    base = X.log_marginal(y[0], e, None, None, c0)
    assert X.log_marginal(y[0], e, M, P0, c0) == base
    assert X.log_marginal(y[0], e, M, np.zeros((6, 1)), c0) == base
    assert X._Model(y[0], e, M, P0, c0, 1.4, 2.0, False, X.DEFAULT_GRID).dims == 1
    two = X.log_marginal(y[0], e, M, np.ones((6, 2)), c0)
    assert abs(two - base) > 0.01
    wiggle = P0.copy()
    wiggle[0, 0] += 2e-5
    as_column = X.log_marginal(y[0], e, M, wiggle, c0)
    assert abs((base - as_column) - 0.0533) < 5e-4, base - as_column


def test_designs_beyond_four_grid_dimensions_are_refused():
    y, e = np.array(ROWS6[0]), np.array(E6)
    P = np.kron(np.eye(3), np.ones((2, 1)))
    with pytest.raises(ValueError, match="6 dimensions"):
        X.log_marginal(y, e, None, P, np.repeat(np.arange(3), 2))


def test_posterior_mean_of_a_gaussian_only_model():
    """At a pinned grid point the posterior mean is the generalised least squares estimate with the prior precisions added."""
    y, e, M, P0, P1, classes, _ = design("c_covariate")
    lam, sg = 0.7, 0.35
    Xd = np.concatenate([np.ones((6, 1)), M, P1], 1)
    W = np.diag(1.0 / (e * e + sg))
    want = np.linalg.solve(Xd.T @ W @ Xd + np.diag([1 / 25.0, 1 / 4.0, 1 / lam]), Xd.T @ W @ y[2])
    pm = X.posterior_mean(y[2], e, M, P1, classes[:, 1], grid=X.Grid(pin=(lam, sg)))
    assert np.allclose([pm["alpha"], pm["beta"][0], pm["eta"][0]], want, rtol=1e-12, atol=0)


# ----------------------------------------------------------------------------- the rule of comparison, shared with the device tests
SE_CAP = 0.02


def check_against_exact(est, exact, what, logit_cap=False):
    """est (rows, R): R independent replicates' estimates of each row; exact (rows,).  |mean - exact| <= 5 s.e., the s.e. the
    replicates' sample standard deviation over sqrt(R).  With logit_cap the estimates are mean gammas: none may be 0 or 1, and the
    s.e. on the logit scale, s.e. / (m (1 - m)), must be at most 0.02, so that a shift of 0.1 in log BF fails.  Prints, then asserts;
    returns the deviations in s.e."""
    est, exact = np.asarray(est, np.float64), np.asarray(exact, np.float64)
    R = est.shape[1]
    m = est.mean(1)
    se = est.std(1, ddof=1) / math.sqrt(R)
    z = (m - exact) / se
    for r in range(est.shape[0]):
        extra = "  logit s.e. %.4f  logit(mean) - logit(exact) %+.4f" % (
            se[r] / (m[r] * (1 - m[r])), math.log(m[r] / (1 - m[r])) - math.log(exact[r] / (1 - exact[r]))) if logit_cap else ""
        print("%s row %d: exact %.5f mean %.5f s.e. %.5f dev %+.2f s.e.%s" % (what, r, exact[r], m[r], se[r], z[r], extra))
    if logit_cap:
        assert np.all((est > 0.0) & (est < 1.0)), "%s: a replicate never left one model" % what
        assert np.all(se / (m * (1.0 - m)) <= SE_CAP), (what, se / (m * (1.0 - m)))
    assert np.all(np.abs(m - exact) <= 5.0 * se), (what, z)
    return z


def check_means(res, g, reps, what):
    """The within-model means of a results dict (alpha (2, F), beta (2, K, F), eta (L0 + L1, F); three rows of `reps` replicates)
    against the golden entry g under check_against_exact: alpha of both models, every beta column of both models, model 0's eta
    where it has one and every eta column of model 1.  An entry of the first five cases holds one beta and one eta column."""
    col = lambda key, j: [row[j] for row in g[key]]
    for m in range(2):
        if g["alpha%d" % m][0] is not None:
            check_against_exact(res["alpha"][m].reshape(3, reps), g["alpha%d" % m], "%s alpha%d" % (what, m))
        if "beta%d_cols" % m in g:
            assert len(g["beta%d_cols" % m][0]) in (0, res["beta"].shape[1])      # a nil M keeps its column and has no entry
            for j in range(len(g["beta%d_cols" % m][0])):
                check_against_exact(res["beta"][m, j].reshape(3, reps), col("beta%d_cols" % m, j), "%s beta%d_%d" % (what, m, j))
        elif g["beta%d" % m][0] is not None:
            check_against_exact(res["beta"][m, 0].reshape(3, reps), g["beta%d" % m], "%s beta%d" % (what, m))
    if "eta1_cols" not in g:
        check_against_exact(res["eta"][-1].reshape(3, reps), g["eta1"], what + " eta1")
        return
    L1 = len(g["eta1_cols"][0])
    L0 = res["eta"].shape[0] - L1                     # a nil P0 keeps its column in the results and has no entry in eta0_cols
    assert L1 >= 1 and len(g["eta0_cols"][0]) in (0, L0)
    for l in range(len(g["eta0_cols"][0])):
        check_against_exact(res["eta"][l].reshape(3, reps), col("eta0_cols", l), "%s eta0_%d" % (what, l))
    for l in range(L1):
        check_against_exact(res["eta"][L0 + l].reshape(3, reps), col("eta1_cols", l), "%s eta1_%d" % (what, l))


def replicate(y, R):
    """Each row R times: row r is features r R .. r R + R - 1."""
    return np.repeat(np.asarray(y, np.float64), R, 0)


def test_restatement_agrees_with_the_exact_reference(orc):
    """tests/mmdiff_ref.py on design a_de33, 32 replicates of each row, 1024 + 2048 iterations, no tuning, seed 7: the run of the
    first trial.  32 x 2048 draws cannot meet the device tests' cap of 0.02 on the logit s.e. (measured: 0.030, 0.031, 0.018), so only the
    5 s.e. rule and the no-stuck-chain rule apply here; the cap holds in tests/test_gpu_mmdiff_exact.py at 512 x 4096.
    Measured deviations in s.e., rows 0, 1, 2: mean gamma -0.90, -2.67, -0.51 (logit(mean) - exact log BF -0.028, -0.080, -0.009);
    alpha0 -1.09, -0.42, +0.76; alpha1 -0.71, +0.45, -1.12; eta1 -1.44, -0.50, -1.11."""
    import mmdiff_ref as R
    y, e, M, P0, P1, classes, kw = design("a_de33")
    reps = 32
    _, res = R.run_bms(replicate(y, reps), np.tile(e, (3 * reps, 1)), M, P0, P1, classes, burnin=1024, iters=2048, tune=False, seed=7)
    g = golden()["a_de33"]
    gm = res["gamma_mean"].reshape(3, reps)
    assert np.all((gm > 0.0) & (gm < 1.0))
    check_against_exact(gm, [_sigmoid(b) for b in g["log_bf"]], "restatement gamma")
    check_against_exact(res["alpha"][0].reshape(3, reps), g["alpha0"], "restatement alpha0")
    check_against_exact(res["alpha"][1].reshape(3, reps), g["alpha1"], "restatement alpha1")
    check_against_exact(res["eta"][1].reshape(3, reps), g["eta1"], "restatement eta1")


@pytest.mark.parametrize("case", WIDE)
def test_restatement_agrees_with_the_exact_reference_on_wide_designs(orc, case):
    """As above for the designs of tests/wide_designs.py: 32 replicates of each row, 1024 + 2048 iterations, no tuning, seed 7, the
    5 s.e. rule for mean gamma and for every beta and eta column of both models (the cap on the logit s.e. is the device tests').
    Measured deviations in s.e., rows 0, 1, 2 of mean gamma, and the largest among the within-model means:
        f_cov3           +0.20  -0.14  -2.97     2.39 of 27 (eta1_0, row 1)
        g_cov2_fixalpha  -2.90  -1.10  +2.81     2.80 of 15 (eta1_0, row 0)
        h_batch          -1.44  +0.35  -0.70     2.20 of 18 (alpha0, row 2)
    At 512 x 4096 on the device the same three rows of mean gamma are within 1.4 s.e. (tests/test_gpu_mmdiff_exact.py)."""
    import mmdiff_ref as R
    y, e, M, P0, P1, classes, kw = design(case)
    reps = 32
    _, res = R.run_bms(replicate(y, reps), np.tile(e, (3 * reps, 1)), M, P0, P1, classes, burnin=1024, iters=2048, tune=False, seed=7,
                       fixalpha=kw["fixalpha"])
    g = golden()[case]
    gm = res["gamma_mean"].reshape(3, reps)
    assert np.all((gm > 0.0) & (gm < 1.0))
    check_against_exact(gm, [_sigmoid(b) for b in g["log_bf"]], case + " restatement gamma")
    check_means(res, g, reps, case + " restatement")


def _same_entry(a, b, rel=1e-9):
    """Two golden entries agree within the tolerance of test_golden_file_is_the_quadrature (lists compared element by element)."""
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(_same_entry(a[k], b[k], rel) for k in a)
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(_same_entry(x, y, rel) for x, y in zip(a, b))
    if a is None or b is None:
        return a is None and b is None
    return abs(a - b) <= rel * max(1.0, abs(b))


if __name__ == "__main__":
    with ProcessPoolExecutor(min(8, os.cpu_count() or 1)) as ex:
        out = dict(zip(CASES, ex.map(compute_case, CASES)))
    recorded = golden() if os.path.exists(GOLDEN) else {}
    for case in CASES:          # an entry that the recomputation confirms stays as it is recorded: other BLAS, other last digits
        if case in recorded and _same_entry(recorded[case], out[case]):
            out[case] = recorded[case]
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    for case in CASES:
        print(case, [round(_sigmoid(b), 4) for b in out[case]["log_bf"]])
