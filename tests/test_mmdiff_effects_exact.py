"""The exact marginal posteriors of tests/mmdiff_effects_exact.py against closed forms, and mmdiff's effect summaries against them.

The statistical rule, shared with the device test (tests/test_gpu_mmdiff_effects.py).  The second and third fixture rows of design
a_de33 (tests/test_mmdiff_exact.py) are replicated R = 512 times, each replicate a feature of its own and so an independent chain:
1024 burn-in iterations, 2048 sampling iterations without tuning at p' = 0.2, every 16th sampling iteration a row (128 rows).  At
p' = 0.2 these two rows spend about half their rows in each model (n between 43 and 85 of 128 on either side in the restatement's
run); the first fixture row would leave model 1 about 5 rows and is not used.  The effect summaries of the rows
(tests/mmdiff_effects_ref.py here, the device's own summary of its own rows there) go through the project's rule
(test_mmdiff_exact.check_against_exact): the replicates' mean within 5 of their own standard errors of the exact value, for
    (a) `mean` of alpha0 (under model 0), alpha1 and eta1_0 (under model 1) against the exact posterior mean;
    (b) n_gt / n of eta1_0 against the exact P(> 0);
    (c) per percentile p in (2.5, 50, 97.5) and for the three of (a), F_exact(q_p) - (k + 1) / (n + 1) against 0, k the picked index:
        E[F(X_(k))] = (k + 1) / (n + 1) for the k-th of n independent draws (k from 0).
Replicates with n < 8 under the model are left out of (b) and (c), at most 5 % of them (none are, here).  (b) is taken for the effect
alone: the exact P(alpha > 0) of these rows is 1 - 3.4e-5 or nearer to 1, about one draw or none among the 33 000 that all replicates
of a row keep together, so n_gt / n of alpha is 1 in nearly every replicate, its standard error is 0 or rests on one or two draws,
and the rule would compare noise; P(eta1 > 0) is 0.019 and 0.030.

Thinning.  Rows 16 iterations apart are close enough to independent for (c): no wider thinning was needed.  Measured with the
restatement of the chain (seed 21; n under model 0 from 43 to 78, under model 1 from 50 to 85), deviations in standard errors, fixture
rows 1 | 2:
    mean      alpha0 +1.63 | -1.73   alpha1 +0.28 | -0.90   eta1_0 +0.28 | +1.47
    P(> 0)                                                  eta1_0 -0.35 | +1.28
    q 2.5     alpha0 +1.90 | +0.04   alpha1 -0.61 | -1.16   eta1_0 +1.45 | +0.79
    q 50      alpha0 +0.62 | -1.42   alpha1 -2.30 | +0.74   eta1_0 -1.12 | +0.30
    q 97.5    alpha0 -0.72 | -0.95   alpha1 -0.36 | -0.70   eta1_0 -0.96 | +0.93
The restatement of the chain takes about 18 ms per iteration whatever the number of features, so its 3072 iterations cost about a
minute; that is why the sampling phase is 2048 iterations and not the 4096 of tests/test_gpu_mmdiff_exact.py.  The replicates are the
full 512.
"""
import functools
import math
import os
import sys
from concurrent.futures import ProcessPoolExecutor

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mmdiff_effects_exact as XE  # noqa: E402
import mmdiff_effects_ref as E  # noqa: E402
import mmdiff_exact as X  # noqa: E402
from test_mmdiff_exact import check_against_exact, design, replicate  # noqa: E402

CASE, ROWS = "a_de33", (1, 2)
R, BURNIN, ITERS, THIN, PDASH, SEED = 512, 1024, 2048, 16, 0.2, 21
PCT = (2.5, 50.0, 97.5)
QUANTITIES = (("alpha0", 0, "alpha"), ("alpha1", 1, "alpha"), ("eta1_0", 1, "eta_0"))   # traced name, model, name in the exact module
P_GT0_OF = ("eta1_0",)
N_MIN, LEFT_OUT_MAX = 8, 0.05
# The same rule on design f_cov3 (three covariate columns, 12 samples; rows 1 and 2 again): every beta column of both models joins
# (a) and (c), and (b) takes the betas too, whose exact P(> 0) lies between 0.2 and 0.9.  p' = 0.5, at which these rows spend
# 0.55 and 0.65 of their time in model 1 (n from 29 to 75 rows under model 0, from 53 to 99 under model 1; none left out).
COV3 = dict(case="f_cov3", pdash=0.5, seed=22,
            quantities=(("alpha0", 0, "alpha"), ("alpha1", 1, "alpha"))
            + tuple(("beta%d_%d" % (m, j), m, "beta_%d" % j) for m in range(2) for j in range(3)) + (("eta1_0", 1, "eta_0"),),
            p_gt0_of=tuple("beta%d_%d" % (m, j) for m in range(2) for j in range(3)) + ("eta1_0",))
BASE = dict(case=CASE, pdash=PDASH, seed=SEED, quantities=QUANTITIES, p_gt0_of=P_GT0_OF)


# ----------------------------------------------------------------------------- the exact marginals against closed forms
def test_pinned_grid_is_one_gaussian():
    """lambda and sigma^2 pinned: the posterior of (alpha, beta, eta) is Gaussian with covariance (X' W X + V0^-1)^-1."""
    y, e, M, P0, P1, classes, _ = design("c_covariate")
    lam, sg = 0.7, 0.35
    Xd = np.concatenate([np.ones((6, 1)), M, P1], 1)
    W = np.diag(1.0 / (e * e + sg))
    A = Xd.T @ W @ Xd + np.diag([1 / 25.0, 1 / 4.0, 1 / lam])
    cov = np.linalg.inv(A)
    mean = cov @ Xd.T @ W @ y[2]
    at = (-0.5, 0.1, 2.0)
    got = XE.moments(y[2], e, M, P1, classes[:, 1], grid=X.Grid(pin=(lam, sg)), at=at)
    assert got["names"] == ["alpha", "beta_0", "eta_0"]
    assert np.allclose(got["mean"], mean, rtol=1e-12, atol=0) and np.allclose(got["sd"], np.sqrt(np.diag(cov)), rtol=1e-9, atol=0)
    from scipy.stats import norm
    want = norm.cdf((np.array(at)[None, :] - mean[:, None]) / np.sqrt(np.diag(cov))[:, None])
    assert np.allclose(got["cdf"], want, rtol=1e-10, atol=0)
    mix = XE.mixture(y[2], e, M, P1, classes[:, 1], grid=X.Grid(pin=(lam, sg)))
    assert mix.w.size == 1 and abs(mix.sd("eta_0") / math.sqrt(cov[2, 2]) - 1.0) < 1e-12
    assert abs(mix.p_gt0("beta_0") - (1.0 - norm.cdf(-mean[1] / math.sqrt(cov[1, 1])))) < 1e-12


def test_mixture_mean_is_the_posterior_mean():
    y, e, M, P0, P1, classes, kw = design("c_covariate")
    for m, P in ((0, P0), (1, P1)):
        pm = X.posterior_mean(y[1], e, M, P, classes[:, m], **kw)
        got = XE.moments(y[1], e, M, P, classes[:, m], **kw)
        want = np.concatenate([[pm["alpha"]], pm["beta"], pm["eta"]])
        assert np.all(np.abs(got["mean"] - want) <= 1e-12 * np.maximum(1.0, np.abs(want))), (got["mean"], want)
        mix = XE.mixture(y[1], e, M, P, classes[:, m], **kw)
        for i, name in enumerate(got["names"]):
            assert abs(mix.mean(name) - got["mean"][i]) < 1e-10 and abs(mix.sd(name) / got["sd"][i] - 1.0) < 1e-10
        assert mix.w.size < 0.5 * X._Model(y[1], e, M, P, classes[:, m], 1.4, 2.0, False, X.DEFAULT_GRID).size or m == 0


def _refinement_job(job):
    r, m = job
    y, e, M, P0, P1, classes, kw = design(CASE)
    P = (P0, P1)[m]
    base = XE.moments(y[r], e, M, P, classes[:, m], **kw)
    at = np.concatenate([[mu - sd, mu, mu + sd] for mu, sd in zip(base["mean"], base["sd"])])
    base = XE.moments(y[r], e, M, P, classes[:, m], at=at, **kw)
    fine = XE.moments(y[r], e, M, P, classes[:, m], at=at, grid=X.DEFAULT_GRID.refined(), **kw)
    p = base["sd"].size
    own = np.arange(p)[:, None] * 3 + np.arange(3)[None, :]          # coefficient i's own three points
    cdf = lambda a: np.take_along_axis(a["cdf"], own, 1)
    return base["names"], fine["sd"] / base["sd"] - 1.0, cdf(fine) / cdf(base) - 1.0


def test_grid_refinement_moves_sd_and_cdf_by_less_than_1e_6():
    """Half the step and both ranges wider by 5 at each end, for the two fixture rows of the statistical test and both models: the
    relative movement of the sd and of F at mean - sd, mean, mean + sd of every coefficient.  Model 1's refined grid has 41 million
    nodes and takes a little over two minutes; the two rows run side by side.  Measured, the largest movements:
        row 1   model 0: sd 0, F 8e-15        model 1: sd 8.4e-09 (alpha), F 2.0e-08 (alpha at its mean and mean + sd)
        row 2   model 0: sd 2.5e-14, F 1e-15  model 1: sd 2.6e-12, F 4.0e-12"""
    jobs = [(r, m) for r in ROWS for m in (1, 0)]
    with ProcessPoolExecutor(min(2, os.cpu_count() or 1)) as ex:
        got = list(ex.map(_refinement_job, jobs))
    for (r, m), (nm, dsd, dcdf) in zip(jobs, got):
        print("refinement row %d model %d %s: sd moves by %s, F by %s" % (r, m, nm, dsd, dcdf.ravel()))
    for (r, m), (nm, dsd, dcdf) in zip(jobs, got):
        assert np.all(np.abs(dsd) < 1e-6) and np.all(np.abs(dcdf) < 1e-6), (r, m)


# ----------------------------------------------------------------------------- the statistical rule
def stat_inputs(case=CASE):
    """y (2 R, N), e (2 R, N), M, P0, P1, classes and the keyword arguments of the design: row ROWS[i] is features i R .. i R + R - 1."""
    y, e, M, P0, P1, classes, kw = design(case)
    return replicate(y[list(ROWS)], R), np.tile(e, (len(ROWS) * R, 1)), M, P0, P1, classes, kw


STAT_GRID = X.DEFAULT_GRID.coarsened(0.5)


@functools.lru_cache(maxsize=None)
def exact_mixtures(case=CASE):
    """The exact marginals of the statistical rule, on half the default grid's points per axis: a second for both rows instead of
    eleven, so that the device test stays short.  test_half_the_grid_points_move_nothing_the_rule_can_see bounds what that costs.
    (f_cov3: model 1's grid has three dimensions, 250 880 nodes of which 24 000 carry the weight; six seconds for both rows.)"""
    y, e, M, P0, P1, classes, kw = design(case)
    return [[XE.mixture(y[r], e, M, P, classes[:, m], grid=STAT_GRID, **kw) for m, P in ((0, P0), (1, P1))] for r in ROWS]


def _half_grid_moves(case, rows):
    y, e, M, P0, P1, classes, kw = design(case)
    for r in rows:
        for m, P in ((0, P0), (1, P1)):
            base = XE.moments(y[r], e, M, P, classes[:, m], **kw)
            at = np.concatenate([[mu + k * sd for k in (-2, -1, 0, 1, 2)] for mu, sd in zip(base["mean"], base["sd"])])
            base = XE.moments(y[r], e, M, P, classes[:, m], at=at, **kw)
            half = XE.moments(y[r], e, M, P, classes[:, m], at=at, grid=STAT_GRID, **kw)
            moved = (np.abs(half["mean"] - base["mean"]).max(), np.abs(half["sd"] / base["sd"] - 1.0).max(), np.abs(half["cdf"] - base["cdf"]).max())
            print("half grid, %s row %d model %d: mean %.1e sd %.1e F %.1e" % ((case, r, m) + moved))
            assert max(moved) < 1e-6, (case, r, m, moved)


def test_half_the_grid_points_move_nothing_the_rule_can_see():
    """STAT_GRID against the default grid, both fixture rows and models: mean, sd (relative) and F at mean, mean +- sd, mean +- 2 sd.
    Measured for model 1: mean 6.5e-08, sd 1.1e-07, F 9.3e-08; the rule's standard errors are 1e-3.  (0.35 of the points: 3.8e-05.)"""
    _half_grid_moves(CASE, ROWS)


def test_half_the_grid_points_move_nothing_the_rule_can_see_with_three_covariates():
    """The same for f_cov3, one row (the default grid of its model 1 has two million nodes and takes a minute).  Measured for model 1:
    mean 1.8e-08, sd 8.5e-08, F 5.5e-08."""
    _half_grid_moves(COV3["case"], ROWS[:1])


def check_effects_against_exact(fx, what, cfg=None):
    """fx: the dict of mmdiff_effects_ref.effects / Diff.effects over the features of stat_inputs() with percentiles PCT.  Prints every
    figure, then asserts (a), (b) and (c) of the module's docstring.  cfg: BASE (the default) or COV3."""
    cfg = cfg or BASE
    names = list(fx["names"])
    mix = exact_mixtures(cfg["case"])
    failures = []

    def rule(est, exact, label):
        try:
            check_against_exact(est, exact, "%s %s" % (what, label))
        except AssertionError as ex:
            failures.append((label, str(ex)))

    for name, m, cname in cfg["quantities"]:
        s = names.index(name)
        n = fx["n"][m].astype(np.float64).reshape(len(ROWS), R)
        ok = n >= N_MIN
        print("%s %s: n under model %d min %d mean %.1f max %d, left out %s" % (what, name, m, n.min(), n.mean(), n.max(), (~ok).sum(1)))
        assert np.all((~ok).mean(1) <= LEFT_OUT_MAX), (name, (~ok).sum(1))
        rule(fx["mean"][s].reshape(len(ROWS), R), [mx[m].mean(cname) for mx in mix], name + " mean")
        for i in range(len(ROWS)):
            k = ok[i]
            ni = n[i][k]
            if name in cfg["p_gt0_of"]:
                p_gt = fx["n_gt"][s].reshape(len(ROWS), R)[i][k] / ni
                rule(p_gt[None, :], [mix[i][m].p_gt0(cname)], "%s row %d P(> 0)" % (name, ROWS[i]))
            # (c)
            for j, p in enumerate(PCT):
                picked = np.array([E.picked_index(p, int(v)) for v in ni], np.float64)
                Fq = mix[i][m].cdf(cname, fx["q"][s, j].reshape(len(ROWS), R)[i][k])
                rule((Fq - (picked + 1.0) / (ni + 1.0))[None, :], [0.0], "%s row %d F(q%g) - (k + 1) / (n + 1)" % (name, ROWS[i], p))
    assert not failures, failures


def test_restated_effects_match_the_exact_posterior(orc):
    """The restatement of the summaries on the rows of the restatement of the chain (tests/mmdiff_trace_ref.py), no device."""
    import mmdiff_trace_ref as TR
    y, e, M, P0, P1, classes, kw = stat_inputs()
    b = TR.TracedBMS(y, e, M, P0, P1, classes, pdash=PDASH, seed=SEED, every_burnin=BURNIN, every_sample=THIN, **kw)
    b.burnin(BURNIN)
    b.sample(ITERS)
    rows = b.stacked(1)
    names = b.names()
    assert rows.shape == (ITERS // THIN, len(names), len(ROWS) * R)
    fx = E.effects(rows, E.model_of_names(names[:-1]), PCT)
    fx["names"] = names[:-1]
    check_effects_against_exact(fx, "restatement")


def test_restated_effects_match_the_exact_posterior_with_three_covariates(orc):
    """As above on design f_cov3 (COV3): 21 traced parameters, the summaries of six beta columns among them.  Measured: the 86
    deviations lie between -1.60 and +2.17 standard errors; the device's own rows give the same figures
    (tests/test_gpu_mmdiff_effects.py).  The restatement of the chain takes about a minute and a half here."""
    import mmdiff_trace_ref as TR
    y, e, M, P0, P1, classes, kw = stat_inputs(COV3["case"])
    b = TR.TracedBMS(y, e, M, P0, P1, classes, pdash=COV3["pdash"], seed=COV3["seed"], every_burnin=BURNIN, every_sample=THIN, **kw)
    b.burnin(BURNIN)
    b.sample(ITERS)
    rows = b.stacked(1)
    names = b.names()
    assert rows.shape == (ITERS // THIN, len(names), len(ROWS) * R)
    fx = E.effects(rows, E.model_of_names(names[:-1]), PCT)
    fx["names"] = names[:-1]
    check_effects_against_exact(fx, "restatement f_cov3", COV3)
