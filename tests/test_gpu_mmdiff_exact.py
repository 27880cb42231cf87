"""mmdiff on the device against exact marginal likelihoods (tests/mmdiff_exact.py through tests/golden/mmdiff_exact.json).

Every other device test of mmdiff compares the kernels with tests/mmdiff_ref.py, which restates them; these compare what the
chain estimates with what the model says it must be.  Each of the three fixture rows is replicated R times, every replicate a
feature of its own and so an independent chain, and runs 1024 burn-in and 4096 sampling iterations.  The rule
(test_mmdiff_exact.check_against_exact): the replicates' mean is within 5 s.e. of the exact value, the s.e. from the replicates'
own spread; for mean gamma the s.e. on the logit scale is at most 0.02 and no replicate sits at 0 or 1.  The seeds are fixed and
the runs bit-reproducible, so the outcome is deterministic.

Compared: mean gamma with sigmoid(logit p' + log BF), and the printed within-model means of alpha, beta and eta with their
posterior means.  beta is the exception in what it estimates: as in src/bms.cpp:650-656 its sums also take the draws from the
pseudoprior while the other model is the fitted one, and the pseudoprior's mean is the burn-in's own estimate of the same
posterior mean, so the expectation is still E[beta | y, model] up to the burn-in's transient.

Measured at R = 512 and 4096 iterations without tuning, seed 11, with tests/mmdiff_ref.py on the CPU, which the device equals bit for
bit on these paths (tests/test_gpu_mmdiff.py); not yet measured on a device, and the tuned, p' = 0.2, chains (with the ratio of
log_bf_mcse to the observed spread) and CLI paths have no recorded figures yet.  Rows 0, 1, 2:
    design       s.e. of mean gamma on the logit scale   logit(mean gamma) - exact log BF   deviation in s.e.
    a_de33       0.0057  0.0052  0.0028                  +0.0094  -0.0041  +0.0034          +1.65  -0.78  +1.21
    b_fixalpha   0.0024  0.0029  0.0025                  +0.0029  -0.0014  +0.0003          +1.18  -0.47  +0.11
    c_covariate  0.0063  0.0049  0.0028                  +0.0013  -0.0031  -0.0027          +0.21  -0.62  -0.94
The within-model means (alpha, beta, eta of both models) of these three runs deviate by at most 2.9 s.e. (beta0 of c_covariate's
second row; every other one below 2.3).  Before the exact reference dropped the eta column it had given model 0 of `-de`, the same
comparison showed a shift of about -0.05 in log BF on every row of a_de33, 9 to 18 of these standard errors.
The designs of tests/wide_designs.py (three covariate columns; two with -fixalpha; a fitted model 0 with two variance classes and two
eta columns in model 1), measured on an MI355X with the same R, iterations and seed:
    f_cov3           0.0059  0.0035  0.0027          +0.0041  +0.0014  +0.0012          +0.69  +0.41  +0.46
    g_cov2_fixalpha  0.0043  0.0047  0.0038          -0.0050  -0.0065  +0.0009          -1.14  -1.38  +0.25
    h_batch          0.0045  0.0034  0.0024          -0.0046  +0.0047  +0.0029          -1.02  +1.41  +1.25
Their within-model means -- every beta column of both models, model 0's eta, every eta column of model 1 -- deviate by at most 2.83
s.e. among f_cov3's 27 (beta1_2, second row), 2.21 among g_cov2_fixalpha's 15 and 2.58 among h_batch's 15.  f_cov3 with the tuning
loop (seed 13): mean gamma -0.63, -0.27, -1.26 s.e., means at most 1.95; its pooled log BF of four chains (seed 14) -0.75, -0.78,
-1.05 s.e., means at most 1.62, log_bf_mcse over the observed spread 0.84, 1.08, 1.10.
"""
import math
import subprocess

import numpy as np
import pytest

from test_mmdiff_exact import check_against_exact, check_means, design, golden, replicate
from test_gpu_mmdiff import MMDIFF, write_tables

R = 512
BURNIN, ITERS = 1024, 4096


def _sig(x):
    x = np.asarray(x, np.float64)
    return 1.0 / (1.0 + np.exp(-x))


def _inputs(case, reps):
    y, e, M, P0, P1, classes, kw = design(case)
    return replicate(y, reps), np.tile(e, (3 * reps, 1)), M, P0, P1, classes, kw


def _check_gamma(gamma_mean, logitp, g, reps, what):
    """Each replicate's mean gamma has expectation s_f = sigmoid(logit p'_f + log BF).  p' may differ between replicates (tuning), so
    the estimate is gamma_f - s_f recentred at the replicates' mean s; without tuning this is gamma_f itself."""
    b = np.repeat(np.array(g["log_bf"]), reps)
    s = _sig(logitp + b).reshape(3, reps)
    est = gamma_mean.reshape(3, reps) - s + s.mean(1, keepdims=True)
    raw = gamma_mean.reshape(3, reps)
    assert np.all((raw > 0.0) & (raw < 1.0)), "%s: a replicate never left one model" % what
    return check_against_exact(est, s.mean(1), what + " gamma", logit_cap=True)


def _check_means(res, g, reps, what):
    """alpha of both models, every beta column of both models, model 0's eta where model 0 has one, every eta column of model 1."""
    check_means(res, g, reps, what)


def _run(case, pdash=0.5, tune=False, seed=11):
    from mmseq_amd.diff import Diff
    y, e, M, P0, P1, classes, kw = _inputs(case, R)
    d = Diff(y, e, M, P0, P1, classes, pdash=pdash, seed=seed, **kw)
    d.burnin(BURNIN)
    nb = d.tune() if tune else 0
    d.sample(ITERS)
    res = d.results()
    d.close()
    return res, nb


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["a_de33", "b_fixalpha", "c_covariate", "d_de66", "e_d3_s05", "f_cov3", "g_cov2_fixalpha", "h_batch"])
def test_notune_matches_the_exact_model_probability(gpu, case):
    res, _ = _run(case)
    assert np.all(res["logitp"] == 0.0)
    g = golden()[case]
    _check_gamma(res["gamma_mean"], res["logitp"], g, R, case + " notune")
    _check_means(res, g, R, case + " notune")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["a_de33", "c_covariate"])
def test_fixed_pdash_does_not_move_the_bayes_factor(gpu, case):
    """p' = 0.2 without tuning: mean gamma follows sigmoid(logit 0.2 + log BF), so the Bayes factor formed from it is the same."""
    res, _ = _run(case, pdash=0.2, seed=12)
    assert np.allclose(res["logitp"], math.log(0.25), rtol=1e-15, atol=0)
    g = golden()[case]
    _check_gamma(res["gamma_mean"], res["logitp"], g, R, case + " pdash 0.2")
    _check_means(res, g, R, case + " pdash 0.2")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["a_de33", "c_covariate", "f_cov3"])
def test_default_tuning_matches_the_exact_model_probability(gpu, case):
    res, nb = _run(case, tune=True, seed=13)
    assert nb >= 2 and np.unique(res["logitp"]).size > 1      # tuning moved some feature's p'
    g = golden()[case]
    _check_gamma(res["gamma_mean"], res["logitp"], g, R, case + " tuned")
    _check_means(res, g, R, case + " tuned")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["a_de33", "c_covariate", "f_cov3"])
def test_chains_pooled_log_bf_and_its_mcse(gpu, case):
    """4 chains, 128 replicates, every chain tuned on its own: the pooled log BF against the exact one, and the reported Monte Carlo
    standard error against the replicates' observed spread of the pooled log BF (within a factor 2: 16 batch means carry about 18 %
    relative error per feature, and autocorrelation biases them low)."""
    from mmseq_amd.diff import DiffChains
    reps, C = 128, 4
    y, e, M, P0, P1, classes, kw = _inputs(case, reps)
    d = DiffChains(y, e, M, P0, P1, classes, C, ITERS, seed=14, **kw)
    d.burnin(BURNIN)
    d.tune()
    d.sample(ITERS)
    d.pool()
    res = d.pooled()
    d.close()
    g = golden()[case]
    lb = res["log_bf"].reshape(3, reps)
    assert np.all(np.isfinite(lb)) and np.all(res["chains_mixed"] == C)
    check_against_exact(lb, g["log_bf"], case + " chains log_bf")
    _check_means(res, g, reps, case + " chains")
    ratio = res["log_bf_mcse"].reshape(3, reps).mean(1) / lb.std(1, ddof=1)
    print(case, "mean log_bf_mcse / observed sd of log_bf:", ratio)
    assert np.all((ratio >= 0.5) & (ratio <= 2.0)), ratio


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["a_de33", "c_covariate"])
def test_cli_bayes_factor_and_posterior_probability(gpu, tmp_path, case):
    """The printed columns: bayes_factor = g / (1 - g) * (1 - p') / p' and posterior_probability = sigmoid(logit p + log BF), here with
    p' = 0.2 and p = 0.3.  Each is mapped back to the mean gamma it was formed from and goes through the same rule."""
    pdash, p = 0.2, 0.3
    y, e, M, P0, P1, classes, kw = _inputs(case, R)
    files = write_tables(tmp_path, y, e, np.ones_like(y))
    args = ["-nonorm", "-notune", "-pdash", str(pdash), "-p", str(p), "-burnin", str(BURNIN), "-iter", str(ITERS), "-seed", "15"]
    if case == "c_covariate":
        mat = tmp_path / "design.txt"
        mat.write_text("# covariate\n" + "".join("%r\n" % float(v) for v in M[:, 0]) + "\n" + "".join("%d %d\n" % tuple(c) for c in classes)
                       + "\n1\n\n0.5\n-0.5\n")
        args += ["-m", str(mat)]
    else:
        args += ["-de", "3", "3"]
    r = subprocess.run([MMDIFF] + args + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    lines = r.stdout.decode().rstrip("\n").split("\n")
    assert lines[0] == "#prior_probability=0.3"
    hdr = lines[1].split("\t")
    assert hdr[:3] == ["feature_id", "bayes_factor", "posterior_probability"]
    rows = [l.split("\t") for l in lines[2:]]
    assert [r_[0] for r_ in rows] == ["f%d" % i for i in range(3 * R)]
    bf = np.array([float(r_[1]) for r_ in rows])
    pp = np.array([float(r_[2]) for r_ in rows])
    odds_dash, odds_p = pdash / (1 - pdash), p / (1 - p)
    g_bf = bf * odds_dash / (1.0 + bf * odds_dash)
    bf_pp = pp / (1.0 - pp) / odds_p
    g_pp = bf_pp * odds_dash / (1.0 + bf_pp * odds_dash)
    g = golden()[case]
    logitp = np.full(3 * R, math.log(odds_dash))
    _check_gamma(g_bf, logitp, g, R, case + " cli bayes_factor")
    _check_gamma(g_pp, logitp, g, R, case + " cli posterior_probability")
    a0 = np.array([float(r_[hdr.index("alpha0")]) for r_ in rows])
    e1 = np.array([float(r_[hdr.index("eta1_0")]) for r_ in rows])
    check_against_exact(a0.reshape(3, R), g["alpha0"], case + " cli alpha0")
    check_against_exact(e1.reshape(3, R), g["eta1"], case + " cli eta1")
