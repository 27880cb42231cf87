"""tests/pooled_ref.py, the specification of mmg_pooled_*, checked on its own: order statistics against np.sort, the pooled variance
against np.var of the pooled logged draws, one chain against contrast_ref.sokal, and the Monte Carlo error of independent chains."""
import math

import numpy as np
import pytest

import contrast_ref as CR
import pooled_ref as P


def _positive(rng, C, S, count):
    x = np.exp(rng.normal(size=(C, S, count)))
    x[:, :, 1::4] = rng.integers(1, 5, size=x[:, :, 1::4].shape)      # heavy ties
    return x


@pytest.mark.parametrize("C,S,count", [(1, 64, 5), (3, 100, 7), (4, 256, 6), (2, 5, 3), (5, 1, 2)])
def test_percentiles_are_the_sorted_pooled_draws(C, S, count):
    rng = np.random.default_rng(C * 100 + S)
    x = _positive(rng, C, S, count)
    N = C * S
    pidx = [0, N // 3, N - 1, -1, N]
    r = P.pooled_of_traces(x, pidx)
    for i in range(count):
        srt = np.sort(x[:, :, i].ravel())
        assert np.array_equal(r["percentiles"][i, :3], srt[[0, N // 3, N - 1]])
        assert np.isnan(r["percentiles"][i, 3:]).all()
    x[0, 0, 0] = np.nan                                               # a NaN sorts last
    r = P.pooled_of_traces(x, [N - 2, N - 1])
    assert r["percentiles"][0, 0] == np.nanmax(x[:, :, 0]) and np.isnan(r["percentiles"][0, 1])


@pytest.mark.parametrize("C,S", [(2, 64), (4, 256), (3, 100), (7, 8), (2, 5)])
def test_var_is_the_sample_variance_of_the_pooled_logged_draws(C, S):
    rng = np.random.default_rng(C + S)
    x = _positive(rng, C, S, 9)
    x[1] *= 3.0                                                       # a shifted chain: the between-chain term matters
    r = P.pooled_of_traces(x)
    want_var = np.var(np.log(x).reshape(C * S, -1), axis=0, ddof=1)
    want_mean = np.log(x).reshape(C * S, -1).mean(axis=0)
    np.testing.assert_allclose(r["log_mean"], want_mean, rtol=1e-12, atol=1e-14)
    if S & (S - 1):
        # Sokal refuses the length: the chains' variances come as zeros and var is the formula on them, the between-chain term alone
        assert (r["rc"] == 201).all() and (r["tau"] == 0).all() and (r["mcse2"] == 0).all() and (r["c_var"] == 0).all()
        between = S * ((r["c_mean"] - r["log_mean"][:, None]) ** 2).sum(axis=1) / (C * S - 1)
        np.testing.assert_allclose(r["var"], between, rtol=1e-12)
    else:
        assert (r["rc"] == 0).all()
        np.testing.assert_allclose(r["var"], want_var, rtol=1e-12)
        # mcse2 = tau W / N with W the mean within-chain variance
        W = r["c_var"].mean(axis=1)
        np.testing.assert_allclose(r["mcse2"], r["tau"] * W / (C * S), rtol=1e-12)


@pytest.mark.parametrize("S", [4, 64, 1024, 100, 3])
def test_one_chain_is_contrast_refs_sokal(S):
    rng = np.random.default_rng(S)
    x = _positive(rng, 1, S, 6)
    r = P.pooled_of_traces(x, [0, S - 1])
    for i in range(6):
        y = np.log(x[0, :, i])
        rc, var, tau = CR.sokal(y)
        acc = np.float64(0.0)
        for s in range(S):
            acc = acc + y[s]
        assert r["rc"][i] == rc and r["var"][i] == var and r["tau"][i] == tau and r["log_mean"][i] == acc / S
        assert r["mcse2"][i] == tau * var / S
        assert r["c_mean"][i, 0] == r["log_mean"][i] and r["c_var"][i, 0] == var and r["c_tau"][i, 0] == tau and r["c_rc"][i, 0] == rc


def test_sokal_batch_is_sokal_row_by_row():
    rng = np.random.default_rng(5)
    Y = rng.normal(size=(40, 128))
    Y[3] = 2.0                                                        # constant: r0 = 0, NaN propagates
    Y[4, 7] = np.inf
    phi = 0.95
    for s in range(1, 128):
        Y[5, s] = phi * Y[5, s - 1] + Y[5, s]
    rc, var, tau = P.sokal_batch(Y)
    for i in range(40):
        r, v, t = CR.sokal(Y[i])
        assert rc[i] == r and np.array_equal([var[i], tau[i]], [v, t], equal_nan=True), i


def test_independent_chains_have_tau_near_one():
    """C iid chains of iid draws: mcse2 N / var estimates tau = 1.  Sokal's estimator is tau_hat = 1 + 2 sum_{k=1}^{M} rho_hat_k with the
    window M the first m - 1 at which -1/3 + sum_{i<m} (rho_hat_i - 1/6) < 0; with rho_hat_k near 0 the running sum passes 1/2, 1/3, 1/6,
    0, -1/6 at m = 1 .. 5, so M is 4 give or take the noise, and M <= 6 covers it.  For iid draws the rho_hat_k, k >= 1, are
    asymptotically independent with variance 1 / S and mean -1 / S, so var(tau_hat) <= 4 M / S and the bias is -2 M / S.  A series' ratio
    is the var_c-weighted mean of C independent tau_hat_c times W / var, whose relative error has variance about 2 / N: its standard
    deviation is at most sigma = sqrt(4 M / (S C)) + sqrt(2 / N).  Every series must lie within 6 sigma + the bias of 1, and the mean
    over K independent series within 4 sigma / sqrt(K) + the bias."""
    C, S, K, M = 4, 1024, 64, 6
    rng = np.random.default_rng(11)
    x = np.exp(rng.normal(size=(C, S, K)))
    r = P.pooled_of_traces(x)
    N = C * S
    ratio = r["mcse2"] * N / r["var"]
    sigma = math.sqrt(4.0 * M / (S * C)) + math.sqrt(2.0 / N)
    bias = 2.0 * M / S
    print("ratio: min %.4f mean %.4f max %.4f; sigma %.4f bias %.4f" % (ratio.min(), ratio.mean(), ratio.max(), sigma, bias))
    assert np.all(np.abs(ratio - 1.0) <= 6 * sigma + bias)
    assert abs(ratio.mean() - 1.0) <= 4 * sigma / math.sqrt(K) + bias
    np.testing.assert_allclose(r["tau"], ratio * r["var"] / r["c_var"].mean(axis=1), rtol=1e-12)


def test_proportions():
    from scipy.special import ndtri
    rng = np.random.default_rng(3)
    C, S, count = 3, 40, 5
    p = rng.uniform(0, 1, size=(C, S, count))
    p[:, :, 1] = 1.0
    p[0, 3, 2] = 0.0                                                  # clamped to 1e-9
    multi = np.array([True, False, True, True, True])
    N = C * S
    r = P.pooled_proportions(p, multi, [0, N - 1, N])
    flat = p.reshape(N, count)
    np.testing.assert_allclose(r["mean"], flat.mean(axis=0), rtol=1e-13)
    z = ndtri(np.clip(flat, 1e-9, 1 - 1e-9))
    ok = multi
    np.testing.assert_allclose(r["probit_mean"][ok], z.mean(axis=0)[ok], rtol=1e-12)
    np.testing.assert_allclose(r["probit_sd"][ok], z.std(axis=0, ddof=1)[ok], rtol=1e-10)
    assert r["probit_mean"][1] == np.inf and np.isnan(r["probit_sd"][1])
    assert np.array_equal(r["percentiles"][:, :2], np.sort(flat, axis=0)[[0, N - 1]].T) and np.isnan(r["percentiles"][:, 2]).all()
    one = P.pooled_proportions(p[:1], multi)
    s1 = np.add.accumulate(ndtri(np.clip(p[0, :, 0], 1e-9, 1 - 1e-9)))[-1]
    assert one["probit_mean"][0] == s1 / S                            # one chain: the single chain's sequential sums
