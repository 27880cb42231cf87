"""CPU checks of tests/convergence_ref.py, the restatement the device diagnostics are tested against: known answers of the rank-normalized
split R-hat and the bulk / tail ESS."""
import math

import numpy as np
from scipy.special import ndtri
from scipy.stats import rankdata

import convergence_ref as R


def ar1(rng, C, S, phi):
    x = np.empty((C, S))
    x[:, 0] = rng.normal(size=C) / math.sqrt(1 - phi * phi)
    e = rng.normal(size=(C, S))
    for s in range(1, S):
        x[:, s] = phi * x[:, s - 1] + e[:, s]
    return x


def test_monotone_transforms_leave_the_bulk_statistics_alone():
    rng = np.random.default_rng(1)
    x = ar1(rng, 4, 300, 0.5)
    a = R.diagnostics(x)
    for y in (np.exp(x), 3 * x + 1):
        b = R.diagnostics(y)
        assert b["rhat_bulk"] == a["rhat_bulk"] and b["ess_bulk"] == a["ess_bulk"]


def test_iid_normal_chains_mix():
    rng = np.random.default_rng(2)
    d = R.diagnostics(rng.normal(size=(4, 1000)))
    assert abs(d["rhat"] - 1) < 0.01
    assert abs(d["ess_bulk"] - 4000) < 0.2 * 4000


def test_ar1_bulk_ess_follows_the_autocorrelation():
    rng = np.random.default_rng(3)
    phi = 0.9
    d = R.diagnostics(ar1(rng, 4, 5000, phi))
    want = 20000 * (1 - phi) / (1 + phi)
    assert abs(d["ess_bulk"] - want) < 0.25 * want


def test_a_shifted_chain_is_caught():
    rng = np.random.default_rng(4)
    x = rng.normal(size=(4, 1000))
    x[2] += 3.0
    # On ranks a chain that sits wholly above the other three scores like their top quarter however far it is shifted: R-hat
    # saturates near 1.47 (3 sd already separate the chain almost completely), so 1.5 is out of reach and 1.4 is the bound here.
    # The R-hat of the raw draws, the same formula without the rank normalization, is well above 1.5.
    assert R.diagnostics(x)["rhat"] > 1.4
    assert R.rhat_split(R.split(x)) > 1.5


def test_a_wider_chain_shows_in_the_tail_rhat_only():
    rng = np.random.default_rng(5)
    x = rng.normal(size=(4, 2000))
    x[1] *= 4.0
    d = R.diagnostics(x)
    assert d["rhat_bulk"] < 1.02 and d["rhat_tail"] > 1.05
    assert d["rhat"] == d["rhat_tail"]


def test_tiny_case_computed_literally():
    x = np.array([[3.0, 1.0, 7.0, 2.0, 5.0]])      # C = 1, S = 5: halves [3, 1] and [2, 5], the middle 7 dropped
    d = R.diagnostics(x)
    y = np.array([[3.0, 1.0], [2.0, 5.0]])
    # ranks among 1, 2, 3, 5: 3 -> 3, 1 -> 1, 2 -> 2, 5 -> 4
    z = ndtri((np.array([[3.0, 1.0], [2.0, 4.0]]) - 0.375) / 4.25)
    N, M = 2, 2
    m = z.mean(axis=1)
    W = np.mean([((z[j] - m[j]) ** 2).sum() / (N - 1) for j in range(M)])
    B = N * ((m - m.mean()) ** 2).sum() / (M - 1)
    rb = math.sqrt(((N - 1) / N * W + B / N) / W)
    assert d["rhat_bulk"] == rb
    med = (2.0 + 3.0) / 2                           # sorted 1, 2, 3, 5
    zf = ndtri((rankdata(np.abs(y - med).ravel()).reshape(2, 2) - 0.375) / 4.25)
    assert d["rhat_tail"] == R.rhat_split(zf)
    assert d["rhat"] == max(rb, d["rhat_tail"])
    # N = 2: Geyer's loop never runs (t < N - 3 is false), tau is its floor 1 / log10(P): ESS = P log10(P)
    assert d["ess_bulk"] == 4 / (1 / math.log10(4))


def test_constant_series_is_nan():
    d = R.diagnostics(np.full((3, 10), 2.5))
    assert all(math.isnan(d[k]) for k in ("rhat", "ess_bulk", "ess_tail"))


def test_odd_length_drops_the_middle_draw():
    rng = np.random.default_rng(6)
    x = rng.normal(size=(3, 41))
    y = x.copy()
    y[:, 20] = 1e6                                  # the middle draws: no part of any statistic
    a, b = R.diagnostics(x), R.diagnostics(y)
    for k in ("rhat", "ess_bulk", "ess_tail"):
        assert a[k] == b[k]
    assert np.array_equal(R.split(x), np.concatenate([x[:, :20], x[:, 21:]], axis=1).reshape(3, 2, 20).reshape(6, 20))
