"""tests/pairs_ref.py, the specification of mmg_pairs_* (DESIGN.md section 15), on the CPU: its symmetries, its accuracy against
np.longdouble, what non-finite samples give, and the statistical reading of its columns on the oracle's chain."""
import numpy as np
import pytest

import pairs_ref as R


def _traces(rng, n, S, sd=None):
    sd = np.exp(rng.uniform(np.log(1e-3), np.log(3.0), n)) if sd is None else sd
    return np.exp(rng.normal(-8.0, 3.0, n)[:, None] + sd[:, None] * rng.normal(0.0, 1.0, (n, S))), sd


def _same(x, y):
    return np.array_equal(x, y, equal_nan=True)


def test_symmetry_and_independence_of_pairing():
    rng = np.random.default_rng(1)
    n, S = 12, 200
    tr, _ = _traces(rng, n, S)
    tr[7] = tr[3]                                                  # two identical rows
    pairs = [(0, m) for m in range(1, n)] + [(5, 2), (2, 5), (3, 7), (4, 9), (4, 9), (9, 0)]
    s = R.summary_ref(tr, pairs)
    ab, ba = pairs.index((5, 2)), pairs.index((2, 5))
    for x, y in (("mean_a", "mean_b"), ("saa", "sbb"), ("sab", "sab"), ("sss", "sss"), ("mean_sum", "mean_sum"), ("sd_a", "sd_b"),
                 ("cor", "cor"), ("sd_sum", "sd_sum")):
        assert s[x][ab] == s[y][ba] and s[y][ab] == s[x][ba], (x, y)
    assert s["n_gt"][ab] + s["n_gt"][ba] == S                      # (continuous values: no ties)
    assert s["n_gt"][ab] == (tr[5] > tr[2]).sum() and s["n_gt"][ba] == (tr[2] > tr[5]).sum()
    # a member's numbers carry the same bits in every pair it is in, on either side
    stats = {}
    for p, (a, b) in enumerate(pairs):
        for m, mean, sq in ((a, s["mean_a"][p], s["saa"][p]), (b, s["mean_b"][p], s["sbb"][p])):
            assert stats.setdefault(m, (mean, sq)) == (mean, sq), (p, m)
    assert len(stats) == n
    i, j = pairs.index((4, 9)), pairs.index((4, 9)) + 1            # one pair twice: the same numbers
    assert all(s[k][i] == s[k][j] for k in s)
    # alone or among others: the same bits
    alone = R.summary_ref(tr, [(5, 2)])
    assert all(alone[k][0] == s[k][ab] for k in s)
    q = pairs.index((3, 7))
    assert abs(s["cor"][q] - 1.0) <= 2 * np.finfo(float).eps
    # x + x = 2 x exactly and log(2 x) = log 2 + log x up to roundings of a number near 8: the spread is sd_a's
    assert abs(s["sd_sum"][q] - s["sd_a"][q]) <= 1e-12 and s["sd_a"][q] == s["sd_b"][q]


@pytest.mark.parametrize("S", [2, 65, 1024])
def test_reference_against_longdouble(S):
    """The bound of two-pass centring, with e = 2^-53, u the logarithms of a series, m their mean, s^2 S = sum (u - m)^2 and
    U = max |u|:

    * every u carries a relative error of at most 1 e from the logarithm (np.log is within an ulp), so an absolute e U;
    * the mean m' of S terms summed in a tree of depth <= S / 64 + 6 carries at most (S / 64 + 7) e U, and its error moves every
      centred value by the same amount, which cancels to first order in sum (u - m')^2 = sum (u - m)^2 + S (m - m')^2;
    * a centred value d = u - m' is then off by at most 2 e U (the logarithm's error and the subtraction's rounding of a number
      below 2 U in size), so d * d is off by at most 2 |d| 2 e U + (2 e U)^2 + e d^2;
    * summed over S terms with Cauchy-Schwarz (sum |d| <= S s): |saa' - saa| <= 4 e U S s + S (2 e U)^2 + S (m - m')^2
      + (S / 64 + 8) e saa.

    Relative to saa = S s^2 that is  4 e (U / s) + (S / 64 + 8) e + [(2 e U)^2 + ((S / 64 + 7) e U)^2] / s^2: the first term
    is what two-pass centring guarantees -- linear in U / s where the one-pass form is quadratic -- and the test allows exactly
    this sum (doubled for the cross term sab against sqrt(saa sbb), whose two factors each carry the error).  The means are held to
    (S / 64 + 8) e U."""
    rng = np.random.default_rng(100 + S)
    n = 24
    tr, _ = _traces(rng, n, S)
    pairs = [(int(a), int(b)) for a, b in zip(rng.permutation(n), np.roll(rng.permutation(n), 1)) if a != b] + [(0, 1), (1, 0)]
    got = R.pairs_ref(tr, pairs)
    e = 2.0 ** -53
    x = tr.astype(np.longdouble)
    depth = S / 64.0 + 8.0

    def exact(series):
        u = np.log(series)
        m = u.sum() / S
        return u, m, u - m

    def rel_bound(U, s2S):
        s = np.sqrt(float(s2S) / S)
        return 4 * e * U / s + depth * e + ((2 * e * U) ** 2 + (depth * e * U) ** 2) / s ** 2

    for p, (a, b) in enumerate(pairs):
        ua, ma, da = exact(x[a])
        ub, mb, db = exact(x[b])
        uw, mw, dw = exact(x[a] + x[b])
        for name, m, u in (("mean_a", ma, ua), ("mean_b", mb, ub), ("mean_sum", mw, uw)):
            assert abs(got[name][p] - m) <= depth * e * float(np.abs(u).max()), (p, name)
        ra, rb, rw = (rel_bound(float(np.abs(u).max()), (d * d).sum()) for u, d in ((ua, da), (ub, db), (uw, dw)))
        for name, d, r in (("saa", da, ra), ("sbb", db, rb), ("sss", dw, rw)):
            want = (d * d).sum()
            assert abs(got[name][p] - want) <= r * want, (p, name, float(abs(got[name][p] - want) / want), r)
        scale = np.sqrt((da * da).sum() * (db * db).sum())
        assert abs(got["sab"][p] - (da * db).sum()) <= (ra + rb) * scale, (p, "sab")
        assert got["n_gt"][p] == int((x[a] > x[b]).sum())


def test_degenerate_samples_give_what_the_arithmetic_gives():
    nan, inf = np.nan, np.inf
    # S = 1: the means are the logarithms, every centred sum is 0, and the derived columns are 0 / 0
    s = R.summary_ref(np.array([[2.0], [3.0]]), [(0, 1)])
    assert s["mean_a"][0] == np.log(2.0) and s["mean_b"][0] == np.log(3.0) and s["mean_sum"][0] == np.log(5.0)
    assert s["saa"][0] == 0.0 and s["sbb"][0] == 0.0 and s["sab"][0] == 0.0 and s["sss"][0] == 0.0 and s["n_gt"][0] == 0
    assert all(np.isnan(s[k][0]) for k in ("cor", "sd_a", "sd_b", "sd_sum")) and s["p_gt"][0] == 0.0
    # constant traces: sums of exact zeros, cor = 0 / 0
    s = R.summary_ref(np.array([[2.0] * 5, [3.0] * 5]), [(1, 0)])
    assert s["saa"][0] == 0.0 and s["sab"][0] == 0.0 and np.isnan(s["cor"][0]) and s["sd_a"][0] == 0.0 and s["n_gt"][0] == 5 and s["p_gt"][0] == 1.0
    base = np.array([[1.0, 2.0, 3.0, 4.0], [4.0, 3.0, 1.0, 2.0], [1.5, 2.5, 0.5, 1.0]])
    pairs = [(0, 1), (2, 1), (1, 2)]
    # a zero in row 0: log 0 = -inf, mean -inf, -inf - -inf = NaN in that member's sums; the sum with the partner stays finite
    tr = base.copy(); tr[0, 2] = 0.0
    s = R.summary_ref(tr, pairs)
    assert s["mean_a"][0] == -inf and np.isnan(s["saa"][0]) and np.isnan(s["sab"][0]) and np.isnan(s["cor"][0]) and np.isnan(s["sd_a"][0])
    assert np.isfinite([s["mean_b"][0], s["sbb"][0], s["mean_sum"][0], s["sss"][0], s["sd_b"][0], s["sd_sum"][0]]).all() and s["n_gt"][0] == 1
    assert np.isfinite([s[k][q] for k in s for q in (1, 2)]).all()          # the pairs without the member are untouched
    # an inf in row 0: mean +inf, NaN in its sums, and in the sum with the partner
    tr = base.copy(); tr[0, 1] = inf
    s = R.summary_ref(tr, pairs)
    assert s["mean_a"][0] == inf and s["mean_sum"][0] == inf and np.isnan([s["saa"][0], s["sab"][0], s["sss"][0], s["cor"][0]]).all()
    assert np.isfinite([s["mean_b"][0], s["sbb"][0]]).all() and s["n_gt"][0] == 3 and np.isfinite([s[k][1] for k in s]).all()
    # a NaN: everything of the member and of the sum is NaN, and the comparison counts it as not greater on either side
    tr = base.copy(); tr[1, 0] = nan
    s = R.summary_ref(tr, pairs)
    assert np.isnan([s["mean_b"][0], s["sbb"][0], s["sab"][0], s["mean_sum"][0], s["sss"][0]]).all() and np.isfinite([s["mean_a"][0], s["saa"][0]]).all()
    assert s["n_gt"][0] == 2 and s["n_gt"][1] == 0 and s["n_gt"][2] == 3          # of samples 1 .. 3 only
    # x_a + x_b overflows where neither does: the members stay finite, the sum's columns do not
    tr = base.copy(); tr[0, 3] = 1e308; tr[1, 3] = 1e308
    s = R.summary_ref(tr, pairs)
    assert np.isfinite([s[k][0] for k in ("mean_a", "mean_b", "saa", "sbb", "sab", "cor", "sd_a", "sd_b")]).all()
    assert s["mean_sum"][0] == inf and np.isnan(s["sss"][0]) and np.isnan(s["sd_sum"][0]) and s["n_gt"][0] == 1


def _oracle_chain(orc, seed):
    rp, ci, k, l = R.stat_problem()
    p = orc.Problem(rp, ci, l, k=k)
    mu0 = orc.start_values_exact(p)
    return orc.gibbs_keyed(p, mu0, seed=seed, n_iter=16384, trace_len=1024)["trace"]


def test_columns_read_as_stated_on_the_oracles_chain(orc):
    s = R.summary_ref(_oracle_chain(orc, 4321), R.STAT_PAIRS)
    R.stat_rule(s)
    # what this chain gave when the test was written
    assert abs(s["cor"][0] - -0.066) < 5e-3 and abs(s["cor"][1] - -0.359) < 5e-3 and abs(s["sd_sum"][1] - 0.034) < 1e-3
