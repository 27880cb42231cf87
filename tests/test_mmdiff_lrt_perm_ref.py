"""The restatement of `mmdiff -lrt FILE -lrtperm B` (tests/mmdiff_lrt_perm_ref.py) against cases worked by hand and against the
definitions it is built from; no device."""
from fractions import Fraction

import numpy as np

import mmdiff_lrt_perm_ref as LP
import mmdiff_lrt_ref as L
import mmdiff_ref as R
import qvalue_ref as Q
from mmdiff_perm_ref import replica_data


def _small(F=3, groups=(2, 2), seed=5):
    rng = np.random.default_rng(seed)
    N = sum(groups)
    y = rng.normal(2.0, 1.0, (F, 1)) + rng.normal(0.0, 0.4, (F, N))
    y[:, :groups[0]] += 1.0
    e = rng.uniform(0.05, 0.5, (F, N))
    return (y, e) + R.de_design(groups)


def test_one_feature_and_five_copies_by_hand():
    """T0 = 2; the copies 1, 2, 3, NaN, 0.5: two of the four that count are not below it, so p = (1 + 2) / (1 + 4)."""
    ge, n, p = LP.counts([2.0], [[1.0], [2.0], [3.0], [np.nan], [0.5]])
    assert ge.dtype == n.dtype == np.uint64 and ge[0] == 2 and n[0] == 4
    assert Fraction(1 + int(ge[0]), 1 + int(n[0])) == Fraction(3, 5) and p[0] == 3.0 / 5.0


def test_nan_copies_leave_both_counts_and_an_observed_nan_gives_nan():
    null = np.array([[np.nan, 1.0], [np.nan, np.nan], [5.0, np.nan]])
    ge, n, p = LP.counts([4.0, np.nan], null)
    assert list(ge) == [1, 0] and list(n) == [1, 1] and p[0] == 2.0 / 2.0 and np.isnan(p[1])
    ge, n, p = LP.counts([4.0], np.full((3, 1), np.nan))       # no copy counts: (1 + 0) / (1 + 0)
    assert ge[0] == 0 and n[0] == 0 and p[0] == 1.0


def test_the_two_zeros_are_one_value():
    for t0, t in ((0.0, -0.0), (-0.0, 0.0)):
        ge, n, p = LP.counts([t0], [[t]])
        assert ge[0] == 1 and n[0] == 1 and p[0] == 1.0


def test_a_copy_whose_shuffle_is_the_identity_reproduces_the_observed_statistic():
    y, e, M, P0, P1, C = _small()
    B = 5
    hit = None
    for seed in range(1, 200):
        for b in range(1, B + 1):
            if list(R.permutation(seed ^ (b << 32), 0, 4)) == [0, 1, 2, 3]:
                hit = (seed, b)
                break
        if hit:
            break
    assert hit, "no identity shuffle among 199 seeds x 5 copies of 4 samples"
    seed, b = hit
    yb, eb = replica_data(y, e, seed, b)
    assert np.array_equal(yb[0], y[0]) and np.array_equal(eb[0], e[0]) and not np.array_equal(yb[1:], y[1:])
    r = LP.lrt_perm(y, e, M, P0, P1, C, B, seed=seed)
    assert r["null_stat"][b - 1, 0] == r["stat"][0] and r["null_status"][b - 1, 0] == r["status"][0, 0] | r["status"][1, 0] << 4
    assert r["perm_ge"][0] >= 1


def test_perm_p_lies_in_0_1_and_the_pooled_columns_are_the_definition():
    y, e, M, P0, P1, C = _small(F=6, groups=(3, 3), seed=8)
    B = 4
    r = LP.lrt_perm(y, e, M, P0, P1, C, B, seed=77)
    want = L.lrt(y, e, M, P0, P1, C)
    for k in ("loglik", "stat", "p_value", "q_value", "theta0", "theta1", "sigmasq0", "sigmasq1", "iters", "status"):
        assert np.array_equal(r[k], want[k], equal_nan=True), k
    assert r["null_stat"].shape == r["null_status"].shape == (B, 6) and r["null_status"].dtype == np.uint8
    assert np.all(r["perm_p"] > 0.0) and np.all(r["perm_p"] <= 1.0) and np.all(r["perm_n"] == B) and np.all(r["perm_ge"] <= B)
    assert np.all(r["perm_p"] >= 1.0 / (B + 1))
    ge, q = Q.qvalues_loops(r["stat"], r["null_stat"].ravel())
    assert np.array_equal(r["null_ge"], ge) and np.array_equal(r["q_perm"], q)
    assert int(r["null_ge"].sum()) >= int(r["perm_ge"].sum())       # a feature's own copies are among the pooled ones


def test_file_appends_four_columns_to_the_plain_file():
    y, e, M, P0, P1, C = _small()
    r = LP.lrt_perm(y, e, M, P0, P1, C, 2)
    feats = ["a", "b", "c"]
    plain, text = L.lrt_file(feats, r, M, P0, P1, False).split("\n"), LP.lrt_perm_file(feats, r, M, P0, P1, False).split("\n")
    assert len(plain) == len(text) == 5 and text[-1] == ""
    assert text[0] == plain[0] + "\tperm_ge\tperm_p\tnull_ge\tq_perm"
    for f in range(3):
        assert text[1 + f].startswith(plain[1 + f] + "\t")
        cols = text[1 + f][len(plain[1 + f]) + 1:].split("\t")
        assert cols == ["%d" % r["perm_ge"][f], "%g" % r["perm_p"][f], "%d" % r["null_ge"][f], "%g" % r["q_perm"][f]]


def test_memory_formula_and_the_default_slab():
    # -de 3 3 on 20 000 features: p = (1, 2), classes (1, 2): W' = 6, 8 * 20000 * 18 bytes per copy
    assert LP.perm_wslots((1, 2), (1, 2)) == 6 and LP.perm_wslots((4, 6), (2, 3)) == 9 + 21 + 6
    assert LP.slab_copies(20000, 6, (1, 2), (1, 2), 1000) == (1 << 30) // (8 * 20000 * 18) == 372
    assert LP.slab_copies(20000, 6, (1, 2), (1, 2), 100) == 100 and LP.slab_copies(20000, 6, (1, 2), (1, 2), 100, asked=7) == 7
    assert LP.slab_copies(30000000, 512, (1, 2), (1, 2), 50) == 1       # a copy above 1 GiB: one at a time
    assert LP.perm_device_bytes(10, 6, (1, 2), (1, 2), 3) == LP.lrt_device_bytes(10, 6, (1, 2), (1, 2)) + 8 * 3 * 10 * 18 + 9 * 30 + 480
