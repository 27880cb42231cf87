"""CPU checks of tests/fold_ref.py, the restatement the device tests of mmg_fold_* compare with: closed forms, the symmetry of the
two sides, the key-space bisection the kernel uses against the brute-force sort, the CLI's rules, and that the package's own host-side
helpers (mmseq_amd.fold) state the same rules."""
import numpy as np
import pytest

import fold_ref as R


def _draws(rng, F, S, sig=6):
    x = np.exp(rng.normal(-3.0, 2.0, F)[:, None] + rng.uniform(0.01, 1.5, F)[:, None] * rng.normal(0.0, 1.0, (F, S)))
    return np.array([[float("%.*g" % (sig, v)) for v in row] for row in x])


def test_equal_sides_split_the_pairs_in_half_and_have_median_zero():
    rng = np.random.default_rng(1)
    for S in (1, 2, 7, 64, 100):
        a = _draws(rng, 3, S, sig=2)
        n = S * S
        r = R.summary_ref(a, a, 0.0, [(n - 1) // 2, n // 2])
        assert (2 * r["n_gt"].astype(np.int64) + r["n_eq"] == n).all()       # n_gt + n_eq / 2 is exactly half the pairs
        assert (r["n_eq"] >= S).all() and (r["p_gt"] == 0.5).all()
        assert (r["quantiles"] == 0.0).all() and (r["lfc"] == 0.0).all()
        assert (r["status"] == 0).all()


def test_a_power_of_two_shift_of_a_moves_every_order_statistic():
    rng = np.random.default_rng(2)
    Sa, Sb = 33, 20
    # logs on a grid of 2^-10: every difference and every shifted difference is exact
    x = np.round(rng.normal(0.0, 2.0, (2, Sa)) * 1024) / 1024
    y = np.round(rng.normal(0.0, 2.0, (2, Sb)) * 1024) / 1024
    ident = lambda v: np.asarray(v, np.float64)                                # the draws are the logs themselves
    ranks = [0, 1, 17, Sa * Sb // 2, Sa * Sb - 1]
    base = R.fold_ref(x + 100.0, y + 100.0, 0.0, ranks, log=ident)             # (+ 100: valid draws are > 0)
    for t in (0.25, 4.0, -8.0):
        got = R.fold_ref(x + 100.0 + t, y + 100.0, 0.0, ranks, log=ident)
        assert np.array_equal(got["quantiles"], base["quantiles"] + t)
        assert np.array_equal(got["n_eq"], base["n_eq"] * 0 + ((x + t)[:, :, None] == y[:, None, :]).sum(axis=(1, 2)))
        off = R.fold_ref(x + 100.0, y + 100.0, -t, ranks, log=ident)           # the offset goes to B: the same shift of d
        assert np.array_equal(off["quantiles"], got["quantiles"]) and np.array_equal(off["n_gt"], got["n_gt"])


def test_swapping_the_sides_negates_and_mirrors():
    rng = np.random.default_rng(3)
    Sa, Sb = 40, 9
    a, b = _draws(rng, 4, Sa, sig=2), _draws(rng, 4, Sb, sig=2)
    n = Sa * Sb
    ranks = [0, 5, 100, n - 1]
    ab = R.summary_ref(a, b, 0.0, ranks)
    ba = R.summary_ref(b, a, 0.0, [n - 1 - k for k in ranks])
    assert np.array_equal(ba["lfc"], -ab["lfc"]) and np.array_equal(ba["sd"], ab["sd"])
    assert np.array_equal(ba["quantiles"], -ab["quantiles"])
    assert np.array_equal(ba["n_gt"], n - ab["n_gt"].astype(np.int64) - ab["n_eq"]) and np.array_equal(ba["n_eq"], ab["n_eq"])
    assert (ab["n_eq"] > 0).any()                                               # two significant digits: ties are there


def test_invalid_draws_set_their_bits_and_nothing_else():
    rng = np.random.default_rng(4)
    a, b = _draws(rng, 7, 5), _draws(rng, 7, 3)
    a[1, 2] = 0.0; b[2, 0] = -1.0; a[3, 4] = np.nan; b[3, 1] = np.inf; a[5, 0] = np.inf
    r = R.summary_ref(a, b, 0.5, [0, 14, 15])
    assert list(r["status"]) == [0, 1, 2, 3, 0, 1, 0]
    bad = r["status"] != 0
    for k in ("mean_a", "mean_b", "ss_a", "ss_b", "lfc", "sd", "p_gt"):
        assert np.isnan(r[k][bad]).all() and np.isfinite(r[k][~bad]).all(), k
    assert np.isnan(r["quantiles"][bad]).all() and (r["n_gt"][bad] == 0).all() and (r["n_eq"][bad] == 0).all()
    assert np.isfinite(r["quantiles"][~bad][:, :2]).all() and np.isnan(r["quantiles"][:, 2]).all()   # rank 15 = Sa Sb: NaN alone
    clean = R.summary_ref(a[[0, 4, 6]], b[[0, 4, 6]], 0.5, [0, 14, 15])
    for k in R.DEVICE_COLUMNS:
        assert np.array_equal(r[k][~bad], clean[k], equal_nan=True), k


def test_key_map_is_monotone_and_inverts():
    v = [-np.inf, -1e300, -1.0, -5e-324, 0.0, 5e-324, 1.0, 1e300, np.inf]
    k = [R.key_of(x) for x in v]
    assert k == sorted(k) and len(set(k)) == len(k)
    assert [R.unkey(x) for x in k] == v
    assert R.key_of(-0.0) + 1 == R.key_of(0.0)


@pytest.mark.parametrize("seed", range(6))
def test_key_space_bisection_equals_the_sort(seed):
    """60 cases a seed: sizes 1 .. 12 a side, continuous draws, heavy ties (two or three distinct values), constant sides, wide
    magnitudes, offsets that tie the sides exactly; every rank of the small cases, the edges and a few of the others"""
    rng = np.random.default_rng(100 + seed)
    ident = lambda v: np.asarray(v, np.float64)
    for case in range(60):
        Sa, Sb = int(rng.integers(1, 13)), int(rng.integers(1, 13))
        kind = case % 5
        if kind == 0:
            x, y = rng.normal(0, 1, Sa), rng.normal(0, 1, Sb)
        elif kind == 1:
            x, y = rng.integers(0, 3, Sa).astype(float), rng.integers(0, 2, Sb).astype(float)
        elif kind == 2:
            x, y = np.full(Sa, 1.5), (np.full(Sb, 1.5) if case % 2 else rng.integers(0, 3, Sb) * 0.75)
        elif kind == 3:
            x, y = rng.choice([-1.0, 1.0], Sa) * 10.0 ** rng.uniform(-300, 300, Sa), rng.choice([-1.0, 1.0], Sb) * 10.0 ** rng.uniform(-300, 300, Sb)
        else:
            x = rng.integers(-4, 5, Sa) / 8.0
            y = x[rng.integers(0, Sa, Sb)] - 0.125                              # with off = 0.125 the sides tie exactly
            y = y + 0.125
        n = Sa * Sb
        want = np.sort(np.subtract.outer(x + 0.0, y + 0.0), axis=None)
        ks = range(n) if n <= 30 else sorted({0, 1, n // 2, n - 2, n - 1, *map(int, rng.integers(0, n, 4))})
        for k in ks:
            assert R.bisect_rank(x, y, k) == want[k], (seed, case, k)
        assert np.isnan(R.bisect_rank(x, y, n))
        ref = R.fold_ref((x + 400.0)[None, :], (y + 400.0)[None, :], 0.0, [0, n - 1], log=ident) if kind != 3 else None
        if ref is not None:
            assert ref["quantiles"][0, 0] == (x.min() + 400.0) - (y.max() + 400.0) and ref["quantiles"][0, 1] == (x.max() + 400.0) - (y.min() + 400.0)


def test_cli_rules():
    off, n = R.offset_rule([1.0, 2.0, 5.0, np.nan, 3.0], [0.5, 0.0, 1.0, 1.0, -np.inf], [1, 2, 0, 3, 3], [1, 1, 4, 1, 1])
    assert (off, n) == (1.25, 2)                                                # features 0 and 1: (0.5 + 2.0) / 2
    off, n = R.offset_rule([1.0, 2.0, 5.0], [0.5, 0.0, 1.0], [1, 2, 0], [1, 1, 4], uhmin=0)
    assert (off, n) == (2.0, 3)
    assert R.offset_rule([1.0], [2.0], [0], [5]) == (None, 0)
    n = 1024 * 1024
    assert R.cli_ranks([0, 2.5, 50, 97.5, 100], 0.01, n) == [0, 26214, 524288, 1022361, n - 1, 10486, 1038089]
    assert R.percentile_rank(50, 2) == 1 and R.percentile_rank(50, 4) == 2 and R.percentile_rank(49.9, 2) == 0   # halves go up
    assert R.gfold_of(0.5, 2.0) == 0.5 and R.gfold_of(-2.0, -0.5) == -0.5 and R.gfold_of(-1.0, 1.0) == 0.0 and R.gfold_of(0.0, 0.0) == 0.0
    assert np.isnan(R.gfold_of(np.nan, 1.0))


def test_the_package_states_the_same_host_side_rules():
    from mmseq_amd import fold as P
    rng = np.random.default_rng(9)
    for p in list(rng.uniform(0, 100, 200)) + [0, 100, 50, 2.5, 97.5, 1, 99]:
        for n in (1, 2, 6, 1024 * 100, 1024 * 1024, 4096 * 4096):
            assert P.percentile_rank(p, n) == R.percentile_rank(p, n)
    a, b = _draws(rng, 5, 6), _draws(rng, 5, 4)
    a[2, 0] = 0.0
    dev = R.fold_ref(a, b, 0.1, [0, 23])
    got, want = P.derived(dev, 6, 4), R.derived(dev, 6, 4)
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    g = P.gfold_of(dev["quantiles"][:, 0], dev["quantiles"][:, 1])
    assert np.array_equal(g, [R.gfold_of(lo, hi) for lo, hi in dev["quantiles"]], equal_nan=True)
    assert P.DEVICE_COLUMNS == R.DEVICE_COLUMNS
