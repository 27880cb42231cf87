"""tests/assign_ref.py -- the restated specification of the posterior assignment probabilities -- against facts that do not depend on
it: exact values, the sum of a row's probabilities, an extended-precision evaluation, the degenerate branch, conservation of reads."""
import math

import numpy as np
import pytest

import assign_ref as R

EPS = 2.0 ** -52
LENGTHS = (1, 2, 3, 8, 9, 64, 65, 300)
SAMPLES = (1, 63, 64, 65, 1024)


def _trace(rng, n_tx, S):
    """positive values over many orders of magnitude, as mu is"""
    return np.exp(rng.normal(0.0, 3.0, (n_tx, S)))


def test_row_of_one_hit_is_exactly_one():
    rng = np.random.default_rng(1)
    for S in SAMPLES:
        tr = _trace(rng, 5, S)
        P = R.assign_ref([0, 1, 2], [3, 0], tr)
        assert P.tolist() == [1.0, 1.0]
    # values whose product with their rounded reciprocal is not 1, a zero, an infinity, a subnormal: one sample each
    for v in (49.0, 5e-324, 0.0, np.inf, 1e308):
        assert 49.0 * (1.0 / 49.0) != 1.0
        assert R.assign_ref([0, 1], [0], np.array([[v]]))[0] == 1.0
    many = np.exp(rng.normal(0.0, 3.0, (1, 2000)))
    assert all(R.assign_ref([0, 1], [0], many, first=s, count=1)[0] == 1.0 for s in range(2000))


def test_identical_trace_rows_share_equally():
    """Every p is v * (1 / (L v summed one by one)): three roundings (the sum's last, the reciprocal, the product) besides the
    representation of 1 / L, then S additions and one division."""
    rng = np.random.default_rng(2)
    for L in LENGTHS:
        for S in (1, 65, 1024):
            row = np.exp(rng.normal(0.0, 3.0, S))
            tr = np.tile(row, (L, 1))
            P = R.assign_ref([0, L], np.arange(L), tr)
            assert np.all(P == P[0])
            assert abs(P[0] * L - 1.0) <= (L + S / 64 + 8) * EPS


@pytest.mark.parametrize("S", SAMPLES)
def test_random_rows_sum_to_one(S):
    rng = np.random.default_rng(100 + S)
    for L in LENGTHS:
        tr = _trace(rng, L + 3, S)
        cols = rng.permutation(L + 3)[:L]
        P = R.assign_ref([0, L], cols, tr)
        assert np.all(P > 0) and np.all(P <= 1.0)
        assert abs(math.fsum(P) - 1.0) <= (L + S / 64 + 8) * EPS, (L, S, math.fsum(P) - 1.0)


@pytest.mark.parametrize("S", SAMPLES)
def test_against_extended_precision(S):
    rng = np.random.default_rng(200 + S)
    for L in LENGTHS:
        tr = _trace(rng, L, S)
        cols = rng.permutation(L)
        P = R.assign_ref([0, L], cols, tr)
        v = tr[cols].astype(np.longdouble)
        want = (v / v.sum(axis=0)).sum(axis=1) / np.longdouble(S)
        rel = np.abs(P.astype(np.longdouble) - want) / want
        assert float(rel.max()) <= 1e-13, (L, S, float(rel.max()))


def test_sample_sub_range():
    rng = np.random.default_rng(3)
    tr = _trace(rng, 6, 100)
    rp, ci = [0, 3, 3, 5], [4, 1, 0, 2, 5]
    assert np.array_equal(R.assign_ref(rp, ci, tr, first=3, count=70), R.assign_ref(rp, ci, tr[:, 3:73]))


def test_degenerate_samples():
    # sample 0: every mu of the row is 0; sample 1: the sum is inf; sample 2: ordinary
    tr = np.array([[0.0, 1e308, 1.0],
                   [0.0, 1e308, 3.0],
                   [7.0, 2.0, 4.0]])
    P = R.assign_ref([0, 2, 3], [0, 1, 2], tr)
    assert P[0] == ((0.5 + 0.5) + 1.0 * (1.0 / 4.0)) / 3.0
    assert P[1] == ((0.5 + 0.5) + 3.0 * (1.0 / 4.0)) / 3.0
    assert P[2] == 1.0
    # all samples degenerate: exactly 1 / L whatever S
    for S in (1, 64, 130):
        P = R.assign_ref([0, 3], [0, 1, 2], np.zeros((3, S)))
        assert abs(P[0] - 1.0 / 3.0) <= (S / 64 + 8) * EPS and np.all(P == P[0])


def test_expected_hits_conserve_the_reads():
    rng = np.random.default_rng(4)
    n_tx, S = 40, 130
    L = rng.integers(0, 7, 300)
    rp = np.concatenate([[0], np.cumsum(L)])
    ci = np.concatenate([rng.permutation(n_tx)[:l] for l in L]).astype(np.uint32)
    k = rng.integers(1, 50, L.size)
    tr = _trace(rng, n_tx, S)
    P = R.assign_ref(rp, ci, tr)
    E = R.expected_hits(rp, ci, P, n_tx, k)
    total = int(k[L > 0].sum())
    H = int(rp[-1])
    assert abs(math.fsum(E) - total) <= H * EPS * total
    assert np.array_equal(R.expected_hits(rp, ci, P, n_tx), R.expected_hits(rp, ci, P, n_tx, np.ones(L.size)))


def test_single_sample_helper_is_the_one_sample_case():
    rng = np.random.default_rng(5)
    tr = _trace(rng, 9, 4)
    rp, ci = [0, 2, 2, 6], [8, 3, 0, 1, 2, 5]
    for s in range(4):
        assert np.array_equal(R.sample_probabilities(rp, ci, tr[:, s]), R.assign_ref(rp, ci, tr, first=s, count=1))


def test_it_estimates_what_the_oracle_chain_draws(orc):
    """The rule of tests/test_gpu_assign.py::test_it_estimates_what_the_sampler_draws on the oracle's keyed chain, for the same
    problem and seed: the counts of iteration s + 1 are redrawn from sample s with the oracle's sample step."""
    rp, ci, k, l, n_tx = R.stat_problem()
    srp, sci, sk, _ = orc.canonical_layout(rp, ci, k)
    p = orc.Problem(srp, sci, l, k=sk)
    mu0 = orc.start_values_exact(p)
    ref = orc.gibbs_keyed(p, mu0, seed=4321, n_iter=1024, trace_len=1024)
    tr = ref["trace"]
    counts = [orc.sample_counts(p, mu0 if s == 0 else tr[:, s - 1], 4321, 0, s) for s in range(1024)]
    assert np.array_equal(counts[-1], ref["cnt"])            # the replay is the chain's own last draw
    worst, n_exact, _ = R.stat_rule(rp, ci, k, tr, counts)
    assert n_exact >= 12 and worst <= 5.0
