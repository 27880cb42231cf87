"""The statistics mmdiff -lrt derives on the host (mmseq_amd/csrc/host/lrt_stats.hpp), through its stand-alone driver
lrt_stats_test: the chi-squared upper tail against scipy, the Benjamini-Hochberg q-values against a plain loop, and the numpy
restatement (tests/mmdiff_lrt_ref.py) against the driver, bit for bit."""
import os
import subprocess

import numpy as np
import pytest
from scipy import stats

import mmdiff_lrt_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN_DIR = os.environ.get("MMSEQ_HOST_BIN_DIR") or os.path.join(ROOT, "mmseq_amd", "csrc")
DRIVER = os.path.join(BIN_DIR, "lrt_stats_test")


def drive(mode, lines, tmp_path):
    path = tmp_path / ("in_%s.txt" % mode)
    path.write_text("".join(lines))
    r = subprocess.run([DRIVER, mode, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert r.returncode == 0, r.stderr
    return np.array([float(t) for t in r.stdout.split()])


# stat from 0 to 1400: the ends, both sides of the branch point x = a + 1 for every df, and a geometric and a linear grid between
def stat_grid(df):
    a = 0.5 * df
    near = [2.0 * (a + 1.0) * (1.0 + s) for s in (-1e-3, -1e-9, 0.0, 1e-9, 1e-3)]
    return np.unique(np.concatenate([[0.0, 1e-300, 1e-12, 1400.0], near, np.geomspace(1e-6, 1400.0, 60), np.linspace(0.0, 1400.0, 57)]))


@pytest.fixture(scope="module")
def p_values(tmp_path_factory):
    cases = [(df, s) for df in range(1, 41) for s in stat_grid(df)]
    got = drive("p", ["%d %.17g\n" % c for c in cases], tmp_path_factory.mktemp("lrt_p"))
    assert len(got) == len(cases)
    return cases, got


def test_p_value_equals_scipy_chi2_sf(p_values):
    """Relative 1e-10: both branches converge to rounding, and the prefactor exp(-x + a log x - lgamma(a)) carries a few ulps of a
    number up to about 700, about 1e-13."""
    cases, got = p_values
    df = np.array([c[0] for c in cases], float)
    st = np.array([c[1] for c in cases])
    want = stats.chi2.sf(st, df)
    assert np.all(want > 0.0) and want.min() < 1e-290 and want.max() == 1.0
    rel = np.abs(got - want) / want
    worst = int(np.argmax(rel))
    print("largest relative difference %.3g at df %d stat %r" % (rel[worst], cases[worst][0], cases[worst][1]))
    assert rel[worst] <= 1e-10


def test_p_value_edges(tmp_path):
    got = drive("p", ["0 1.0\n", "-3 1.0\n", "2 nan\n", "2 -5.0\n", "2 0.0\n", "2 inf\n", "1 -0.0\n"], tmp_path)
    assert np.isnan(got[:3]).all()                  # df <= 0, a NaN stat
    assert np.array_equal(got[3:], [1.0, 1.0, 0.0, 1.0])    # max(stat, 0); the ends


def test_restatement_of_p_equals_the_driver(p_values):
    cases, got = p_values
    pick = range(0, len(cases), 7)
    assert np.array_equal([L.chi2_sf(cases[i][0], float(cases[i][1])) for i in pick], got[list(pick)])


def plain_bh(p):
    """Benjamini-Hochberg by definition: q_i = min over the p_j >= p_i (in sorted order, ties by input order) of p_j m / rank_j."""
    p = np.asarray(p, float)
    live = [i for i in range(len(p)) if not np.isnan(p[i])]
    order = sorted(live, key=lambda i: (p[i], i))
    m = len(order)
    q = np.full(len(p), np.nan)
    for r, i in enumerate(order):
        q[i] = min([1.0] + [p[order[s]] * float(m) / float(s + 1) for s in range(r, m)])
    return q


BH_CASES = {
    "distinct": [0.01, 0.5, 0.03, 0.9, 0.002, 0.2],
    "ties": [0.04, 0.04, 0.01, 0.04, 0.5, 0.5, 0.01, 1.0],
    "nan": [0.2, float("nan"), 0.001, float("nan"), 0.03, 0.03],
    "all_nan": [float("nan")] * 3,
    "one": [0.25],
    "ones_and_zeros": [1.0, 0.0, 1.0, 0.0, 0.5],
    "random": list(np.random.default_rng(77).uniform(0, 1, 300) ** 3),
}


@pytest.mark.parametrize("name", sorted(BH_CASES))
def test_q_value_equals_plain_loop(tmp_path, name):
    p = np.array(BH_CASES[name])
    got = drive("q", ["%.17g\n" % v for v in p], tmp_path)
    want = plain_bh(p)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(L.bh_qvalues(p), got, equal_nan=True)
    live = ~np.isnan(p)
    assert np.all(got[live] >= p[live]) and np.all(got[live] <= 1.0)
