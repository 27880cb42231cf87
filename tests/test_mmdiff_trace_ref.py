"""The trace restatement (tests/mmdiff_trace_ref.py) on a closed case: 3 features, 4 samples in two groups with one covariate, a
burn-in of 112 iterations recorded every 7th, two tuning batches, 40 sampling iterations recorded every 5th.  So 16 burn-in rows
(iterations 0, 7, ..., 105), 8 sampling rows (0, 5, ..., 35) and one tuning row (before batch 1)."""
import numpy as np
import pytest

import mmdiff_ref as R
import mmdiff_trace_ref as TR


@pytest.fixture(scope="module")
def run():
    rng = np.random.default_rng(12)
    y = rng.normal(2, 1, (3, 1)) + rng.normal(0, 0.3, (3, 4))
    e = rng.uniform(0.05, 0.5, (3, 4))
    M = np.array([[0.3], [1.1], [-0.4], [0.9]])
    C = np.array([[0, 0], [0, 0], [0, 1], [0, 1]])
    P0 = np.ones((4, 1))
    P1 = np.where(C[:, 1:] == 0, 0.5, -0.5)
    b, pseudo = TR.run_traced(y, e, M, P0, P1, C, 112, 40, batches=2, every_burnin=7, every_sample=5, seed=5)
    return b, pseudo


def test_names_follow_initialise_streams(run):
    b, _ = run
    assert b.names() == ["alpha0", "alpha1", "beta0_0", "beta1_0", "eta0_0", "eta1_0", "lambda0_0", "lambda1_0", "sigmasq0_0", "sigmasq1_0",
                         "sigmasq1_1", "rho0", "rho1", "gamma"]
    assert TR.param_names(2, [1, 3], [1, 3])[2:10] == ["beta0_0", "beta0_1", "beta1_0", "beta1_1", "eta0_0", "eta1_0", "eta1_1", "eta1_2"]


def test_row_counts_and_empty_files(run):
    b, pseudo = run
    assert b.stacked(0).shape == (16, 13, 3) and b.stacked(1).shape == (8, 14, 3) and len(b.tune_rows) == 1
    files = TR.files_of(b, pseudo)
    names = b.names()
    assert set(files) == {n + "-burnin" for n in names} | set(names) | {"logitp-burnin", "meanLO-burnin", "logitp", "meanLO", "pseudo"}
    assert files["gamma-burnin"] == "" and files["logitp-burnin"] == ""
    assert files["meanLO-burnin"] == "\n" * 16
    for n in names[:-1]:
        lines = files[n + "-burnin"].split("\n")
        assert len(lines) == 17 and lines[-1] == "" and all(len(l.split(" ")) == 4 and l.endswith(" ") for l in lines[:-1]), n
        assert files[n].count("\n") == 8
    assert set(files["gamma"].replace("\n", " ").split()) <= {"0", "1"} and files["gamma"].count("\n") == 8
    assert files["logitp"].count("\n") == 1 and files["logitp"] == TR.line(b.tune_rows[0][1])
    lo = files["meanLO"].split("\n")
    assert len(lo) == 10 and len(lo[0].split()) == 3 and lo[1:] == [""] * 9          # one tuning line, then an empty line per row
    # P0 is a constant column: nil, so eta0_0 and lambda0_0 keep their starting values in every line
    lam0 = R.fmt(2.0 / (1.4 - 1.0))          # s / (d - 1)
    assert files["eta0_0-burnin"] == "0 0 0 \n" * 16 and files["lambda0_0"] == ((lam0 + " ") * 3 + "\n") * 8
    # the first burn-in row is the state after iteration 0, the tuning row the state before batch 1
    first = b.stacked(0)[0]
    assert files["alpha0-burnin"].split("\n")[0] == TR.line(first[0])[:-1]


def test_pseudo_header_and_rows(run):
    b, pseudo = run
    want = ("A0\tValpha0\tB0_0\tVbeta0_0\tF0_0\tVeta0_0\tS0_0\tJ0_0\tL0_0\tQ0\tR0\t"
            "A1\tValpha1\tB1_0\tVbeta1_0\tF1_0\tVeta1_0\tS1_0\tJ1_0\tL1_0\tJ1_1\tL1_1\tQ1\tR1\t\n")
    assert TR.pseudo_header(1, [1, 1], [1, 2]) == want
    text = TR.files_of(b, pseudo)["pseudo"]
    rows = text.split("\n")
    assert rows[0] + "\n" == want and len(rows) == 5 and rows[-1] == ""
    assert pseudo.shape == (24, 3) and all(len(r.split("\t")) == 25 and r.endswith("\t") for r in rows[1:4])
    # model 0's P is nil: F0_0 = 0, Veta0_0 = 1 and S0_0 = 1 / (1 / s) = s stay at the constructor's values
    assert rows[1].split("\t")[4:7] == ["0", "1", "2"]
