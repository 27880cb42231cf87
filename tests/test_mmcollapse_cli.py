"""CPU checks of the mmcollapse CLI (src/mmcollapse.cpp): usage and exit codes, errors on missing inputs before any device is
touched, a loud failure without a device, and the numpy restatement (tests/mmcollapse_ref.py) against closed forms."""
import gzip
import math
import os
import subprocess

import numpy as np
import pytest

import mmcollapse_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN_DIR = os.environ.get("MMSEQ_HOST_BIN_DIR") or os.path.join(ROOT, "mmseq_amd", "csrc")
MMCOLLAPSE = os.path.join(BIN_DIR, "mmcollapse")


def run(args, **kw):
    return subprocess.run([MMCOLLAPSE] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, **kw)


@pytest.mark.parametrize("args", [[], ["-x", "a"], ["-thres", "0", "a"], ["-thres", "150", "a"], ["-thres", "abc", "a"], ["-thres"]])
def test_usage_and_exit_1(args):
    r = run(args)
    assert r.returncode == 1
    assert r.stderr.startswith(b"Usage: mmcollapse [-thres FLOAT] basename1 [basename2...]")


def _mmseq_table(path, rows, ident=False, mapped=1000):
    hdr = ["feature_id", "log_mu", "sd", "mcse", "iact", "effective_length", "true_length", "unique_hits", "observed"]
    with open(path, "w") as f:
        f.write("# Mapped fragments: %d\n" % mapped)
        f.write("\t".join(hdr) + "\n")
        for name, sd, uh, obs in rows:
            f.write("\t".join([name, "-1", str(sd), "0.1", "1.5", "1000", "1180", str(uh), str(obs)]) + "\n")


def _trace(path, ids, M):
    with gzip.open(path, "wt") as f:
        f.write("".join(i + " " for i in ids) + "\n")
        for row in M:
            f.write("".join("%g " % v for v in row) + "\n")


def _sample(tmp_path, base, seed=0):
    """A sample of four unidentifiable transcripts, one identical set, two identifiable transcripts."""
    rng = np.random.default_rng(seed)
    b = str(tmp_path / base)
    _mmseq_table(b + ".mmseq", [("A", 2.0, 0, 1), ("B", 2.0, 0, 1), ("C", 2.0, 0, 1), ("D", 2.0, 0, 1), ("E", 0.5, 1, 1),
                                ("F", 0.5, 5, 1), ("I1", 1, 0, 1), ("I2", 1, 0, 1)])
    _mmseq_table(b + ".identical.mmseq", [("I1+I2", 2.0, 0, 1)])
    ids = ["A", "B", "C", "D", "E", "F", "I1", "I2"]
    _trace(b + ".trace_gibbs.gz", ids, rng.gamma(2.0, 1.0, (1024, len(ids))))
    _trace(b + ".identical.trace_gibbs.gz", ["I1+I2"], rng.gamma(2.0, 1.0, (1024, 1)))
    open(b + ".M", "w").write("#\t" + "\t".join(ids) + "\n0\t0\n0\t1\n")
    open(b + ".k", "w").write("1\n")
    return b


@pytest.mark.parametrize("missing,msg", [(".identical.mmseq", b"Error: cannot open %s.identical.mmseq"),
                                         (".mmseq", b"Error: cannot open %s.mmseq"),
                                         (".trace_gibbs.gz", b"Error: couldn't open %s.trace_gibbs.gz."),
                                         (".identical.trace_gibbs.gz", b"Error: couldn't open %s.identical.trace_gibbs.gz."),
                                         (".M", b"Error reading %s.M file.")])
def test_missing_input_fails_before_the_device(tmp_path, missing, msg):
    b1 = _sample(tmp_path, "s1", 1)
    b2 = _sample(tmp_path, "s2", 2)
    os.remove(b2 + missing)
    r = run([b1, b2], env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 1
    assert (msg % b2.encode()) in r.stderr
    assert b"no HIP device" not in r.stderr
    assert not os.path.exists(b1 + ".collapsed.mmseq")


def test_missing_column_is_named(tmp_path):
    b = _sample(tmp_path, "s1")
    txt = open(b + ".mmseq").read().replace("unique_hits", "uniq")
    open(b + ".mmseq", "w").write(txt)
    r = run([b])
    assert r.returncode == 1 and b'.mmseq file does not contain "unique_hits" column.' in r.stderr


def test_without_device_fails_loudly(tmp_path):
    from mmseq_amd import gibbs
    if gibbs.device_count() > 0:
        pytest.skip("a HIP device is present")
    b = _sample(tmp_path, "s1")
    before = {p: open(p, "rb").read() for p in sorted(tmp_path.iterdir())}
    r = run([b])
    assert r.returncode == 1 and b"no HIP device available" in r.stderr
    assert b"5 transcripts or sets of identical transcripts are unidentifiable in all samples." in r.stderr
    assert not os.path.exists(b + ".collapsed.mmseq")
    assert {p: open(p, "rb").read() for p in sorted(tmp_path.iterdir())} == before


def test_candidates_follow_the_rules(tmp_path):
    b1 = _sample(tmp_path, "s1", 1)
    cd = R.candidates([b1])
    # E (1 unique hit, sd 0.5, iact 1.5 >= 1.1: no SD bar), F (5 unique hits) leave; I1, I2 are members of a set; the set stays
    assert cd["candidates"] == ["A", "B", "C", "D", "I1+I2"]
    assert cd["observed"].all()


# ------------------------------------------------------------------------------------------ the restatement vs closed forms
def _four_traces(N=1024, seed=5):
    """columns: u, -u + small noise, an independent w, and u + w"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=N)
    w = rng.normal(size=N)
    e = rng.normal(size=N) * 0.1
    return np.stack([u, -u + e, w, u + w], axis=1)


def test_restatement_correlations_closed_form():
    X = _four_traces()
    Xc = X - X.mean(axis=0)
    want = np.corrcoef(X, rowvar=False)
    V = R.mean_corr(R.centre([X, X]), np.ones((4, 2), bool))
    np.testing.assert_allclose(V, want, rtol=1e-12, atol=1e-14)
    # a masked sample drops out of the mean; a pair observed nowhere is NaN
    Y = _four_traces(seed=9)
    obs = np.array([[1, 1], [1, 0], [1, 1], [0, 0]], bool)
    V2 = R.mean_corr(R.centre([X, Y]), obs)
    wy = np.corrcoef(Y, rowvar=False)
    assert V2[0, 1] == pytest.approx(want[0, 1], rel=1e-12)
    assert V2[0, 2] == pytest.approx((want[0, 2] + wy[0, 2]) / 2, rel=1e-12)
    assert np.isnan(V2[3, 0]) and np.isnan(V2[3, 3])
    assert Xc.shape == (1024, 4)


def test_restatement_one_planted_merge_and_the_threshold_index():
    X = _four_traces()
    g = R.Greedy([X], np.ones((4, 1), bool), ["u", "neg", "w", "uw"])
    rmax = R.row_max(g.V)
    c = np.corrcoef(X, rowvar=False)
    np.fill_diagonal(c, -np.inf)
    np.testing.assert_allclose(rmax, c.max(axis=1), rtol=1e-12)
    assert R.threshold_index(4, 0.975) == 3 and R.threshold_index(4, 1.0) == 3 and R.threshold_index(4, 0.5) == 2
    thr = -0.9                               # only (u, -u) lies below
    merges = g.run(thr, tie_tol=1e-9)
    assert [(a, b) for a, b, _ in merges] == [(0, 1)]
    assert merges[0][2] == pytest.approx(np.corrcoef(X[:, 0], X[:, 1])[0, 1], rel=1e-12)
    assert g.names == ["neg*u", "NA", "w", "uw"]
    # the merged row is the correlation of the summed trace
    s = X[:, 0] + X[:, 1]
    assert g.V[0, 2] == pytest.approx(np.corrcoef(s, X[:, 2])[0, 1], rel=1e-10)
    assert g.V[2, 0] == g.V[0, 2] and np.isnan(g.V[1]).all() and np.isnan(g.V[:, 1]).all()
    assert math.isclose(g.V[0, 0], 1.0, rel_tol=1e-12)
