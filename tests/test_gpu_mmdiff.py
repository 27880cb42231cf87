"""mmdiff on the device against the numpy restatement (tests/mmdiff_ref.py): the CLI's whole stdout byte for byte on synthetic
.mmseq tables, reruns, tuning with frozen features, MAXBATCHES, a planted effect, and a 200 000-feature run."""
import os
import subprocess

import numpy as np
import pytest

import mmdiff_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MMDIFF = os.path.join(ROOT, "mmseq_amd", "csrc", "mmdiff")
COLS = ("feature_id", "log_mu", "sd", "mcse", "iact", "effective_length", "true_length", "unique_hits")


def write_tables(tmp_path, y, e, uh, prefix="s"):
    F, S = y.shape
    files = []
    for s in range(S):
        path = str(tmp_path / ("%s%d.mmseq" % (prefix, s)))
        with open(path, "w") as f:
            f.write("# Mapped fragments: 1000\n" + "\t".join(COLS) + "\n")
            for i in range(F):
                f.write("f%d\t%r\t%r\t0.01\t1.5\t1000\t1200\t%d\n" % (i, float(y[i, s]), float(e[i, s]), int(uh[i, s])))
        files.append(path)
    return files


def synth(F, S, seed=0, effect=1.5, planted=0.2, groups=None):
    rng = np.random.default_rng(seed)
    y = rng.normal(2, 1, (F, 1)) + rng.normal(0, 0.3, (F, S))
    n = int(F * planted)
    first = groups[0] if groups else S // 2
    y[:n, :first] += effect
    e = rng.uniform(0.05, 0.5, (F, S))
    uh = rng.integers(1, 5, (F, S))
    return y, e, uh, n


def cli(args, timeout=300):
    r = subprocess.run([MMDIFF] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout.decode(), r.stderr.decode()


FAST = ["-burnin", "1024", "-iter", "1024", "-notune"]
CASE_SEED = {"de33": 101, "de222": 102, "covariate": 103, "fixalpha": 104, "permute": 105}


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["de33", "de222", "covariate", "fixalpha", "permute"])
def test_cli_table_is_byte_identical_to_the_restatement(gpu, tmp_path, case):
    """With -notune (the restatement costs ~10 ms per iteration, and these 120-feature fixtures tune for up to a few hundred
    batches); test_cli_default_tuning_is_byte_identical runs the CLI's own tuning loop."""
    S = 6
    groups = [2, 2, 2] if case == "de222" else [3, 3]
    y, e, uh, _ = synth(120, S, seed=CASE_SEED[case], groups=groups)
    files = write_tables(tmp_path, y, e, uh)
    design = None
    args = list(FAST)
    kw = {}
    if case == "covariate":
        M = np.array([[0.3], [1.1], [-0.4], [0.9], [0.0], [-1.2]])
        C = np.array([[0, 0], [0, 0], [0, 0], [0, 1], [0, 1], [0, 1]])
        P0 = np.ones((S, 1))
        P1 = np.where(C[:, 1:] == 0, 0.5, -0.5)
        mat = tmp_path / "design.txt"
        mat.write_text("# covariate\n" + "".join("%r\n" % float(v) for v in M[:, 0]) + "\n" + "".join("%d %d\n" % tuple(c) for c in C)
                       + "\n1\n\n0.5\n-0.5\n")
        design = (M, P0, P1, C)
        args += ["-m", str(mat)]
    else:
        if case == "fixalpha":
            args = ["-fixalpha"] + args
            kw["fixalpha"] = True
        if case == "permute":
            args = ["-permute", "-seed", "77"] + args
            kw.update(permute=True, seed=77)
        args += ["-de"] + [str(g) for g in groups]
    out, err = cli(args + files)
    want = R.mmdiff(files, groups=None if design else groups, design=design, burnin=1024, iters=1024, tune=False, **kw)
    assert out == want
    if case == "covariate":
        assert "beta0_0\t" in out.split("\n")[1] and "eta1_0" in out.split("\n")[1]


@pytest.mark.gpu
def test_cli_default_tuning_is_byte_identical(gpu, tmp_path):
    """The CLI's default tuning loop (batches of 128 until every feature is tuned) on a fixture that tunes in 7 batches; fewer
    than 100 features, so the normalisation is skipped, as in the reference."""
    y, e, uh, _ = synth(6, 6, seed=200)
    files = write_tables(tmp_path, y, e, uh)
    out, err = cli(["-burnin", "1024", "-iter", "1024", "-de", "3", "3"] + files)
    assert "Warning: fewer than 100 features found for normalisation. Skipping." in err
    assert "sampling after 7 tuning batches" in err
    want = R.mmdiff(files, groups=[3, 3], burnin=1024, iters=1024, tune=True)
    assert out == want


@pytest.mark.gpu
def test_end_to_end_mmseq_mmcollapse_mmdiff(gpu, tmp_path):
    """mmseq on three small samples, mmcollapse across them, mmdiff on the collapsed tables: the table equals the restatement's
    on the same collapsed tables."""
    from oracle import host_oracle as H
    from test_gpu_mmcollapse import _families
    bases = []
    for s in range(3):
        p = tmp_path / ("s%d.hits" % s)
        p.write_bytes(H.write_hits_text(_families(100 + s)))
        base = str(tmp_path / ("s%d" % s))
        r = subprocess.run([os.path.join(ROOT, "mmseq_amd", "csrc", "mmseq"), str(p), base], stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        bases.append(base)
    r = subprocess.run([os.path.join(ROOT, "mmseq_amd", "csrc", "mmcollapse")] + bases, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    files = [b + ".collapsed.mmseq" for b in bases]
    out, err = cli(FAST + ["-de", "1", "2"] + files)
    rows = out.rstrip("\n").split("\n")
    assert rows[1].startswith("feature_id\tbayes_factor\tposterior_probability\talpha0\talpha1\teta1_0\tmu_s0.collapsed\t")
    assert any("*" in row.split("\t")[0] for row in rows[2:])      # collapsed sets reach mmdiff
    assert out == R.mmdiff(files, groups=[1, 2], burnin=1024, iters=1024, tune=False)


@pytest.mark.gpu
def test_reruns_are_bit_identical(gpu, tmp_path):
    y, e, uh, _ = synth(300, 6, seed=5)
    files = write_tables(tmp_path, y, e, uh)
    a, _ = cli(FAST + ["-de", "3", "3"] + files)
    b, _ = cli(FAST + ["-de", "3", "3"] + files)
    assert a == b
    c, _ = cli(["-seed", "99"] + FAST + ["-de", "3", "3"] + files)
    assert c != a


@pytest.mark.gpu
def test_tuning_batches_with_frozen_features_match_the_restatement(gpu):
    from mmseq_amd.diff import Diff
    y, e, _, _ = synth(60, 6, seed=11)
    M, P0, P1, C = R.de_design([3, 3])
    d = Diff(y, e, M, P0, P1, C, seed=42)
    d.burnin(1024)
    counts = [d.tune_batch() for _ in range(4)]
    d.sample(1024)
    got = d.results()
    b = R.BMS(y, e, M, P0, P1, C, seed=42)
    b.burnin(1024)
    want_counts = [b.tune_batch() for _ in range(4)]
    b.sample(1024)
    want = b.results()
    assert counts == want_counts
    assert counts[0] == 60 and 0 < counts[-1] < 60, counts      # some features froze after the second batch, some did not
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert d.info()["batches"] == 4


@pytest.mark.gpu
def test_untuned_features_stop_at_the_batch_limit(gpu):
    """Two features with a huge difference between two groups of 50 samples: the log odds (about N/2 times the log of the ratio of
    the models' variances, several hundred) stay beyond what tuning can move logit p' (about 2 sqrt(b) after b batches), so the
    host loop (mmseq_amd.diff.Diff.tune) stops at its batch limit with features still untuned.  The limit here is 512, for run time;
    the CLI's MAXBATCHES = 8192 stop is the same rule with a larger constant and is not exercised by this test."""
    from mmseq_amd.diff import Diff
    limit = 512
    rng = np.random.default_rng(8)
    y = np.concatenate([np.zeros((2, 50)), np.full((2, 50), 40.0)], 1) + rng.normal(0, 0.05, (2, 100))
    e = np.full_like(y, 0.01)
    M, P0, P1, C = R.de_design([50, 50])
    d = Diff(y, e, M, P0, P1, C, seed=3)
    d.burnin(1024)
    nb = d.tune(limit)
    assert nb == limit and d.info()["batches"] == limit
    assert d.tune_batch() == 2   # still untuned after the limit
    d.sample(1024)
    r = d.results()
    assert np.all(r["gamma_mean"] == 1.0)


@pytest.mark.gpu
def test_planted_effects_are_found(gpu, tmp_path):
    y, e, uh, n = synth(200, 6, seed=21, effect=3.0, planted=0.15)
    files = write_tables(tmp_path, y, e, uh)
    out, err = cli(["-burnin", "1024", "-iter", "2048", "-de", "3", "3"] + files, timeout=600)
    rows = [l.split("\t") for l in out.strip().split("\n")[2:]]
    pp = np.array([float(r[2]) for r in rows])
    assert len(rows) == 200
    assert np.mean(pp[:n] > 0.9) >= 0.9, pp[:n]
    assert np.mean(pp[n:] < 0.5) >= 0.8, np.sort(pp[n:])[-20:]
    assert "sampling after" in err


@pytest.mark.gpu
def test_200000_features_shape_and_memory(gpu, tmp_path):
    from mmseq_amd.diff import Diff
    F, S = 200000, 6
    y, e, uh, _ = synth(F, S, seed=1)
    files = write_tables(tmp_path, y, e, uh)
    out, _ = cli(FAST + ["-de", "3", "3"] + files, timeout=600)
    lines = out.split("\n")
    assert lines[0] == "#prior_probability=0.1" and len(lines) == F + 3 and lines[-1] == ""
    assert all(len(l.split("\t")) == 3 + 2 + 1 + 2 * S for l in lines[1:-1:997])
    M, P0, P1, C = R.de_design([3, 3])
    d = Diff(y, e, M, P0, P1, C)
    # y, e^2 and the state: 2 * F * S doubles plus 2 * (11 + 6 + 11 + 5 * classes) + 3 slots per feature (P1 only has a column)
    assert d.device_bytes() < F * 8 * (2 * S + 80)
    d.close()
