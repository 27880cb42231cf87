"""CPU checks of the mmdiff CLI (src/mmdiff.cpp): usage and exit codes, every validation error before any device is touched, header
lookup, feature mismatch, NA, the normalisation factors, the matrices file, -tracedir, and a loud failure without a device."""
import os
import re
import subprocess

import numpy as np
import pytest

import mmdiff_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN_DIR = os.environ.get("MMSEQ_HOST_BIN_DIR") or os.path.join(ROOT, "mmseq_amd", "csrc")
MMDIFF = os.path.join(BIN_DIR, "mmdiff")
NODEV = dict(os.environ, HIP_VISIBLE_DEVICES="-1")


def run(args, env=NODEV):
    return subprocess.run([MMDIFF] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)


def table(path, names, y, sd, uh, cols=("feature_id", "log_mu", "sd", "mcse", "iact", "effective_length", "true_length", "unique_hits")):
    with open(path, "w") as f:
        f.write("# Mapped fragments: 1000\n")
        f.write("\t".join(cols) + "\n")
        for n, a, b, u in zip(names, y, sd, uh):
            vals = {"feature_id": n, "log_mu": repr(float(a)) if not isinstance(a, str) else a, "sd": repr(float(b)), "unique_hits": str(u),
                    "mean_probit_proportion": repr(float(a)) if not isinstance(a, str) else a, "sd_probit_proportion": repr(float(b))}
            f.write("\t".join(vals.get(c, "1") for c in cols) + "\n")
    return path


def samples(tmp_path, S=4, F=150, seed=0, **kw):
    rng = np.random.default_rng(seed)
    names = ["f%d" % i for i in range(F)]
    files = []
    for s in range(S):
        files.append(table(str(tmp_path / ("s%d.mmseq" % s)), names, rng.normal(2, 1, F), rng.uniform(0.1, 0.5, F),
                           rng.integers(0, 4, F), **kw))
    return files


def test_usage_on_no_arguments():
    r = run([])
    assert r.returncode == 1
    assert b"Error: mandatory arguments missing." in r.stderr
    assert b"Usage: mmdiff [OPTIONS...] [-de n1 n2 ... nC | -m matrices_file] mmseq_file1 mmseq_file2... > out.mmdiff" in r.stderr
    assert b"-tracedir STRING  not implemented" in r.stderr


def test_help_exits_1():
    r = run(["-h"])
    assert r.returncode == 1 and r.stderr.startswith(b"Bayesian model selection for RNA-seq expression estimates.\nUsage: mmdiff")


@pytest.mark.parametrize("args,msg", [
    (["-x", "a", "b", "c"], b"Error: unrecognised option -x."),
    (["-p", "1.5", "-de", "1", "2", "a", "b", "c"], b"Error: p must be between 0 and 1."),
    (["-s", "0", "-de", "1", "2", "a", "b", "c"], b"Error: s must be positive."),
    (["-d", "-1", "-de", "1", "2", "a", "b", "c"], b"Error: d must be positive."),
    (["-pdash", "2", "-de", "1", "2", "a", "b", "c"], b"Error: pdash must be between 0 and 1."),
    (["-burnin", "1000", "-de", "1", "2", "a", "b", "c"], b"Error: burnin and iter parameters must be multiples of 1024"),
    (["-iter", "0", "-de", "1", "2", "a", "b", "c"], b"Error: negative burnin and iter parameters."),
    (["-de", "1", "2", "-p", "0.2", "a", "b", "c"], b"Error: optional arguments must be specified before -de or -m."),
    (["-de", "1", "0", "a", "b", "c"], b"Error: each grouping must contain at least one sample"),
    (["-de", "1", "3", "a", "b", "c"], b"Error: total number of samples specified with -de must equal number of MMSEQ files"),
    (["-de", "3", "a", "b", "c"], b"Error: -de requires at least two groupings"),
    (["-nonorm", "a", "b", "c"], b"Error: either -de or -m must be specified"),
    (["-uhfrac", "0.1", "-de", "1", "2", "a", "b", "c"], b"Error: uhfrac must be <= 1 and >= 1/N."),
    (["-tracedir", "t", "-de", "1", "2", "a", "b", "c"], b"Error: -tracedir is not implemented"),
    (["-de", "1", "2", "missing1.mmseq", "missing2.mmseq", "missing3.mmseq"], b"Error: couldn't open missing1.mmseq"),
])
def test_validation_errors_exit_1(args, msg):
    r = run(args)
    assert r.returncode == 1, r.stderr
    assert msg in r.stderr, r.stderr
    assert b"no HIP device" not in r.stderr and r.stdout == b""


def test_columns_are_found_by_header_name(tmp_path):
    cols = ("unique_hits", "sd", "feature_id", "mcse", "log_mu")
    files = samples(tmp_path, S=3, F=10, cols=cols)
    r = run(["-de", "1", "2"] + files)
    assert b"Analysing 10 features" in r.stderr and b"input tables must have" not in r.stderr
    files = samples(tmp_path, S=3, F=10, cols=("feature_id", "log_mu", "unique_hits"))
    r = run(["-de", "1", "2"] + files)
    assert r.returncode == 1 and b"Error: input tables must have feature_id, log_mu, sd and unique_hits columns." in r.stderr
    r = run(["-useprops", "-de", "1", "2"] + files)
    assert r.returncode == 1 and b"feature_id, mean_probit_proportion, sd_probit_proportion and unique_hits" in r.stderr


def test_feature_mismatch_and_na(tmp_path):
    a = table(str(tmp_path / "a.mmseq"), ["x", "y"], [1, 2], [0.1, 0.1], [1, 1])
    b = table(str(tmp_path / "b.mmseq"), ["x", "z"], [1, 2], [0.1, 0.1], [1, 1])
    r = run(["-de", "1", "2", a, a, b])
    assert r.returncode == 1 and b"Error: features across files do not match (1,z,y)" in r.stderr
    c = table(str(tmp_path / "c.mmseq"), ["x", "y"], [1, "NA"], [0.1, 0.1], [1, 1])
    r = run(["-de", "1", "2", a, a, c])
    assert r.returncode == 1 and b"Error: encountered NA" in r.stderr


def test_normalisation_factors_match_numpy(tmp_path):
    files = samples(tmp_path, S=4, F=150)
    r = run(["-de", "2", "2"] + files)
    assert b"Min unique hits fraction for normalisation: 1" in r.stderr
    tabs = [R.read_table(f) for f in files]
    y = np.stack([t[1] for t in tabs], 1)
    uh = np.stack([t[3] for t in tabs], 1)
    use = int(np.sum(np.all(uh > 0, 1)))
    if use < 100:
        assert b"Warning: fewer than 100 features found for normalisation. Skipping." in r.stderr
    r = run(["-uhfrac", "0.25", "-de", "2", "2"] + files)
    _, factors = R.normalise(y, uh, 0.25)
    assert factors is not None
    assert ("Using %d/150 features for normalisation." % int(np.sum(np.mean(uh > 0, 1) >= 0.25))).encode() in r.stderr
    got = re.findall(rb"\t(\S+)\t(\S+)\n", r.stderr.split(b"Log scale normalisation factors:\n")[1])
    assert [float(v) for _, v in got] == pytest.approx(factors, rel=1e-5, abs=1e-6)
    assert [n.decode() for n, _ in got] == files


def write_matrices(path, text):
    with open(path, "w") as f:
        f.write(text)
    return str(path)


@pytest.mark.parametrize("text,msg", [
    ("1\n1\n1\n1\n\n0 0\n0 0\n0 1\n0 1\n\n1\n\n1\n2\n3\n", b"Error: more distinct rows of P than classes for model 1 (2 > 1)."),
    ("1\n1\n1\n1\n1\n\n0 0\n", b"Error: number of rows of matrices greater than number of samples."),
    ("1\n1\n1\n1\n\n1 1\n1 1\n1 2\n1 2\n\n1\n\n1\n-1\n", b"Error: need at least one class in each model labelled 0."),
    ("1\n1\n1\n1\n\n0 0\n0 0\n0 1\n0 1\n\n1\n\n1\n", b"Error: number of classes does not correspond to number of disinct rows of P for  model 1."),
    ("1\n1\n1\n1\n\n0 0\n0 0\n0 0\n0 0\n\n1\n\n1 1\n", b"Error: collinearity in matrix P1"),
    ("0 1\n0 2\n1 3\n1 4\n\n0 0\n0 0\n0 1\n0 1\n\n1\n\n1\n-1\n", None),
    ("1 1\n2 2\n3 3\n4 4\n\n0 0\n0 0\n0 1\n0 1\n\n1\n\n1\n-1\n", b"Error: collinearity in combined matrix of intercept and covariates for model 0"),
])
def test_matrices_file_parse_and_collinearity(tmp_path, text, msg):
    files = samples(tmp_path, S=4, F=20)
    m = write_matrices(tmp_path / "mat.txt", text)
    r = run(["-m", m] + files)
    assert r.returncode == 1
    if msg is None:   # a valid design: only the device is missing
        assert b"Design matrix for model 0 ([1|M]):" in r.stderr and b"Design matrix for model 1 ([1|M|P0]):" in r.stderr
    else:
        assert msg in r.stderr, r.stderr
        assert b"no HIP device" not in r.stderr


def test_without_device_fails_loudly_after_reading_the_inputs(tmp_path):
    from mmseq_amd import gibbs
    if gibbs.device_count() > 0:
        pytest.skip("a HIP device is present")
    files = samples(tmp_path, S=4, F=120)
    r = run(["-de", "2", "2"] + files, env=dict(os.environ))
    assert r.returncode == 1
    assert b"Analysing 120 features" in r.stderr and b"Design matrix for model 1 ([1||P0]):" in r.stderr   # (the reference's separator logic)
    assert b"Error: no HIP device available: mmdiff has no CPU fallback" in r.stderr
    assert r.stdout == b""


@pytest.mark.parametrize("bad", ["nan", "inf", "-inf", "NaN"])
@pytest.mark.parametrize("column", ["log_mu", "sd"])
def test_non_finite_entries_exit_1_before_the_device(tmp_path, bad, column):
    """atof accepts "nan" and "inf"; they would reach the device's log densities and samplers, so they are errors like "NA"."""
    names = ["x", "y", "z"]
    a = table(str(tmp_path / "a.mmseq"), names, [1, 2, 3], [0.1, 0.1, 0.1], [1, 1, 1])
    y, sd = [1, 2, 3], [0.1, 0.1, 0.1]
    if column == "log_mu":
        y[1] = bad
    else:
        sd = [0.1, float(bad), 0.1]
    b = table(str(tmp_path / "b.mmseq"), names, y, sd, [1, 1, 1])
    r = run(["-de", "1", "2", a, a, b], env=dict(os.environ))
    assert r.returncode == 1
    assert b"Error: encountered a non-finite value (feature y in " + b.encode() + b")" in r.stderr
    assert b"no HIP device" not in r.stderr and b"Design matrix" not in r.stderr and r.stdout == b""


@pytest.mark.parametrize("args,msg", [
    (["-d", "inf"], b"Error: d must be positive."),
    (["-s", "nan"], b"Error: s must be positive."),
    (["-p", "nan"], b"Error: p must be between 0 and 1."),
    (["-pdash", "nan"], b"Error: pdash must be between 0 and 1."),
])
def test_non_finite_hyperparameters_exit_1(args, msg):
    r = run(args + ["-de", "1", "2", "a", "b", "c"])
    assert r.returncode == 1 and msg in r.stderr


def test_non_finite_design_entry_exits_1(tmp_path):
    files = samples(tmp_path, S=4, F=20)
    m = write_matrices(tmp_path / "mat.txt", "0 nan\n0 2\n1 3\n1 4\n\n0 0\n0 0\n0 1\n0 1\n\n1\n\n1\n-1\n")
    r = run(["-m", m] + files)
    assert r.returncode == 1 and b"Error: non-finite value in the design matrices." in r.stderr


def test_library_rejects_non_finite_input_before_the_device():
    """mmg_diff_create checks its arguments before it looks for a device: the same error with or without one."""
    from mmseq_amd._lib import MMGError
    from mmseq_amd.diff import Diff
    M, P0, P1, C = R.de_design([3, 3])
    y = np.ones((4, 6))
    y[2, 3] = np.nan
    with pytest.raises(MMGError) as ex:
        Diff(y, np.full((4, 6), 0.1), M, P0, P1, C)
    assert ex.value.code == 1 and "finite" in str(ex.value)

