"""CPU checks of the mmfold CLI: the usage text, every refusal with its message and exit code 1 before any device is looked for, and a
loud failure without a device once the inputs are in order.  Fixtures are tiny hand-made tables and gzip traces."""
import gzip
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN_DIR = os.environ.get("MMSEQ_HOST_BIN_DIR") or os.path.join(ROOT, "mmseq_amd", "csrc")
MMFOLD = os.path.join(BIN_DIR, "mmfold")
NODEV = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
TRACELEN = 1024
INFIX = {"transcript": "", "identical": ".identical", "gene": ".gene"}


def run(args, env=NODEV):
    return subprocess.run([MMFOLD] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)


def write_table(path, ids, log_mu, uh):
    with open(path, "w") as f:
        f.write("# Mapped fragments: 1000\n")
        f.write("feature_id\tlog_mu\tsd\tmcse\tiact\teffective_length\ttrue_length\tunique_hits\n")
        for n, m, u in zip(ids, log_mu, uh):
            f.write("%s\t%s\t0.1\t0.01\t1\t1000\t1200\t%d\n" % (n, m if isinstance(m, str) else repr(float(m)), u))


def write_trace(path, ids, draws, rows=TRACELEN):
    """draws: (len(ids), TRACELEN); written as mmseq writes them, six significant digits.  Returns the values as they read back."""
    text = [" ".join(ids)]
    for k in range(rows):
        text.append(" ".join("%g" % draws[c][k] for c in range(len(ids))))
    with gzip.open(path, "wt") as f:
        f.write("\n".join(text) + "\n")
    return np.array([[float("%g" % v) for v in row] for row in draws])


def sample(tmp_path, name, level="transcript", ids=("t0", "t1", "t2"), seed=0, trace_ids=None, rows=TRACELEN, log_mu=None, uh=None):
    rng = np.random.default_rng(seed)
    base = str(tmp_path / name)
    ids = list(ids)
    lm = rng.normal(1.0, 1.0, len(ids)) if log_mu is None else log_mu
    write_table(base + INFIX[level] + ".mmseq", ids, lm, [2] * len(ids) if uh is None else uh)
    tids = ids if trace_ids is None else list(trace_ids)
    draws = np.exp(rng.normal(0.0, 0.3, (len(tids), TRACELEN)))
    write_trace(base + INFIX[level] + ".trace_gibbs.gz", tids, draws, rows)
    return base


@pytest.fixture(scope="module")
def pair(tmp_path_factory):
    d = tmp_path_factory.mktemp("mmfold")
    return sample(d, "a", seed=1), sample(d, "b", seed=2)


def _refused(r, msg):
    assert r.returncode == 1, r
    assert msg in r.stderr, r.stderr
    assert b"Usage: mmfold" in r.stderr and r.stdout == b""
    assert b"HIP" not in r.stderr.split(b"Usage: mmfold")[0]                    # refused before a device was looked for


def test_usage_names_every_flag_and_says_what_it_is_not():
    r = run(["-h"])
    assert r.returncode == 1 and r.stdout == b""
    for flag in (b"-level", b"transcript|identical|gene", b"-nonorm", b"-offset FLOAT", b"-uhmin INT", b"-percentiles", b"-gfold", b"-device INT",
                 b"baseA baseB"):
        assert flag in r.stderr, flag
    text = b" ".join(r.stderr.split())
    assert b"This is the posterior given the reads of these two libraries; it says nothing about biological variability: for groups with replicates the tool is mmdiff." in text


@pytest.mark.parametrize("n", [0, 1, 3])
def test_wrong_number_of_bases(pair, n):
    _refused(run((list(pair) + [pair[0]])[:n]), b"Error: exactly two basenames are needed (%d given)." % n)


@pytest.mark.parametrize("args,msg", [
    (["-level", "exon"], b"Error: unknown level exon"),
    (["-nonorm", "-offset", "0.5"], b"Error: -nonorm and -offset exclude each other."),
    (["-offset", "inf"], b"Error: -offset must be a finite number."),
    (["-offset", "nan"], b"Error: -offset must be a finite number."),
    (["-offset", "1.5x"], b"Error: -offset must be a finite number."),
    (["-percentiles", "2.5,101"], b"Error: percentiles must be numbers between 0 and 100."),
    (["-percentiles", "-1"], b"Error: percentiles must be numbers between 0 and 100."),
    (["-percentiles", "5,x"], b"Error: percentiles must be numbers between 0 and 100."),
    (["-gfold", "0"], b"Error: -gfold must be above 0 and below 0.5."),
    (["-gfold", "0.5"], b"Error: -gfold must be above 0 and below 0.5."),
    (["-gfold", "-0.1"], b"Error: -gfold must be above 0 and below 0.5."),
    (["-percentiles", ",".join(str(i) for i in range(63))], b"Error: more than 64 ranks (63 percentiles and the two of -gfold)."),
    (["-uhmin", "-2"], b"Error: -uhmin must be a non-negative integer."),
    (["-device", "x"], b"Error: -device must be a non-negative integer."),
    (["-frobnicate"], b"Error: unrecognised option -frobnicate."),
])
def test_refusals_of_the_options(pair, args, msg):
    _refused(run(args + list(pair)), msg)


def test_an_option_without_its_value(pair):
    _refused(run(list(pair) + ["-offset"]), b"Error: -offset needs a value.")


def test_missing_and_unreadable_files(tmp_path, pair):
    a, b = pair
    _refused(run([a, str(tmp_path / "nothing")]), b"Error: cannot open " + str(tmp_path / "nothing").encode() + b".mmseq")
    _refused(run(["-level", "gene", a, b]), b"Error: cannot open " + a.encode() + b".gene.mmseq")
    c = sample(tmp_path, "c", seed=3)
    os.remove(c + ".trace_gibbs.gz")
    _refused(run([a, c]), b"Error: couldn't open " + c.encode() + b".trace_gibbs.gz.")
    d = sample(tmp_path, "d", seed=4)
    with open(d + ".trace_gibbs.gz", "wb") as f:
        f.write(b"")
    _refused(run([d, a]), d.encode() + b".trace_gibbs.gz is empty.")
    e = sample(tmp_path, "e", seed=5)
    with open(e + ".mmseq", "w") as f:
        f.write("# Mapped fragments: 1000\n")
    _refused(run([e, a]), e.encode() + b".mmseq is truncated")
    g = sample(tmp_path, "g", seed=6)
    with open(g + ".mmseq", "w") as f:
        f.write("feature_id\tlog_mu\tsd\nt0\t1.0\t0.1\n")
    _refused(run([a, g]), g.encode() + b".mmseq does not contain a \"unique_hits\" column.")


def test_truncated_trace(tmp_path, pair):
    short = sample(tmp_path, "short", seed=7, rows=TRACELEN - 1)
    _refused(run([pair[0], short]), b"Error: " + short.encode() + b".trace_gibbs.gz is truncated (fewer than 1024 rows).")


def test_tables_that_differ(tmp_path, pair):
    fewer = sample(tmp_path, "fewer", ids=("t0", "t1"), seed=8)
    _refused(run([pair[0], fewer]), b"Error: the two tables list different numbers of features (3 and 2).")
    other = sample(tmp_path, "other", ids=("t0", "t2", "t1"), seed=9)
    _refused(run([pair[0], other]), b"Error: the two tables do not list the same features in the same order (row 2: t1 and t2).")


def test_no_feature_sets_the_offset(tmp_path, pair):
    lone = sample(tmp_path, "lone", seed=10, uh=[0, 0, 0])
    _refused(run([pair[0], lone]), b"Error: no feature has 1 unique hits and a finite log_mu in both samples: use -nonorm or -offset.")
    na = sample(tmp_path, "na", seed=11, log_mu=["NA", "NA", "NA"])
    _refused(run(["-uhmin", "0", na, pair[1]]), b"Error: no feature has 0 unique hits and a finite log_mu in both samples")
    # with an offset given the same inputs are in order: the next stop is the device
    for flags in (["-nonorm"], ["-offset", "0.25"]):
        r = run(flags + [pair[0], lone])
        assert r.returncode == 1 and b"no CPU fallback" in r.stderr and b"Usage" not in r.stderr


@pytest.mark.parametrize("level", ["transcript", "identical", "gene"])
def test_valid_inputs_without_a_device_fail_loudly(tmp_path, level):
    a, b = sample(tmp_path, "a", level=level, seed=1), sample(tmp_path, "b", level=level, seed=2, trace_ids=("t2", "t0"))
    r = run(["-level", level, "-percentiles", "0,50,100", "-gfold", "0.05", "-uhmin", "2", a, b])
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.strip() == b"Error: no HIP device available: mmfold has no CPU fallback"
