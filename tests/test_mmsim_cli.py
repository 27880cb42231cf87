"""CPU checks of the mmsim CLI: the usage text, every refusal with its message and exit code 1 before any device is looked for, and a
loud failure without a device once the inputs are in order.  Fixtures are tiny generated tables and gzip traces, as
tests/test_mmfold_cli.py makes its own."""
import os
import subprocess

import numpy as np
import pytest

from sim_fixtures import INFIX, MMSIM, write_table, write_trace

NODEV = dict(os.environ, HIP_VISIBLE_DEVICES="-1")
T = 8


def run(args, env=NODEV):
    return subprocess.run([MMSIM] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)


def sample(tmp_path, name, level="transcript", ids=("t0", "t1", "t2"), seed=0, trace_ids=None, rows=T, log_mu=None, uh=None):
    rng = np.random.default_rng(seed)
    base = str(tmp_path / name)
    ids = list(ids)
    lm = rng.normal(1.0, 1.0, len(ids)) if log_mu is None else log_mu
    write_table(base + INFIX[level] + ".mmseq", ids, lm, [2] * len(ids) if uh is None else uh)
    tids = ids if trace_ids is None else list(trace_ids)
    draws = np.exp(rng.normal(0.0, 0.3, (len(tids), rows)))
    write_trace(base + INFIX[level] + ".trace_gibbs.gz", tids, draws, rows)
    return base


@pytest.fixture(scope="module")
def trio(tmp_path_factory):
    d = tmp_path_factory.mktemp("mmsim")
    return [sample(d, n, seed=i + 1) for i, n in enumerate("abc")]


def _refused(r, msg):
    assert r.returncode == 1, r
    assert msg in r.stderr, r.stderr
    assert b"Usage: mmsim" in r.stderr and r.stdout == b""
    assert b"HIP" not in r.stderr.split(b"Usage: mmsim")[0]                     # refused before a device was looked for


def test_usage_names_every_flag():
    r = run(["-h"])
    assert r.returncode == 1 and r.stdout == b""
    for flag in (b"-level", b"transcript|identical|gene", b"-nonorm", b"-uhfrac FLOAT", b"-uhmin INT", b"-centre mean|none", b"-percentiles",
                 b"-matrix FILE", b"-device INT", b"base1 base2 [base3 ...]"):
        assert flag in r.stderr, flag


@pytest.mark.parametrize("n", [0, 1])
def test_fewer_than_two_bases(trio, n):
    _refused(run(trio[:n]), b"Error: at least two basenames are needed (%d given)." % n)


def test_more_than_256_bases(trio):
    _refused(run([trio[0]] * 257), b"Error: at most 256 basenames are taken (257 given).")


@pytest.mark.parametrize("args,msg", [
    (["-level", "exon"], b"Error: unknown level exon"),
    (["-centre", "median"], b"Error: unknown centre median (mean or none)."),
    (["-percentiles", "2.5,101"], b"Error: percentiles must be numbers between 0 and 100."),
    (["-percentiles", "-1"], b"Error: percentiles must be numbers between 0 and 100."),
    (["-percentiles", "5,x"], b"Error: percentiles must be numbers between 0 and 100."),
    (["-percentiles", ",".join(str(i) for i in range(65))], b"Error: more than 64 ranks (65 percentiles)."),
    (["-uhmin", "-2"], b"Error: -uhmin must be a non-negative integer."),
    (["-uhfrac", "1.5"], b"Error: uhfrac must be <= 1 and >= 1/N."),
    (["-uhfrac", "0.1"], b"Error: uhfrac must be <= 1 and >= 1/N."),
    (["-uhfrac", "x"], b"Error: -uhfrac must be a number."),
    (["-device", "x"], b"Error: -device must be a non-negative integer."),
    (["-frobnicate"], b"Error: unrecognised option -frobnicate."),
])
def test_refusals_of_the_options(trio, args, msg):
    _refused(run(args + trio), msg)


def test_an_option_without_its_value(trio):
    _refused(run(trio + ["-matrix"]), b"Error: -matrix needs a value.")


def test_missing_and_truncated_files(tmp_path, trio):
    a, b, _ = trio
    _refused(run([a, b, str(tmp_path / "nothing")]), b"Error: cannot open " + str(tmp_path / "nothing").encode() + b".mmseq")
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
    import gzip
    k = sample(tmp_path, "k", seed=7)
    with gzip.open(k + ".trace_gibbs.gz", "wt") as f:                          # the last row lacks a value
        f.write("t0 t1 t2\n1 2 3\n4 5\n")
    _refused(run([a, k]), b"Error: " + k.encode() + b".trace_gibbs.gz is truncated (5 values are not whole rows of 3).")
    n = sample(tmp_path, "n", seed=8)
    with gzip.open(n + ".trace_gibbs.gz", "wt") as f:                          # a header and no row
        f.write("t0 t1 t2\n")
    _refused(run([a, n]), b"Error: " + n.encode() + b".trace_gibbs.gz is truncated (0 values are not whole rows of 3).")


def test_trace_lengths_that_differ_or_are_too_long(tmp_path, trio):
    short = sample(tmp_path, "short", seed=9, rows=T - 1)
    _refused(run([trio[0], trio[1], short]),
             b"Error: the trace lengths differ (8 rows in " + trio[0].encode() + b".trace_gibbs.gz and 7 in " + short.encode() + b".trace_gibbs.gz).")
    long_ = sample(tmp_path, "long", ids=("t0",), seed=10, rows=4097)
    _refused(run([long_, long_]), b".trace_gibbs.gz has 4097 rows, more than 4096.")


def test_tables_that_differ(tmp_path, trio):
    fewer = sample(tmp_path, "fewer", ids=("t0", "t1"), seed=11)
    _refused(run([trio[0], trio[1], fewer]),
             b"Error: the tables of " + trio[0].encode() + b" and " + fewer.encode() + b" list different numbers of features (3 and 2).")
    other = sample(tmp_path, "other", ids=("t0", "t2", "t1"), seed=12)
    _refused(run([trio[0], other]),
             b"Error: the tables of " + trio[0].encode() + b" and " + other.encode() + b" do not list the same features in the same order (row 2: t1 and t2).")


@pytest.mark.parametrize("level", ["transcript", "identical", "gene"])
def test_valid_inputs_without_a_device_fail_loudly(tmp_path, level):
    bases = [sample(tmp_path, n, level=level, seed=i, trace_ids=("t2", "t0") if n == "b" else None) for i, n in enumerate("abc")]
    r = run(["-level", level, "-percentiles", "0,50,100", "-centre", "none", "-uhmin", "2", "-uhfrac", "0.5", "-matrix", str(tmp_path / "m.txt")] + bases)
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.strip().splitlines()[-1] == b"Error: no HIP device available: mmsim has no CPU fallback"
    assert b"Usage" not in r.stderr and not os.path.exists(str(tmp_path / "m.txt"))
