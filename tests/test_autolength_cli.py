"""mmseq -gibbs_auto MAX [-auto_ess E] [-auto_rhat R] [-auto_frac F]: the refusals (CPU: each exits 1 with its message and the usage
text before the hits file is opened or a device looked for), and on the GPU the identity the flag promises -- every output but
BASE.autolength is byte for byte what a plain `mmseq -gibbs_iter L` writes for the length L the run stopped at."""
import glob
import gzip
import os

import pytest

from oracle import host_oracle as H
from test_cli import dataset, run

USAGE = b"Usage: mmseq [OPTIONS...] hits_file output_base"


@pytest.mark.parametrize("args,message", [
    (["-gibbs_auto", "3000"], b"-gibbs_auto must be gibbs_iter times a power of 2"),                       # default gibbs_iter 16384
    (["-gibbs_iter", "2048", "-gibbs_auto", "6144"], b"-gibbs_auto must be gibbs_iter times a power of 2"),  # 3 x
    (["-gibbs_iter", "2048", "-gibbs_auto", "1024"], b"-gibbs_auto must be gibbs_iter times a power of 2"),  # below the start
    (["-gibbs_iter", "2048", "-gibbs_auto", "0"], b"-gibbs_auto must be gibbs_iter times a power of 2"),
    (["-gibbs_iter", "1024", "-gibbs_auto", "2147483647"], b"-gibbs_auto must be at most 2^30"),
    (["-gibbs_iter", "1024", "-gibbs_auto", "2048", "-gpus", "2"], b"-gibbs_auto extends the chains on one device"),
    (["-gibbs_iter", "1024", "-gibbs_auto", "2048", "-auto_ess", "0"], b"-auto_ess must be a number > 0"),
    (["-gibbs_iter", "1024", "-gibbs_auto", "2048", "-auto_ess", "-5"], b"-auto_ess must be a number > 0"),
    (["-gibbs_iter", "1024", "-gibbs_auto", "2048", "-auto_ess", "many"], b"-auto_ess must be a number > 0"),
    (["-gibbs_iter", "1024", "-gibbs_auto", "2048", "-auto_rhat", "1"], b"-auto_rhat must be a number > 1"),
    (["-gibbs_iter", "1024", "-gibbs_auto", "2048", "-auto_rhat", "0.99"], b"-auto_rhat must be a number > 1"),
    (["-gibbs_iter", "1024", "-gibbs_auto", "2048", "-auto_frac", "0"], b"-auto_frac must be a number in (0, 1]"),
    (["-gibbs_iter", "1024", "-gibbs_auto", "2048", "-auto_frac", "1.01"], b"-auto_frac must be a number in (0, 1]"),
    (["-gibbs_iter", "1024", "-gibbs_auto", "2048", "-auto_frac", "nan"], b"-auto_frac must be a number in (0, 1]"),
    (["-auto_ess", "300"], b"-auto_ess, -auto_rhat and -auto_frac need -gibbs_auto"),
    (["-auto_rhat", "1.05"], b"-auto_ess, -auto_rhat and -auto_frac need -gibbs_auto"),
    (["-auto_frac", "0.9"], b"-auto_ess, -auto_rhat and -auto_frac need -gibbs_auto"),
])
def test_refusals_come_before_the_reads_and_the_device(tmp_path, args, message):
    r = run(args + [str(tmp_path / "no_such.hits"), str(tmp_path / "out")])
    assert r.returncode == 1 and message in r.stderr and USAGE in r.stderr, r.stderr
    assert b"Error reading hits file" not in r.stderr and r.stdout == b""
    assert glob.glob(str(tmp_path / "out*")) == []


def test_usage_lists_the_flags():
    r = run(["-help"])
    for flag in (b"-gibbs_auto MAX", b"-auto_ess FLOAT", b"-auto_rhat FLOAT", b"-auto_frac FLOAT"):
        assert flag in r.stderr


def _files(base):
    out = {}
    for path in sorted(glob.glob(base + ".*")):
        key = path[len(base):]
        out[key] = gzip.open(path, "rb").read() if path.endswith(".gz") else open(path, "rb").read()
    return out


def _stages(base):
    lines = open(base + ".autolength").read().rstrip("\n").split("\n")
    assert lines[0].startswith("# auto_ess ") and " auto_rhat " in lines[0] and " auto_frac " in lines[0] and lines[0].endswith(" chains 2")
    rows = [ln.split("\t") for ln in lines[1:]]
    assert all(len(r) == 7 for r in rows)
    return rows


def _check_identity(tmp_path, hits, name, auto_args, extra):
    base = str(tmp_path / name)
    r = run(["-chains", "2", "-gibbs_iter", "1024", "-gibbs_auto", "4096"] + auto_args + extra + [hits, base], timeout=300)
    assert r.returncode == 0, r.stderr
    assert (base + ".autolength").encode() in r.stdout                 # listed with the other outputs
    rows = _stages(base)
    assert r.stdout.count(b"Gibbs auto: length ") == len(rows)           # one line per stage
    lengths = [int(x[0]) for x in rows]
    assert lengths == [1024 << j for j in range(len(rows))] and [int(x[1]) for x in rows] == [v // 1024 for v in lengths]
    assert [x[6] for x in rows[:-1]] == ["extend"] * (len(rows) - 1) and rows[-1][6] in ("stop", "max")
    L = lengths[-1]
    plain = str(tmp_path / (name + "_plain"))
    r = run(["-chains", "2", "-gibbs_iter", str(L)] + extra + [hits, plain], timeout=300)
    assert r.returncode == 0, r.stderr
    got, want = _files(base), _files(plain)
    assert ".autolength" in got and ".autolength" not in want
    del got[".autolength"]
    assert sorted(got) == sorted(want) and {".trace_gibbs.gz", ".identical.trace_gibbs.gz", ".gene.trace_gibbs.gz", ".prop.trace_gibbs.gz"} <= set(got)
    for key in want:
        assert got[key] == want[key], key
    return rows


@pytest.fixture(scope="module")
def hits_file(tmp_path_factory):
    p = tmp_path_factory.mktemp("autolength") / "in.hits"
    p.write_bytes(H.write_hits_binary(dataset()))
    return str(p)


@pytest.mark.gpu
def test_outputs_equal_a_plain_run_of_the_length_it_stopped_at(tmp_path, hits_file, gpu):
    _check_identity(tmp_path, hits_file, "auto", [], ["-convergence", "-pool", "-assign", "-pairs", "-isoforms"])


@pytest.mark.gpu
def test_targets_beyond_reach_end_at_max(tmp_path, hits_file, gpu):
    rows = _check_identity(tmp_path, hits_file, "far", ["-auto_ess", "1e9"], [])
    assert rows[-1][6] == "max" and int(rows[-1][0]) == 4096 and len(rows) == 3
    assert all(int(x[3]) == 0 for x in rows)                             # nothing passes an ESS of 1e9
