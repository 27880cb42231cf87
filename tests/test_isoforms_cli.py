"""mmseq -isoforms without a device: the usage text names the flags, every refusal exits 1 with its message before the reads and
before any device is looked for, and writes nothing."""
import os

import pytest

from test_cli import run


def test_help_names_both_flags():
    r = run(["-help"])
    assert r.returncode == 1 and b"\n  -isoforms " in r.stderr and b"\n  -iso_thresholds STR" in r.stderr
    assert b".isoforms" in r.stderr and b".gene.isoforms" in r.stderr and b"0.1,0.5" in r.stderr


@pytest.mark.parametrize("args,message", [
    (["-isoforms", "-gpus", "2"], b"Error: -isoforms reads the chain's trace on one device: it cannot be combined with -gpus > 1."),
    (["-iso_thresholds", "0.2"], b"Error: -iso_thresholds needs -isoforms."),
    (["-isoforms", "-iso_thresholds", "0.1,abc"], b"Error: -iso_thresholds: `abc` is no number."),
    (["-isoforms", "-iso_thresholds", "0.1x"], b"Error: -iso_thresholds: `0.1x` is no number."),
    (["-isoforms", "-iso_thresholds", "0.1,,0.5"], b"Error: -iso_thresholds: `` is no number."),
    (["-isoforms", "-iso_thresholds", ""], b"Error: -iso_thresholds: `` is no number."),
    (["-isoforms", "-iso_thresholds", "1"], b"Error: -iso_thresholds: 1 lies outside [0, 1)."),
    (["-isoforms", "-iso_thresholds", "0.5,-0.1"], b"Error: -iso_thresholds: -0.1 lies outside [0, 1)."),
    (["-isoforms", "-iso_thresholds", "nan"], b"Error: -iso_thresholds: nan lies outside [0, 1)."),
    (["-isoforms", "-iso_thresholds", "inf"], b"Error: -iso_thresholds: inf lies outside [0, 1)."),
    (["-isoforms", "-iso_thresholds", ",".join(["0.1"] * 9)], b"Error: -iso_thresholds takes at most 8 thresholds."),
])
def test_refusals_come_before_the_reads_and_the_device(tmp_path, args, message):
    """(the hits file does not exist: a refusal that came after the reads would say so instead)"""
    r = run(args + [str(tmp_path / "missing.hits"), str(tmp_path / "out")])
    assert r.returncode == 1 and message in r.stderr, r.stderr.decode()
    assert b"no HIP device available" not in r.stderr and b"missing.hits" not in r.stderr
    assert os.listdir(tmp_path) == []


def test_eight_thresholds_and_the_edges_of_the_range_are_accepted(tmp_path):
    """the command line passes: what stops the run is the hits file that is not there"""
    r = run(["-isoforms", "-iso_thresholds", "0,0.125,0.25,0.375,0.5,0.625,0.75,0.9999999", str(tmp_path / "missing.hits"), str(tmp_path / "out")])
    assert r.returncode != 0 and b"-iso_thresholds" not in r.stderr.split(b"Usage")[0] and b"missing.hits" in r.stderr
