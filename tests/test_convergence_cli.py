"""CPU checks of mmseq -convergence: the flag is known, listed by -h, and refused with -gpus > 1 before any device use."""
import os
import subprocess

import pytest

from oracle import host_oracle as H
from test_cli import dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN_DIR = os.environ.get("MMSEQ_HOST_BIN_DIR") or os.path.join(ROOT, "mmseq_amd", "csrc")
MMSEQ = os.path.join(BIN_DIR, "mmseq")


def run(args):
    return subprocess.run([MMSEQ] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_help_lists_the_flag():
    r = run(["-h"])
    assert r.returncode == 1 and b"-convergence" in r.stderr


def test_flag_is_accepted_and_fails_only_for_want_of_a_device(tmp_path):
    from mmseq_amd import gibbs
    if gibbs.device_count() > 0:
        pytest.skip("a HIP device is present")
    p = tmp_path / "x.hits"
    p.write_bytes(H.write_hits_text(dataset(n_reads=300)))
    r = run(["-convergence", "-chains", "2", str(p), str(tmp_path / "out")])
    assert r.returncode == 1
    assert b"unrecognised option" not in r.stderr and b"no HIP device available" in r.stderr


def test_several_devices_are_refused_before_device_use(tmp_path):
    p = tmp_path / "x.hits"
    p.write_bytes(H.write_hits_text(dataset(n_reads=300)))
    r = run(["-gpus", "2", "-chains", "2", "-convergence", str(p), str(tmp_path / "out")])
    assert r.returncode == 1
    assert b"-convergence needs every chain on one device" in r.stderr
    assert not (tmp_path / "out.k").exists()          # refused before the hits file was read
