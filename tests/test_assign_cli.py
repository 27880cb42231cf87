"""CPU checks of mmseq -assign: the flag is known, listed by -h, refused with -gpus > 1 before any device use, and without a device
the run fails exactly as it does without the flag."""
import os
import subprocess

import pytest

from oracle import host_oracle as H
from test_cli import dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN_DIR = os.environ.get("MMSEQ_HOST_BIN_DIR") or os.path.join(ROOT, "mmseq_amd", "csrc")   # (make -C mmseq_amd/csrc asan: a sanitizer build)
MMSEQ = os.path.join(BIN_DIR, "mmseq")


def run(args):
    return subprocess.run([MMSEQ] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_help_lists_the_flag():
    r = run(["-h"])
    assert r.returncode == 1 and b"-assign" in r.stderr


def test_several_devices_are_refused_before_device_use(tmp_path):
    p = tmp_path / "x.hits"
    p.write_bytes(H.write_hits_text(dataset(n_reads=300)))
    r = run(["-assign", "-gpus", "2", str(p), str(tmp_path / "out")])
    assert r.returncode == 1
    assert b"Error: -assign reads the chain's trace on one device: it cannot be combined with -gpus > 1.\n" in r.stderr
    assert r.stdout == b"" and b"no HIP device" not in r.stderr
    assert not (tmp_path / "out.k").exists()          # refused before the hits file was read


def test_without_a_device_the_flag_changes_nothing(tmp_path):
    from mmseq_amd import gibbs
    if gibbs.device_count() > 0:
        pytest.skip("a HIP device is present")
    p = tmp_path / "x.hits"
    p.write_bytes(H.write_hits_text(dataset(n_reads=300)))
    plain = run([str(p), str(tmp_path / "out")])
    flag = run(["-assign", str(p), str(tmp_path / "out")])
    assert flag.returncode == plain.returncode == 1
    assert flag.stderr == plain.stderr and flag.stdout == plain.stdout
    assert flag.stderr.endswith(b"Error: no HIP device available: libmmgibbs has no CPU fallback (mmg_problem_create(&pd, device, &prob))\n")
    for ext in (".assign", ".counts", ".gene.counts"):
        assert not (tmp_path / ("out" + ext)).exists()
