"""CPU checks of mmseq -pool: the flag is known, listed by -h with what it does to log_mu, refused with -gpus > 1 before the hits file is
read, and a run with it gets exactly as far as a run without it (without a device: the loud failure at the device problem)."""
import os
import subprocess

from oracle import host_oracle as H
from test_cli import dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN_DIR = os.environ.get("MMSEQ_HOST_BIN_DIR") or os.path.join(ROOT, "mmseq_amd", "csrc")   # (make -C mmseq_amd/csrc asan: a sanitizer build)
MMSEQ = os.path.join(BIN_DIR, "mmseq")


def run(args):
    return subprocess.run([MMSEQ] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def test_help_lists_the_flag():
    r = run(["-h"])
    assert r.returncode == 1 and b"  -pool " in r.stderr
    text = b" ".join(r.stderr.split())
    assert b"log_mu is then the mean of log mu over the kept samples" in text and b"running moments" in text


def test_several_devices_are_refused_before_the_hits_file_is_read(tmp_path):
    p = tmp_path / "x.hits"
    p.write_bytes(H.write_hits_text(dataset(n_reads=300)))
    r = run(["-gpus", "2", "-chains", "2", "-pool", str(p), str(tmp_path / "out")])
    assert r.returncode == 1
    assert b"Error: -pool needs every chain on one device: it cannot be combined with -gpus > 1.\n" in r.stderr
    assert b"unrecognised option" not in r.stderr and b"no HIP device" not in r.stderr and r.stdout == b""
    assert not (tmp_path / "out.k").exists()


def test_the_flag_is_accepted_and_fails_only_for_want_of_a_device(tmp_path):
    from mmseq_amd import gibbs
    p = tmp_path / "x.hits"
    p.write_bytes(H.write_hits_text(dataset(n_reads=300)))
    plain = run(["-gibbs_iter", "1024", "-chains", "2", str(p), str(tmp_path / "a")])
    flag = run(["-gibbs_iter", "1024", "-chains", "2", "-pool", str(p), str(tmp_path / "b")])
    assert b"unrecognised option" not in flag.stderr
    assert flag.returncode == plain.returncode
    assert (tmp_path / "b.k").read_bytes() == (tmp_path / "a.k").read_bytes()     # the run got past the command line and the hits file
    if gibbs.device_count() == 0:
        assert flag.returncode == 1 and flag.stderr == plain.stderr
        assert flag.stderr.endswith(b"Error: no HIP device available: libmmgibbs has no CPU fallback (mmg_problem_create(&pd, device, &prob))\n")
        assert not (tmp_path / "b.mmseq").exists()
    else:
        assert flag.returncode == 0, flag.stderr.decode()
        assert (tmp_path / "b.mmseq").exists() and (tmp_path / "b.gene.mmseq").exists()
