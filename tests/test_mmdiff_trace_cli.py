"""CPU checks of `mmdiff -traces DIR`: every refusal exits 1 with its message before any device is touched, the directory is made and
checked before the device is looked for, and the usage text names the option."""
import os

import pytest

from test_mmdiff_cli import run, samples, write_matrices
from test_mmdiff_poly_cli import ALT_A, ALT_B

FAST = ["-burnin", "1024", "-iter", "1024", "-notune"]


def refused(r, msg):
    assert r.returncode == 1 and msg in r.stderr, r.stderr
    assert b"no HIP device" not in r.stderr and r.stdout == b""
    assert b"unrecognised option" not in r.stderr


def test_traces_without_a_value():
    refused(run(["-traces"]), b"Error: mandatory arguments missing.")


def test_unwritable_directory(tmp_path):
    files = samples(tmp_path, S=4, F=20)
    blocker = tmp_path / "a_file"
    blocker.write_text("x")
    bad = str(blocker / "traces")          # below a regular file: mkdir fails for every user
    refused(run(FAST + ["-traces", bad, "-de", "2", "2"] + files), b"Error: can't write to trace directory " + bad.encode() + b".")
    assert not os.path.exists(bad)


def test_traces_with_chains(tmp_path):
    files = samples(tmp_path, S=4, F=20)
    d = str(tmp_path / "tr")
    r = run(FAST + ["-traces", d, "-chains", "2", "-de", "2", "2"] + files)
    refused(r, b"Error: -traces cannot be combined with -chains, more than one -m or -polyclass")
    assert b"left for later" in r.stderr and not os.path.exists(d)


def test_traces_with_two_alternatives(tmp_path):
    files = samples(tmp_path, S=4, F=20)
    a, b = write_matrices(tmp_path / "a.mat", ALT_A), write_matrices(tmp_path / "b.mat", ALT_B)
    d = str(tmp_path / "tr")
    r = run(FAST + ["-traces", d, "-m", a, "-m", b] + files)
    refused(r, b"Error: -traces cannot be combined with -chains, more than one -m or -polyclass")
    assert not os.path.exists(d)


def test_directory_is_created_before_the_device_is_looked_for(tmp_path):
    files = samples(tmp_path, S=4, F=120)
    d = str(tmp_path / "tr")
    r = run(FAST + ["-traces", d, "-de", "2", "2"] + files)
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr.rstrip().endswith(b"Error: no HIP device available: mmdiff has no CPU fallback")
    assert os.path.isdir(d) and os.listdir(d) == []          # the files need the handle's layout: none yet
    r = run(FAST + ["-traces", d, "-de", "2", "2"] + files)   # an existing directory is fine
    assert r.stderr.rstrip().endswith(b"Error: no HIP device available: mmdiff has no CPU fallback")


def test_usage_names_traces_and_tracedir_still_refuses():
    r = run(["-h"])
    for text in (b"-traces STRING", b"sigar<model>.txt is not", b"not with -chains or repeated -m", b"-tracedir STRING  not implemented"):
        assert text in r.stderr, text
    r = run(["-tracedir", "t", "-de", "1", "2", "a", "b", "c"])
    refused(r, b"Error: -tracedir is not implemented")
    assert b"-traces DIR" in r.stderr


def test_library_refuses_bad_trace_arguments_without_a_handle():
    from mmseq_amd import _lib
    lib = _lib.load()
    assert lib.mmg_diff_trace_open(None, 1, 1, None, None) == 1
    assert lib.mmg_diff_trace_layout(None, None, None) == 1
    assert lib.mmg_diff_get_tune_state(None, None, None) == 1
    assert lib.mmg_diff_get_pseudo(None, None) == 1
