"""CPU checks of `mmdiff -effects FILE`: every refusal exits 1 with its message before any device is touched, and the usage text
lists the options."""
import os

import pytest

from test_mmdiff_cli import run, samples, write_matrices
from test_mmdiff_poly_cli import ALT_A, ALT_B

FAST = ["-burnin", "1024", "-iter", "1024", "-notune"]


def refused(r, msg):
    assert r.returncode == 1 and msg in r.stderr, r.stderr
    assert b"no HIP device" not in r.stderr and r.stdout == b""
    assert b"unrecognised option" not in r.stderr


def test_effects_without_a_value():
    refused(run(["-effects"]), b"Error: mandatory arguments missing.")


def test_effects_with_traces(tmp_path):
    files = samples(tmp_path, S=4, F=20)
    out, d = str(tmp_path / "fx.txt"), str(tmp_path / "tr")
    r = run(FAST + ["-effects", out, "-traces", d, "-de", "2", "2"] + files)
    refused(r, b"Error: -effects cannot be combined with -traces")
    assert not os.path.exists(out) and not os.path.exists(d)


def test_effects_with_chains(tmp_path):
    files = samples(tmp_path, S=4, F=20)
    out = str(tmp_path / "fx.txt")
    r = run(FAST + ["-effects", out, "-chains", "2", "-de", "2", "2"] + files)
    refused(r, b"Error: -effects cannot be combined with -chains, more than one -m or -polyclass")
    assert b"left for later" in r.stderr and not os.path.exists(out)


def test_effects_with_two_alternatives(tmp_path):
    files = samples(tmp_path, S=4, F=20)
    a, b = write_matrices(tmp_path / "a.mat", ALT_A), write_matrices(tmp_path / "b.mat", ALT_B)
    out = str(tmp_path / "fx.txt")
    refused(run(FAST + ["-effects", out, "-m", a, "-m", b] + files), b"Error: -effects cannot be combined with -chains, more than one -m or -polyclass")
    assert not os.path.exists(out)


def test_effects_with_polyclass(tmp_path):
    refused(run(["-polyclass", "-effects", str(tmp_path / "fx.txt"), "a.mmdiff", "b.mmdiff"]),
            b"Error: -effects cannot be combined with -chains, more than one -m or -polyclass")


@pytest.mark.parametrize("opt", [["-effects_every", "4"], ["-effects_percentiles", "5,95"]])
def test_effects_options_need_effects(tmp_path, opt):
    files = samples(tmp_path, S=4, F=20)
    refused(run(FAST + opt + ["-de", "2", "2"] + files), b"Error: -effects_every and -effects_percentiles need -effects.")


@pytest.mark.parametrize("text", ["", "5,", ",5", "5,,95", "abc", "5;95", "-1", "100.5", "nan", "inf", "2.5,50,x", ",".join(["50"] * 33)])
def test_malformed_percentile_lists(tmp_path, text):
    files = samples(tmp_path, S=4, F=20)
    out = str(tmp_path / "fx.txt")
    r = run(FAST + ["-effects", out, "-effects_percentiles", text, "-de", "2", "2"] + files)
    refused(r, b"Error: -effects_percentiles takes a comma-separated list of 1 to 32 percentiles in [0, 100].")
    assert not os.path.exists(out)


@pytest.mark.parametrize("value", ["0", "-3", "x", "2.5", "1073741825", ""])
def test_malformed_effects_every(tmp_path, value):
    files = samples(tmp_path, S=4, F=20)
    r = run(FAST + ["-effects", str(tmp_path / "fx.txt"), "-effects_every", value, "-de", "2", "2"] + files)
    refused(r, b"Error: -effects_every takes an integer between 1 and 1073741824.")


def test_more_than_4096_rows(tmp_path):
    files = samples(tmp_path, S=4, F=20)
    out = str(tmp_path / "fx.txt")
    r = run(["-burnin", "1024", "-iter", "8192", "-effects", out, "-effects_every", "1", "-de", "2", "2"] + files)
    refused(r, b"Error: -effects keeps at most 4096 rows: -iter 8192 with -effects_every 1 needs 8192.")
    r = run(["-burnin", "1024", "-iter", "12288", "-effects", out, "-effects_every", "2", "-de", "2", "2"] + files)
    refused(r, b"Error: -effects keeps at most 4096 rows")
    assert not os.path.exists(out)


def test_accepted_arguments_reach_the_device_check(tmp_path):
    """The default interval (iter / 1024: 4096 rows would be 4 x 1024) and a list of 32 percentiles pass every check; without a device
    the run ends where it looks for one, and FILE is not created."""
    files = samples(tmp_path, S=4, F=120)
    out = str(tmp_path / "fx.txt")
    for extra in ([], ["-effects_every", "4"], ["-effects_percentiles", ",".join(["12.5"] * 32)], ["-effects_percentiles", "0,100"]):
        r = run(["-burnin", "1024", "-iter", "4096", "-notune", "-effects", out] + extra + ["-de", "2", "2"] + files)
        assert r.returncode == 1 and r.stdout == b""
        assert r.stderr.rstrip().endswith(b"Error: no HIP device available: mmdiff has no CPU fallback"), r.stderr
    assert not os.path.exists(out)


def test_usage_lists_the_effects_options():
    r = run(["-h"])
    for text in (b"-effects STRING", b"-effects_every INT", b"-effects_percentiles P1,P2,...", b"at most 4096", b"(default: 2.5,50,97.5)",
                 b"not with -traces, -chains, repeated -m or -polyclass"):
        assert text in r.stderr, text


def test_library_refuses_bad_effects_arguments_without_a_handle():
    import ctypes as C
    from mmseq_amd import _lib
    lib = _lib.load()
    out = C.c_void_p()
    assert lib.mmg_diff_effects_open(None, 1, 1) == 1
    assert lib.mmg_diff_effects_open(None, 0, 1) == 1 and b"interval" in lib.mmg_last_error()
    assert lib.mmg_diff_effects_summarize(None, 0, None, C.byref(out)) == 1
    rows = (C.c_double * 4)(1.0, 0.0, 2.0, 1.0)
    model = (C.c_uint8 * 1)(0)
    pct = (C.c_double * 1)(50.0)
    bad = (C.c_double * 1)(100.5)
    # every argument check comes before the device is looked for: code 1 (argument), never 2 (no device)
    for S, P, F, r, m, np_, p in ((0, 2, 1, rows, model, 1, pct), (4097, 2, 1, rows, model, 1, pct), (2, 1, 1, rows, model, 1, pct),
                                  (2, 2, 1, None, model, 1, pct), (2, 2, 1, rows, None, 1, pct), (2, 2, 1, rows, model, 1, None),
                                  (2, 2, 1, rows, model, 1, bad), (2, 2, 1, rows, model, 33, pct), (2, 2, 0, rows, model, 1, pct)):
        assert lib.mmg_effects_of_rows(0, S, P, F, r, m, np_, p, C.byref(out)) == 1, (S, P, F, np_)
    half = (C.c_double * 4)(1.0, 0.0, 2.0, 0.5)
    assert lib.mmg_effects_of_rows(0, 2, 2, 1, half, model, 1, pct, C.byref(out)) == 1 and b"neither 0 nor 1" in lib.mmg_last_error()
    assert lib.mmg_effects_get(None, None, None, None, None, None) == 1
    assert lib.mmg_effects_device_bytes(None, None) == 1
    lib.mmg_effects_destroy(None)
