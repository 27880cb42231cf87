"""CPU checks of `mmdiff -lrt FILE` / `-lrtonly` (run with HIP_VISIBLE_DEVICES=-1, as test_mmdiff_cli.run does): the usage text names
both flags, every refusal exits 1 with its message before any device is touched, an unwritable FILE is an error, and a valid
run passes every check and ends, loudly, at the missing device."""
import os

import pytest

from test_mmdiff_cli import run, samples, write_matrices
from test_mmdiff_poly_cli import ALT_A, ALT_B

FAST = ["-burnin", "1024", "-iter", "1024", "-notune"]
REFUSAL = b"Error: -lrt and -lrtonly cannot be combined with -chains, more than one -m, -permutations or -polyclass."
NO_DEVICE = b"Error: no HIP device available: mmdiff has no CPU fallback"


def test_usage_names_both_flags():
    r = run(["-h"])
    for text in (b"-lrt STRING", b"-lrtonly", b"loglik0, loglik1, lrt_stat, df, p_value", b"q_value (Benjamini-",
                 b"not with -chains, repeated -m, -permutations or -polyclass", b"skip the MCMC and leave stdout empty"):
        assert text in r.stderr, text


def test_lrtonly_needs_lrt(tmp_path):
    files = samples(tmp_path, S=4, F=20)
    r = run(["-lrtonly", "-de", "2", "2"] + files)
    assert r.returncode == 1 and b"Error: -lrtonly needs -lrt." in r.stderr and b"Usage: mmdiff" in r.stderr, r.stderr
    assert NO_DEVICE not in r.stderr and r.stdout == b""


@pytest.mark.parametrize("only", [[], ["-lrtonly"]], ids=["lrt", "lrtonly"])
@pytest.mark.parametrize("extra", [["-chains", "2"], ["-chains", "1"], ["-permutations", "2"]], ids=["chains", "chains1", "permutations"])
def test_combinations_out_of_scope_are_refused_before_the_device(tmp_path, extra, only):
    files = samples(tmp_path, S=4, F=20)
    out = str(tmp_path / "out.lrt")
    for args in (["-lrt", out] + only + extra, extra + only + ["-lrt", out]):
        r = run(FAST + args + ["-de", "2", "2"] + files)
        assert r.returncode == 1 and REFUSAL in r.stderr and b"Usage: mmdiff" in r.stderr, r.stderr
        assert NO_DEVICE not in r.stderr and r.stdout == b""
    assert not os.path.exists(out)


def test_repeated_m_and_polyclass_are_refused(tmp_path):
    files = samples(tmp_path, S=4, F=20)
    out = str(tmp_path / "out.lrt")
    a, b = write_matrices(tmp_path / "a.mat", ALT_A), write_matrices(tmp_path / "b.mat", ALT_B)
    r = run(["-lrt", out, "-m", a, "-m", b] + files)
    assert r.returncode == 1 and REFUSAL in r.stderr and b"Usage: mmdiff" in r.stderr and NO_DEVICE not in r.stderr and r.stdout == b""
    r = run(["-polyclass", "-lrt", out, "x.mmdiff", "y.mmdiff"])
    assert r.returncode == 1 and REFUSAL in r.stderr and b"Usage: mmdiff" in r.stderr
    assert not os.path.exists(out)


def test_options_go_before_the_design_and_need_their_value(tmp_path):
    files = samples(tmp_path, S=4, F=20)
    r = run(["-de", "2", "2", "-lrt", str(tmp_path / "o")] + files)
    assert r.returncode == 1 and b"Error: optional arguments must be specified before -de or -m." in r.stderr
    r = run(["-de", "2", "2", "-lrtonly"] + files)
    assert r.returncode == 1 and b"Error: optional arguments must be specified before -de or -m." in r.stderr
    r = run(["-lrt"])
    assert r.returncode == 1 and b"Error: mandatory arguments missing." in r.stderr
    r = run(["-lrt", "", "-de", "2", "2"] + files)
    assert r.returncode == 1 and b"Error: -lrt needs a file name." in r.stderr


@pytest.mark.parametrize("only", [[], ["-lrtonly"]], ids=["lrt", "lrtonly"])
def test_unwritable_file_is_an_error_before_the_device(tmp_path, only):
    files = samples(tmp_path, S=4, F=120)
    out = str(tmp_path / "no_such_dir" / "out.lrt")
    r = run(FAST + ["-lrt", out] + only + ["-de", "2", "2"] + files)
    assert r.returncode == 1 and b"Error: couldn't create " + out.encode() in r.stderr, r.stderr
    assert NO_DEVICE not in r.stderr and r.stdout == b""


@pytest.mark.parametrize("extra", [[], ["-lrtonly"], ["-fixalpha", "-nonorm", "-permute", "-range", "3", "40"]], ids=["plain", "lrtonly", "options"])
def test_valid_run_fails_loudly_without_a_device(tmp_path, extra):
    files = samples(tmp_path, S=4, F=120)
    out = str(tmp_path / "out.lrt")
    r = run(FAST + ["-lrt", out] + extra + ["-de", "2", "2"] + files)
    assert r.returncode == 1 and r.stdout == b""
    assert b"Design matrix for model 1" in r.stderr
    assert r.stderr.rstrip().endswith(NO_DEVICE)
    assert os.path.exists(out) and os.path.getsize(out) == 0      # opened before the device was looked for, nothing computed


def test_library_refuses_what_mmg_diff_create_refuses_with_the_same_message():
    """mmg_diff_lrt_create checks its arguments as mmg_diff_create does, before any device work: the same code and message."""
    import numpy as np
    from mmseq_amd._lib import MMGError
    from mmseq_amd.diff import Diff, DiffLrt

    def design(N=6, K=1, L1=1, classes=None):
        C = np.zeros((N, 2), np.int32) if classes is None else np.array(classes, np.int32)
        return np.zeros((N, K)), np.ones((N, 1)), np.ones((N, L1)), C

    y, e = np.ones((3, 6)), np.full((3, 6), 0.1)
    bad_y = y.copy()
    bad_y[1, 2] = np.nan
    bad_M = design()
    bad_M[0][3, 0] = np.inf
    cases = {
        "the number of samples must be between 2 and 512": (np.ones((3, 1)), np.ones((3, 1))) + design(N=1),
        "M must have between 1 and 8 columns": (y, e) + design(K=9),
        "P0 and P1 must have between 1 and 16 columns": (y, e) + design(L1=17),
        "y and e must be finite": (bad_y, e) + design(),
        "M, P0 and P1 must be finite": (y, e) + bad_M,
        "class labels must be between 0 and 15": (y, e) + design(classes=[[0, 16]] * 6),
        "the class labels of each model must be 0, 1, ..., n - 1 without gaps": (y, e) + design(classes=[[0, 0]] * 3 + [[0, 2]] * 3),
    }
    for message, args in cases.items():
        errors = []
        for cls in (Diff, DiffLrt):
            with pytest.raises(MMGError) as err:
                cls(*args, device=99)                 # (a device that does not exist: the refusal comes first)
            errors.append(err.value)
        assert errors[0].code == errors[1].code == 1 and str(errors[0]) == str(errors[1]) and message in str(errors[1]), message
