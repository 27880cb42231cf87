"""CPU checks of `mmdiff -lrt FILE -lrtperm B` (run with HIP_VISIBLE_DEVICES=-1, as test_mmdiff_cli.run does): the usage text names
the flag and repeats the known limit of a shuffled null, every refusal exits 1 with its message and the usage text before any device
is touched, an unwritable FILE is still an error, a valid run ends, loudly, at the missing device, and the library refuses the
new arguments before any device work."""
import os

import numpy as np
import pytest

from test_mmdiff_cli import run, samples
from test_mmdiff_lrt_cli import FAST, NO_DEVICE, REFUSAL


def test_usage_names_the_flag_and_the_limit():
    r = run(["-h"])
    for text in (b"-lrtperm INT", b"perm_ge", b"perm_p", b"null_ge", b"q_perm", b"1 to 65535", b"not with -permute",
                 b"With few samples many shuffles", b"reproduce the original grouping, and this null is conservative too",
                 # the sentences that were there stay
                 b"-lrt STRING", b"not with -chains, repeated -m, -permutations or -polyclass", b"skip the MCMC and leave stdout empty",
                 b"shuffles reproduce the original grouping (a third of them for 2 vs 2), and the q-values are conservative"):
        assert text in r.stderr, text


def refused(r, message):
    assert r.returncode == 1 and message in r.stderr and b"Usage: mmdiff" in r.stderr, r.stderr
    assert NO_DEVICE not in r.stderr and r.stdout == b""


@pytest.mark.parametrize("only", [[], ["-lrtonly"]], ids=["lrt", "lrtonly"])
def test_lrtperm_needs_lrt(tmp_path, only):
    files = samples(tmp_path, S=4, F=20)
    r = run(FAST + ["-lrtperm", "3"] + only + ["-de", "2", "2"] + files)
    refused(r, b"Error: -lrtonly needs -lrt." if only else b"Error: -lrtperm needs -lrt.")


@pytest.mark.parametrize("B", ["0", "65536", "-1", "3.5", "x", "", "99999999999999999999"])
def test_the_number_of_copies_is_an_integer_between_1_and_65535(tmp_path, B):
    files = samples(tmp_path, S=4, F=20)
    out = str(tmp_path / "out.lrt")
    r = run(FAST + ["-lrt", out, "-lrtperm", B, "-de", "2", "2"] + files)
    refused(r, b"Error: -lrtperm takes an integer between 1 and 65535.")
    assert not os.path.exists(out)


def test_lrtperm_with_permute_is_refused_in_either_order(tmp_path):
    files = samples(tmp_path, S=4, F=20)
    out = str(tmp_path / "out.lrt")
    for args in (["-permute", "-lrt", out, "-lrtperm", "3"], ["-lrtperm", "3", "-lrt", out, "-lrtonly", "-permute"]):
        refused(run(FAST + args + ["-de", "2", "2"] + files), b"Error: -lrtperm cannot be combined with -permute.")
    assert not os.path.exists(out)


@pytest.mark.parametrize("extra", [["-chains", "2"], ["-permutations", "2"]], ids=["chains", "permutations"])
def test_the_refusals_of_lrt_stay_word_for_word(tmp_path, extra):
    files = samples(tmp_path, S=4, F=20)
    r = run(FAST + ["-lrt", str(tmp_path / "out.lrt"), "-lrtperm", "3"] + extra + ["-de", "2", "2"] + files)
    refused(r, REFUSAL)


def test_the_flag_goes_before_the_design_and_needs_its_value(tmp_path):
    files = samples(tmp_path, S=4, F=20)
    r = run(["-lrt", str(tmp_path / "o"), "-de", "2", "2", "-lrtperm", "3"] + files)
    assert r.returncode == 1 and b"Error: optional arguments must be specified before -de or -m." in r.stderr
    r = run(["-lrtperm"])
    assert r.returncode == 1 and b"Error: mandatory arguments missing." in r.stderr


@pytest.mark.parametrize("only", [[], ["-lrtonly"]], ids=["lrt", "lrtonly"])
def test_unwritable_file_is_still_an_error_before_the_device(tmp_path, only):
    files = samples(tmp_path, S=4, F=120)
    out = str(tmp_path / "no_such_dir" / "out.lrt")
    r = run(FAST + ["-lrt", out, "-lrtperm", "5"] + only + ["-de", "2", "2"] + files)
    assert r.returncode == 1 and b"Error: couldn't create " + out.encode() in r.stderr, r.stderr
    assert NO_DEVICE not in r.stderr and r.stdout == b""


@pytest.mark.parametrize("extra", [[], ["-lrtonly"], ["-fixalpha", "-nonorm", "-seed", "9", "-range", "3", "40"]], ids=["plain", "lrtonly", "options"])
@pytest.mark.parametrize("B", ["1", "65535"])
def test_valid_run_fails_loudly_without_a_device(tmp_path, extra, B):
    files = samples(tmp_path, S=4, F=120)
    out = str(tmp_path / "out.lrt")
    r = run(FAST + ["-lrt", out, "-lrtperm", B] + extra + ["-de", "2", "2"] + files)
    assert r.returncode == 1 and r.stdout == b""
    assert b"Design matrix for model 1" in r.stderr
    assert r.stderr.rstrip().endswith(NO_DEVICE)
    assert os.path.exists(out) and os.path.getsize(out) == 0


def test_library_refuses_its_arguments_before_any_device_work():
    """The new cases, and those of mmg_diff_lrt_create with the same code and message, on a device that does not exist."""
    from mmseq_amd._lib import MMGError
    from mmseq_amd.diff import DiffLrt, DiffLrtPerm

    y, e = np.ones((3, 6)), np.full((3, 6), 0.1)
    design = (np.zeros((6, 1)), np.ones((6, 1)), np.ones((6, 1)), np.zeros((6, 2), np.int32))
    for B in (0, 65536):
        with pytest.raises(MMGError) as err:
            DiffLrtPerm(y, e, *design, B, device=99)
        assert err.value.code == 1 and "the number of permutations must be between 1 and 65535" in str(err.value)
    big = np.ones((32768, 2))                                  # 65535 x 32768 = 2^31 - 32768 fits, 65535 x 32769 does not
    two = (np.zeros((2, 1)), np.ones((2, 1)), np.ones((2, 1)), np.zeros((2, 2), np.int32))
    with pytest.raises(MMGError) as err:
        DiffLrtPerm(np.ones((32769, 2)), np.ones((32769, 2)), *two, 65535, device=99)
    assert err.value.code == 1 and "times the number of features must be at most 2147483647" in str(err.value)
    with pytest.raises(MMGError) as err:
        DiffLrtPerm(big, big, *two, 65535, device=99)
    assert err.value.code != 1                                 # past the argument checks: the device is what is missing
    bad_y = y.copy()
    bad_y[1, 2] = np.nan
    cases = {
        "the number of samples must be between 2 and 512": (np.ones((3, 1)), np.ones((3, 1)), np.zeros((1, 1)), np.ones((1, 1)), np.ones((1, 1)),
                                                            np.zeros((1, 2), np.int32)),
        "M must have between 1 and 8 columns": (y, e, np.zeros((6, 9))) + design[1:],
        "y and e must be finite": (bad_y, e) + design,
        "class labels must be between 0 and 15": (y, e) + design[:3] + (np.array([[0, 16]] * 6, np.int32),),
    }
    for message, args in cases.items():
        errors = []
        for make in (lambda: DiffLrt(*args, device=99), lambda: DiffLrtPerm(*args, 3, device=99)):
            with pytest.raises(MMGError) as err:
                make()
            errors.append(err.value)
        assert errors[0].code == errors[1].code == 1 and str(errors[0]) == str(errors[1]) and message in str(errors[1]), message
