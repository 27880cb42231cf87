"""CPU checks of `mmdiff -permutations`: the usage text names both flags and the known limit, every refusal exits 1 with its message
before any device is touched, and a valid run passes every check and ends at the missing device."""
import os

import pytest

from test_mmdiff_cli import run, samples, write_matrices
from test_mmdiff_poly_cli import ALT_A, ALT_B

FAST = ["-burnin", "1024", "-iter", "1024", "-notune"]
REFUSAL = b"Error: -permutations cannot be combined with -permute, -chains above 1 (or -chainout), more than one -m, -traces, -effects or -polyclass."


def test_usage_lists_the_new_options_and_the_limit():
    r = run(["-h"])
    for text in (b"-permutations INT", b"-permout STRING", b"STRING.perm<b>.mmdiff", b"-permutations B [-permout BASE]", b"perm_ge", b"q_value",
                 b"a third of them for 2 vs 2", b"conservative", b"At most 31 permutations."):
        assert text in r.stderr, text


@pytest.mark.parametrize("value", ["0", "32", "-1", "2.5", "x", "3x", ""])
def test_permutations_value_must_be_an_integer_from_1_to_31(tmp_path, value):
    files = samples(tmp_path, S=4, F=20)
    r = run(["-permutations", value, "-de", "2", "2"] + files)
    assert r.returncode == 1 and b"Error: -permutations takes an integer between 1 and 31." in r.stderr, r.stderr
    assert b"no HIP device" not in r.stderr and r.stdout == b""


@pytest.mark.parametrize("extra", [["-permute"], ["-chains", "2"], ["-chains", "1", "-chainout", "BASE"], ["-traces", "DIR"], ["-effects", "FILE"]],
                         ids=["permute", "chains", "chainout", "traces", "effects"])
def test_combinations_out_of_scope_are_refused_before_the_device(tmp_path, extra):
    files = samples(tmp_path, S=4, F=20)
    extra = [str(tmp_path / a) if a in ("BASE", "DIR", "FILE") else a for a in extra]
    for args in (["-permutations", "2"] + extra, extra + ["-permutations", "2"]):
        r = run(FAST + args + ["-de", "2", "2"] + files)
        assert r.returncode == 1 and REFUSAL in r.stderr and b"Usage: mmdiff" in r.stderr, r.stderr
        assert b"no HIP device" not in r.stderr and r.stdout == b""
    assert not os.path.exists(str(tmp_path / "DIR"))


def test_more_refusals_come_before_the_device(tmp_path):
    files = samples(tmp_path, S=4, F=20)
    a, b = write_matrices(tmp_path / "a.mat", ALT_A), write_matrices(tmp_path / "b.mat", ALT_B)
    r = run(["-permutations", "2", "-m", a, "-m", b] + files)
    assert r.returncode == 1 and REFUSAL in r.stderr and b"no HIP device" not in r.stderr and r.stdout == b""
    r = run(["-polyclass", "-permutations", "2", "x.mmdiff", "y.mmdiff"])
    assert r.returncode == 1 and REFUSAL in r.stderr
    r = run(["-permout", str(tmp_path / "o"), "-de", "2", "2"] + files)
    assert r.returncode == 1 and b"Error: -permout needs -permutations." in r.stderr and b"Usage: mmdiff" in r.stderr
    r = run(["-permutations"])
    assert r.returncode == 1 and b"Error: mandatory arguments missing." in r.stderr
    r = run(FAST + ["-permutations", "2", "-permout", str(tmp_path / "no_such_dir" / "base"), "-de", "2", "2"] + files)
    assert r.returncode == 1 and b"Error: couldn't create" in r.stderr and b".perm1.mmdiff" in r.stderr, r.stderr
    assert b"no HIP device" not in r.stderr and r.stdout == b""
    r = run(["-de", "2", "2", "-permutations", "2"] + files)
    assert r.returncode == 1 and b"Error: optional arguments must be specified before -de or -m." in r.stderr


def test_no_refusal_reaches_a_device(tmp_path):
    """The refusals above run with HIP_VISIBLE_DEVICES=-1; here with the caller's environment."""
    files = samples(tmp_path, S=4, F=20)
    r = run(["-permutations", "32", "-de", "2", "2"] + files, env=dict(os.environ))
    assert r.returncode == 1 and b"no HIP device" not in r.stderr and r.stdout == b""
    r = run(["-permutations", "2", "-permute", "-de", "2", "2"] + files, env=dict(os.environ))
    assert r.returncode == 1 and b"no HIP device" not in r.stderr and r.stdout == b""


@pytest.mark.parametrize("extra", [[], ["-fixalpha", "-nonorm", "-p", "0.2", "-range", "3", "40"]], ids=["plain", "options"])
def test_valid_run_passes_every_check_then_needs_a_device(tmp_path, extra):
    files = samples(tmp_path, S=4, F=120)
    base = str(tmp_path / "out")
    r = run(FAST + extra + ["-permutations", "3", "-permout", base, "-de", "2", "2"] + files)
    assert r.returncode == 1 and r.stdout == b""
    assert b"Design matrix for model 1" in r.stderr and b"Permuting input data" not in r.stderr
    assert r.stderr.rstrip().endswith(b"Error: no HIP device available: mmdiff has no CPU fallback")
    assert all(os.path.exists("%s.perm%d.mmdiff" % (base, b)) for b in (1, 2, 3)) and not os.path.exists(base + ".perm0.mmdiff")
