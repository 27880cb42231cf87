"""The stopping rule of mmseq -gibbs_auto (mmseq_amd/csrc/host/auto_rule.hpp) through its stand-alone driver auto_rule_test, against
the Python restatement tests/autolength_ref.py and against counts worked out by hand: NaNs, an empty judged set, f = 1, counts exactly
at ceil(f judged) and one below, a tail ESS below with a bulk ESS above the target, and rhat equal to the bound."""
import math
import os
import subprocess

import numpy as np
import pytest

import autolength_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN_DIR = os.environ.get("MMSEQ_HOST_BIN_DIR") or os.path.join(ROOT, "mmseq_amd", "csrc")
DRIVER = os.path.join(BIN_DIR, "auto_rule_test")
NAN = float("nan")


def drive(rows, ess, rhat, frac, tmp_path):
    path = tmp_path / "rule.txt"
    path.write_text("".join("%.17g %.17g %.17g\n" % tuple(r) for r in rows))
    r = subprocess.run([DRIVER, repr(ess), repr(rhat), repr(frac), str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 0, r.stderr
    f = r.stdout.split()
    return dict(judged=int(f[0]), passes=int(f[1]), needed=int(f[2]), min_ess=float(f[3]), max_rhat=float(f[4]), stop=f[5] == b"1")


def both(rows, ess, rhat, frac, tmp_path):
    got = drive(rows, ess, rhat, frac, tmp_path)
    a = np.array(rows, float).reshape(-1, 3)
    want = A.judge(a[:, 0], a[:, 1], a[:, 2], ess, rhat, frac)
    for k in want:
        same = got[k] == want[k] or (isinstance(want[k], float) and math.isnan(want[k]) and math.isnan(got[k]))
        assert same, (k, got, want)
    return got


GOOD, BAD = (1.001, 900.0, 800.0), (1.2, 50.0, 40.0)


def test_nans_are_not_judged(tmp_path):
    rows = [GOOD, (NAN, 900.0, 900.0), (1.0, NAN, 900.0), (1.0, 900.0, NAN), (NAN, NAN, NAN), BAD]
    v = both(rows, 400.0, 1.01, 0.5, tmp_path)
    assert (v["judged"], v["passes"], v["needed"], v["stop"]) == (2, 1, 1, True)
    assert v["min_ess"] == 40.0 and v["max_rhat"] == 1.2          # over the judged transcripts only


def test_nothing_judged_stops(tmp_path):
    v = both([(NAN, 1.0, 1.0), (1.0, NAN, 1.0)], 400.0, 1.01, 0.99, tmp_path)
    assert (v["judged"], v["passes"], v["needed"], v["stop"]) == (0, 0, 0, True)
    assert math.isnan(v["min_ess"]) and math.isnan(v["max_rhat"])
    v = both([], 400.0, 1.01, 1.0, tmp_path)
    assert (v["judged"], v["stop"]) == (0, True)


def test_fraction_one_needs_every_judged_transcript(tmp_path):
    v = both([GOOD] * 7 + [(NAN, 1.0, 1.0)], 400.0, 1.01, 1.0, tmp_path)
    assert (v["judged"], v["passes"], v["needed"], v["stop"]) == (7, 7, 7, True)
    v = both([GOOD] * 6 + [BAD], 400.0, 1.01, 1.0, tmp_path)
    assert (v["judged"], v["passes"], v["needed"], v["stop"]) == (7, 6, 7, False)


@pytest.mark.parametrize("judged,frac", [(200, 0.99), (101, 0.99), (10, 0.3), (7, 0.5), (1000, 0.999), (3, 1.0 / 3.0)])
def test_exactly_at_the_count_and_one_below(tmp_path, judged, frac):
    needed = int(math.ceil(frac * float(judged)))                # product and ceiling in double, as the rule is stated
    for passes, stop in ((needed, True), (needed - 1, False)):
        rows = [GOOD] * passes + [BAD] * (judged - passes)
        v = both(rows, 400.0, 1.01, frac, tmp_path)
        assert (v["judged"], v["passes"], v["needed"], v["stop"]) == (judged, passes, needed, stop)


def test_the_smaller_of_the_two_ess_counts(tmp_path):
    rows = [(1.0, 900.0, 399.999), (1.0, 399.999, 900.0), (1.0, 400.0, 400.0), (1.0, 900.0, 400.0)]
    v = both(rows, 400.0, 1.01, 1.0, tmp_path)
    assert (v["judged"], v["passes"], v["stop"]) == (4, 2, False)  # a tail ESS below the target fails whatever the bulk ESS; >= passes
    assert v["min_ess"] == 399.999


def test_rhat_equal_to_the_bound_passes(tmp_path):
    rows = [(1.01, 500.0, 500.0), (np.nextafter(1.01, 2.0), 500.0, 500.0), (0.999, 500.0, 500.0)]
    v = both(rows, 400.0, 1.01, 1.0, tmp_path)
    assert (v["judged"], v["passes"], v["stop"]) == (3, 2, False)
    assert v["max_rhat"] == np.nextafter(1.01, 2.0)


def test_infinite_ess_and_random_arrays(tmp_path):
    rng = np.random.default_rng(5)
    for frac in (0.5, 0.99, 1.0):
        r = 1.0 + rng.exponential(0.01, 300)
        eb, et = rng.uniform(100.0, 1200.0, 300), rng.uniform(100.0, 1200.0, 300)
        eb[::17] = np.inf
        r[::13] = NAN
        et[5::29] = NAN
        both(list(zip(r, eb, et)), 400.0, 1.01, frac, tmp_path)


def test_library_rule_equals_the_restatement():
    from mmseq_amd.autolength import judge
    rng = np.random.default_rng(6)
    r = 1.0 + rng.exponential(0.01, 500)
    eb, et = rng.uniform(100.0, 1200.0, 500), rng.uniform(100.0, 1200.0, 500)
    r[::11] = NAN
    for frac in (0.3, 0.99, 1.0):
        got, want = judge(r, eb, et, 400.0, 1.01, frac), A.judge(r, eb, et, 400.0, 1.01, frac)
        assert got == want
    assert judge([NAN], [1.0], [1.0])["stop"] and math.isnan(judge([NAN], [1.0], [1.0])["min_ess"])


def test_driver_refuses_bad_targets(tmp_path):
    p = tmp_path / "e.txt"
    p.write_text("")
    for args in (("0", "1.01", "0.99"), ("400", "1", "0.99"), ("400", "1.01", "0"), ("400", "1.01", "1.5"), ("nan", "1.01", "0.99")):
        r = subprocess.run([DRIVER, *args, str(p)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
        assert r.returncode == 2 and b"targets" in r.stderr
