"""CPU checks of polytomous model selection in the mmdiff CLI: `-polyclass` against the numpy restatement (tests/mmdiff_poly_ref.py)
byte for byte, its closed forms, every error of -polyclass / -prior / -polyout / repeated -m before any device is touched, and a valid
repeated -m run that ends at the missing device."""
import os
import subprocess

import numpy as np
import pytest

import mmdiff_poly_ref as PR
from test_mmdiff_cli import samples, write_matrices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN_DIR = os.environ.get("MMSEQ_HOST_BIN_DIR") or os.path.join(ROOT, "mmseq_amd", "csrc")
MMDIFF = os.path.join(BIN_DIR, "mmdiff")
NODEV = dict(os.environ, HIP_VISIBLE_DEVICES="-1")


def run(args, env=NODEV):
    return subprocess.run([MMDIFF] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env)


def mmdiff_table(path, feats, bfs, comment=None, extra_cols=True):
    """A hand-written mmdiff table: bfs are written as text."""
    lines = ["#prior_probability=0.1"]
    hdr = ["feature_id", "bayes_factor", "posterior_probability"] + (["alpha0", "alpha1", "eta1_0"] if extra_cols else []) \
        + ["mu_a", "mu_b", "sd_a", "sd_b"]
    lines.append("\t".join(hdr))
    for i, (f, b) in enumerate(zip(feats, bfs)):
        if comment is not None and i == comment:
            lines.append("# a comment between rows")
        cells = [f, b, "0.5"] + (["1.5", "1.25", "-0.3"] if extra_cols else []) + ["%g" % (1 + i), "%g" % (2 + i), "0.1", "0.25"]
        lines.append("\t".join(cells))
    text = "\n".join(lines) + "\n"
    with open(path, "w") as fh:
        fh.write(text)
    return str(path), text


FEATS = ["f%d" % i for i in range(8)]
BF_A = ["1", "2.5", "0", "inf", "inf", "1e-300", "12345.6", "0"]
BF_B = ["1", "0.125", "3", "7", "inf", "1e+300", "0.000123", "0"]


def two_tables(tmp_path):
    a, ta = mmdiff_table(tmp_path / "a.mmdiff", FEATS, BF_A, comment=3)
    b, tb = mmdiff_table(tmp_path / "b.mmdiff", FEATS, BF_B, extra_cols=False)
    return [a, b], [ta, tb]


@pytest.mark.parametrize("prior", [None, [0.5, 0.25, 0.25], [0.7, 0.3, 0.0], [0.0, 0.5, 0.5]])
def test_polyclass_equals_the_restatement_j2(tmp_path, prior):
    """Flat and explicit priors, a zero entry, BF 0 (with prior (0, .5, .5) the last row's weights are all zero: NaN), one infinite BF,
    two infinite BFs in a row, a '#' comment line between rows."""
    files, texts = two_tables(tmp_path)
    args = ["-polyclass"] + ([] if prior is None else ["-prior", ",".join(repr(v) for v in prior)])
    r = run(args + files)
    assert r.returncode == 0, r.stderr
    want, warned = PR.polyclass(texts, prior)
    assert r.stdout.decode() == want
    assert (b"Warning: assuming flat prior across models" in r.stderr) == (prior is None)
    assert r.stderr.count(b"Warning: more than one infinite Bayes factor") == 1
    assert r.stderr.count(b"Warning:") == warned + (1 if prior is None else 0)
    rows = [ln.split("\t") for ln in r.stdout.decode().split("\n")[2:-1]]
    assert len(rows) == 8
    assert rows[3][-3:] == ["0", "1", "0"]                 # one infinite BF: that model 1, whatever its prior
    assert rows[4][-3:] == ["0", "nan", "nan"]             # two: those NaN, the others 0
    hdr = r.stdout.decode().split("\n")[1].split("\t")
    assert hdr == ["feature_id", "mu_a", "mu_b", "sd_a", "sd_b", "postprob_model0", "postprob_model1", "postprob_model2"]
    if prior == [0.0, 0.5, 0.5]:
        assert rows[7][-3:] == ["nan", "nan", "nan"]


def test_polyclass_equals_the_restatement_j5(tmp_path):
    rng = np.random.default_rng(3)
    feats = ["g%d" % i for i in range(40)]
    files, texts = [], []
    for j in range(5):
        bf = ["%g" % v for v in np.exp(rng.normal(0, 4, 40))]
        bf[j] = "inf"
        bf[7 + j] = "0"
        bf[20] = "nan" if j == 2 else bf[20]
        f, t = mmdiff_table(tmp_path / ("t%d.mmdiff" % j), feats, bf)
        files.append(f)
        texts.append(t)
    prior = [0.4, 0.1, 0.1, 0.2, 0.15, 0.05]
    r = run(["-polyclass", "-prior", ",".join(repr(v) for v in prior)] + files)
    assert r.returncode == 0, r.stderr
    want, warned = PR.polyclass(texts, prior)
    assert r.stdout.decode() == want and warned == 1
    assert r.stdout.decode().split("\n")[0] == "#prior_probabilities=0.4,0.1,0.1,0.2,0.15,0.05"
    assert b"Warning: NaN Bayes factor for feature 20 (g20)" in r.stderr


def test_all_bayes_factors_one_gives_the_prior(tmp_path):
    files = [mmdiff_table(tmp_path / ("t%d.mmdiff" % j), FEATS, ["1"] * 8)[0] for j in range(3)]
    prior = [0.125, 0.5, 0.25, 0.125]
    r = run(["-polyclass", "-prior", "0.125,0.5,0.25,0.125"] + files)
    assert r.returncode == 0, r.stderr
    for ln in r.stdout.decode().split("\n")[2:-1]:
        assert [float(v) for v in ln.split("\t")[-4:]] == prior


@pytest.mark.parametrize("p", [0.1, 0.5, 0.03])
def test_two_models_with_prior_1mp_p_0_is_recompute_pp(tmp_path, p):
    """J = 2 and prior (1 - p, p, 0): model 2 drops out and postprob_model1 is the two-model posterior, the reference's
    recompute_pp(bf, p), to 1e-12 relative.  The CLI prints 6 significant digits, so the identity is checked on the restatement's
    doubles (the CLI's text equals the restatement's in test_polyclass_equals_the_restatement_*), and the printed value to %g."""
    bfs = [0.001, 0.37, 1.0, 2.5, 1234.5, 1e12]
    a, ta = mmdiff_table(tmp_path / "a.mmdiff", FEATS[:6], ["%g" % v for v in bfs])
    b, tb = mmdiff_table(tmp_path / "b.mmdiff", FEATS[:6], ["%g" % v for v in reversed(bfs)])
    prior = [1.0 - p, p, 0.0]
    r = run(["-polyclass", "-prior", ",".join(repr(v) for v in prior), a, b])
    assert r.returncode == 0, r.stderr
    assert r.stdout.decode() == PR.polyclass([ta, tb], prior)[0]
    rows = r.stdout.decode().split("\n")[2:-1]
    for bf, ln in zip(bfs, rows):
        post, _ = PR.posteriors([1.0, bf, 7.0], prior)
        want = PR.recompute_pp(bf, p)
        assert abs(post[1] - want) <= 1e-12 * want
        assert post[2] == 0.0
        assert ln.split("\t")[-2] == "%g" % post[1]


def test_polyclass_errors_exit_1(tmp_path):
    files, _ = two_tables(tmp_path)
    c, _ = mmdiff_table(tmp_path / "c.mmdiff", FEATS[:4] + ["zz"] + FEATS[5:], BF_B)
    r = run(["-polyclass", files[0], c])
    assert r.returncode == 1 and b"Error: features across tables do not match (4,zz,f4)" in r.stderr and r.stdout == b""
    d, _ = mmdiff_table(tmp_path / "d.mmdiff", FEATS[:5], BF_B[:5])
    r = run(["-polyclass", files[0], d])
    assert r.returncode == 1 and b"Error: features across tables do not match (8 in" in r.stderr
    nob = tmp_path / "nobf.mmdiff"
    nob.write_text("feature_id\tposterior_probability\tmu_a\nf0\t0.5\t1\n")
    r = run(["-polyclass", files[0], str(nob)])
    assert r.returncode == 1 and b"must have feature_id and bayes_factor columns." in r.stderr
    r = run(["-polyclass", files[0]])
    assert r.returncode == 1 and b"Error: -polyclass needs at least two mmdiff tables." in r.stderr and b"Usage: mmdiff" in r.stderr
    r = run(["-polyclass", files[0], str(tmp_path / "missing.mmdiff")])
    assert r.returncode == 1 and b"Error: couldn't open" in r.stderr
    for bad in ["0.5,0.5", "0.5,0.25,0.125,0.125", "0.5,0.3,0.3", "0.5,0.25,0.2499", "0.5,x,0.5", "1.5,-0.25,-0.25", "nan,0.5,0.5"]:
        r = run(["-polyclass", "-prior", bad] + files)
        assert r.returncode == 1, bad
        assert b"Error: -prior must list 3 prior probabilities" in r.stderr and r.stdout == b""
    r = run(["-polyclass", "-prior", "0.5,0.25,0.250000001"] + files)      # within 1.5e-8 of 1
    assert r.returncode == 0
    for r in (run(["-polyclass", "-m", "x.mat"] + files), run(["-polyclass", "-de", "1", "1"] + files)):
        assert r.returncode == 1 and b"Error: -polyclass takes mmdiff tables" in r.stderr and b"no HIP device" not in r.stderr


MODEL0 = "1\n1\n1\n1\n\n"                       # M nil; then the class block, P0 = 1, P1
ALT_A = MODEL0 + "0 0\n0 0\n0 1\n0 1\n\n1\n\n0.5\n-0.5\n"
ALT_B = MODEL0 + "0 0\n0 1\n0 1\n0 1\n\n1\n\n0.5\n-0.5\n"
ALT_C = MODEL0 + "0 0\n0 0\n0 1\n0 2\n\n1\n\n1 0 0\n0 1 0\n0 0 1\n"


def alts(tmp_path, texts=(ALT_A, ALT_B, ALT_C)):
    return [write_matrices(tmp_path / ("alt%d.mat" % i), t) for i, t in enumerate(texts)]


def m_args(mats):
    return [a for m in mats for a in ("-m", m)]


def test_repeated_m_errors_come_before_the_device(tmp_path):
    files = samples(tmp_path, S=4, F=20)
    mats = alts(tmp_path)
    r = run(["-de", "2", "2"] + m_args(mats[:2]) + files)
    assert r.returncode == 1 and b"Error: -de cannot be combined with more than one -m." in r.stderr and b"Usage: mmdiff" in r.stderr
    r = run(m_args(mats[:2]) + ["-de", "2", "2"] + files)
    assert r.returncode == 1 and b"Error: -de cannot be combined with more than one -m." in r.stderr
    for opt in (["-prior", "0.5,0.5"], ["-polyout", str(tmp_path / "o")]):
        for mode in (["-de", "2", "2"], ["-m", mats[0]]):
            r = run(opt + mode + files)
            assert r.returncode == 1 and b"need" in r.stderr and b"more than one -m" in r.stderr and b"Usage: mmdiff" in r.stderr, r.stderr
    r = run(["-polyclass", "-polyout", "x", "a", "b"])
    assert r.returncode == 1 and b"Error: -polyout needs more than one -m." in r.stderr
    # model 0 differs: another M, another P0 value, another class column of model 0
    for other in ("1\n2\n3\n5\n\n0 0\n0 0\n0 1\n0 1\n\n1\n\n0.5\n-0.5\n", MODEL0 + "0 0\n0 0\n1 1\n1 1\n\n1\n2\n\n0.5\n-0.5\n"):
        bad = write_matrices(tmp_path / "bad.mat", other)
        r = run(m_args([mats[0], bad]) + files)
        assert r.returncode == 1 and ("Error: model 0 differs between %s and %s" % (mats[0], bad)).encode() in r.stderr, r.stderr
    # wrong prior count and sum
    for bad in ("0.5,0.5", "0.5,0.25,0.125,0.25"):
        r = run(["-prior", bad] + m_args(mats) + files)
        assert r.returncode == 1 and b"Error: -prior must list 4 prior probabilities" in r.stderr
    # a per-design check fails in the second file
    col = write_matrices(tmp_path / "col.mat", MODEL0 + "0 0\n0 0\n0 0\n0 0\n\n1\n\n1 1\n")
    r = run(m_args([mats[0], col]) + files)
    assert r.returncode == 1 and b"Error: collinearity in matrix P1" in r.stderr
    # J over the cap
    r = run(m_args([mats[0]] * 17) + files)
    assert r.returncode == 1 and b"Error: this mmdiff handles at most 16 alternative models (-m) in one run." in r.stderr
    # BASE that cannot be created
    r = run(["-polyout", str(tmp_path / "no_such_dir" / "base")] + m_args(mats) + files)
    assert r.returncode == 1 and b"Error: couldn't create" in r.stderr and b".model1.mmdiff" in r.stderr
    r = run(m_args(mats[:2]) + ["-p", "0.2"] + files)
    assert r.returncode == 1 and b"Error: optional arguments must be specified before -de or -m." in r.stderr


def test_no_error_path_reaches_a_device(tmp_path):
    """Every failing call above runs with HIP_VISIBLE_DEVICES=-1 and fails with its own message; here with the caller's environment."""
    files = samples(tmp_path, S=4, F=20)
    mats = alts(tmp_path)
    r = run(["-prior", "0.5,0.5"] + m_args(mats) + files, env=dict(os.environ))
    assert r.returncode == 1 and b"no HIP device" not in r.stderr and r.stdout == b""


def test_valid_repeated_m_passes_every_check_then_needs_a_device(tmp_path):
    files = samples(tmp_path, S=4, F=120)
    mats = alts(tmp_path)
    base = str(tmp_path / "out")
    r = run(["-prior", "0.4,0.3,0.2,0.1", "-polyout", base, "-burnin", "1024", "-iter", "1024", "-notune"] + m_args(mats) + files)
    assert r.returncode == 1 and r.stdout == b""
    assert b"Analysing 120 features" in r.stderr
    for j, m in enumerate(mats):
        assert ("Alternative %d (%s):" % (j + 1, m)).encode() in r.stderr
    assert r.stderr.count(b"Design matrix for model 1 ([1||P0]):") == 3
    assert r.stderr.rstrip().endswith(b"Error: no HIP device available: mmdiff has no CPU fallback")
    assert all(os.path.exists("%s.model%d.mmdiff" % (base, j)) for j in (1, 2, 3))    # creatable: checked before the device


def test_usage_lists_the_new_options():
    r = run(["-h"])
    for text in (b"-prior P0,...,PJ", b"-polyout STRING", b"-polyclass", b"-m alt1 -m alt2 [-m ...]", b"16 alternatives (-m) per run",
                 b"mmdiff -polyclass [-prior P0,...,PJ] a.mmdiff b.mmdiff [...] > out.polyclass"):
        assert text in r.stderr, text


def test_library_checks_poly_arguments_before_the_device():
    from mmseq_amd._lib import MMGError
    from mmseq_amd.diff import DiffPoly
    import mmdiff_ref as R
    M, P0, P1, C = R.de_design([3, 3])
    y, e = np.ones((4, 6)), np.full((4, 6), 0.1)
    with pytest.raises(MMGError) as ex:
        DiffPoly(y, e, M, P0, C[:, 0], [P1] * 17, [C[:, 1]] * 17)
    assert ex.value.code == 1 and "between 1 and 16" in str(ex.value)
    bad = C[:, 1].copy()
    bad[bad == 1] = 2
    with pytest.raises(MMGError) as ex:
        DiffPoly(y, e, M, P0, C[:, 0], [P1, P1], [C[:, 1], bad])
    assert ex.value.code == 1 and "without gaps" in str(ex.value)
