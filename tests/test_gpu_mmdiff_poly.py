"""Polytomous mmdiff on the device: a repeated -m run against separate single -m runs of the same binary (byte for byte), against the
numpy restatement (tests/mmdiff_ref.py), its combined table against -polyclass and tests/mmdiff_poly_ref.py; the mmg_diff_poly_*
entries through DiffPoly against separate Diff handles (bitwise), memory, reruns, edges, planted structure and a 200 000-feature run."""
import os
import re
import subprocess

import numpy as np
import pytest

import mmdiff_poly_ref as PR
import mmdiff_ref as R
from test_gpu_mmdiff import MMDIFF, write_tables

GROUPS = [3, 3, 2]
S = 8
# classes under each alternative to "all groups equal": A != B = C, A = B != C, all differ (the shape of the reference's doc/332.mat)
CLASSES1 = [np.array([0, 0, 0, 1, 1, 1, 1, 1]), np.array([0, 0, 0, 0, 0, 0, 1, 1]), np.array([0, 0, 0, 1, 1, 1, 2, 2])]
# rows of P1 per class: one contrast column, two and three indicator columns (L1 = 1, 2, 3; 2, 2, 3 classes)
P1ROWS = [np.array([[0.5], [-0.5]]), np.eye(2), np.eye(3)]
TUNE_SEED = 201     # the restatement tunes its three comparisons in 21, 17 and more than 40 batches


def design(j, M=None, classes1=CLASSES1, p1rows=P1ROWS):
    c1 = classes1[j]
    n = len(c1)
    M = np.zeros((n, 1)) if M is None else M
    return M, np.ones((n, 1)), p1rows[j][c1], np.stack([np.zeros(n, np.int64), c1], 1)


def write_mat(path, M, C, p1rows):
    txt = "".join(" ".join(repr(float(v)) for v in row) + "\n" for row in M) + "\n"
    txt += "".join("%d %d\n" % tuple(c) for c in C) + "\n1\n\n"
    txt += "".join(" ".join(repr(float(v)) for v in row) + "\n" for row in p1rows)
    with open(path, "w") as f:
        f.write(txt)
    return str(path)


def write_alternatives(tmp_path, M=None, classes1=CLASSES1, p1rows=P1ROWS):
    mats = []
    for j in range(len(classes1)):
        Mj, _, _, C = design(j, M, classes1, p1rows)
        mats.append(write_mat(tmp_path / ("alt%d.mat" % (j + 1)), Mj, C, p1rows[j]))
    return mats


def synth(F, seed, n_samples=S, effect=1.5):
    rng = np.random.default_rng(seed)
    y = rng.normal(2, 1, (F, 1)) + rng.normal(0, 0.3, (F, n_samples))
    y[: F // 5, :3] += effect
    return y, rng.uniform(0.05, 0.5, (F, n_samples)), rng.integers(1, 5, (F, n_samples))


def cli(args, timeout=300):
    r = subprocess.run([MMDIFF] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=timeout)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout.decode(), r.stderr.decode()


def m_args(mats):
    return [a for m in mats for a in ("-m", m)]


def read(path):
    with open(path) as f:
        return f.read()


def poly_and_separate(tmp_path, opts, mats, files, prior=None, timeout=300):
    """The polytomous run with -polyout and one single -m run per alternative; asserts the contract and returns (stdout, stderr,
    tables, stderrs of the single runs)."""
    base = str(tmp_path / "poly")
    pr = [] if prior is None else ["-prior", ",".join(repr(v) for v in prior)]
    out, err = cli(opts + pr + ["-polyout", base] + m_args(mats) + files, timeout)
    tables, errs = [], []
    for j, m in enumerate(mats):
        single, serr = cli(opts + ["-m", m] + files, timeout)
        got = read("%s.model%d.mmdiff" % (base, j + 1))
        assert got == single, "table of alternative %d differs from the single -m run" % (j + 1)
        tables.append(got)
        errs.append(serr)
    # the combined table: -polyclass on the written tables, and the numpy restatement
    again, _ = cli(["-polyclass"] + pr + ["%s.model%d.mmdiff" % (base, j + 1) for j in range(len(mats))])
    assert out == again
    assert out == PR.polyclass(tables, prior)[0]
    return out, err, tables, errs


FAST = ["-burnin", "1024", "-iter", "1024", "-notune"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["plain", "permute", "fixalpha", "covariate"])
def test_notune_tables_equal_separate_runs(gpu, tmp_path, case):
    y, e, uh = synth(120, {"plain": 301, "permute": 302, "fixalpha": 303, "covariate": 304}[case])
    files = write_tables(tmp_path, y, e, uh)
    M = np.array([[0.3], [1.1], [-0.4], [0.9], [0.0], [-1.2], [0.6], [-0.7]]) if case == "covariate" else None
    mats = write_alternatives(tmp_path, M)
    opts = {"plain": [], "permute": ["-permute", "-seed", "77"], "fixalpha": ["-fixalpha"], "covariate": []}[case] + FAST
    prior = [0.4, 0.3, 0.2, 0.1] if case == "plain" else None
    out, err, tables, _ = poly_and_separate(tmp_path, opts, mats, files, prior)
    for j in (1, 2, 3):
        assert "model %d: sampling after 0 tuning batches" % j in err
    hdrs = [t.split("\n")[1] for t in tables]
    assert "eta1_1\t" in hdrs[1] and "eta1_2\t" in hdrs[2] and "eta1_1" not in hdrs[0]        # L1 varies between the alternatives
    assert ("beta0_0\t" in hdrs[0]) == (case == "covariate")
    assert out.split("\n")[1].split("\t")[-4:] == ["postprob_model%d" % j for j in range(4)]
    if case == "plain":
        # one comparison against the independent restatement as well
        want = R.mmdiff(files, design=design(1), burnin=1024, iters=1024, tune=False)
        assert tables[1] == want


@pytest.mark.gpu
def test_default_tuning_each_comparison_stops_at_its_own_batch(gpu, tmp_path):
    """Fewer than 100 features, so no normalisation, as in test_gpu_mmdiff's tuning test.  The restatement (run on a CPU when this
    fixture was chosen) tunes the three comparisons of this seed in different numbers of batches; the test asserts that from the run
    itself, since otherwise the per-comparison stream index is not exercised."""
    y, e, uh = synth(6, TUNE_SEED)
    files = write_tables(tmp_path, y, e, uh)
    mats = write_alternatives(tmp_path)
    out, err, tables, errs = poly_and_separate(tmp_path, ["-burnin", "1024", "-iter", "1024"], mats, files)
    nb = [int(n) for n in re.findall(r"model \d+: sampling after (\d+) tuning batches", err)]
    print("tuning batches per comparison:", nb)
    assert len(nb) == 3 and len(set(nb)) >= 2, nb
    for j in range(3):
        assert "sampling after %d tuning batches" % nb[j] in errs[j]


def drive(h, burnin, max_batches, iters):
    h.burnin(burnin)
    nb = h.tune(max_batches) if max_batches else 0
    h.sample(iters)
    return nb


@pytest.mark.gpu
def test_diffpoly_is_bitwise_j_separate_diff_handles(gpu):
    """Results, logit p' and batch counts of every comparison against separate Diff handles driven the same way (tune until the
    untuned count is 0 or 48 batches); device memory against the documented formula and against the separate handles; a rerun."""
    from mmseq_amd.diff import Diff, DiffPoly
    y, e, _ = synth(6, TUNE_SEED)
    y = np.concatenate([y, synth(58, 12)[0]])
    e = np.concatenate([e, synth(58, 12)[1]])
    ds = [design(j) for j in range(3)]
    M, P0 = ds[0][0], ds[0][1]

    def poly():
        h = DiffPoly(y, e, M, P0, np.zeros(S, int), [d[2] for d in ds], [d[3][:, 1] for d in ds], seed=42)
        nb = drive(h, 1024, 48, 1024)
        res = [h.results(j) for j in range(3)]
        info = [h.info(j) for j in range(3)]
        nbytes = h.device_bytes()
        h.close()
        return nb, res, info, nbytes

    nb, res, info, nbytes = poly()
    print("batches per comparison:", nb)
    single_bytes = 0
    for j, (Mj, P0j, P1j, Cj) in enumerate(ds):
        d = Diff(y, e, Mj, P0j, P1j, Cj, seed=42)
        want_nb = drive(d, 1024, 48, 1024)
        want = d.results()
        assert nb[j] == want_nb and info[j]["batches"] == d.info()["batches"] == want_nb
        assert info[j]["n_classes"] == d.info()["n_classes"] and info[j]["Pnil"] == d.info()["Pnil"]
        for k in want:
            assert np.array_equal(res[j][k], want[k], equal_nan=True), (j, k)
        single_bytes += d.device_bytes()
        assert d.device_bytes() == PR.single_device_bytes(64, S, 1, 1, P1j.shape[1], 1, int(Cj[:, 1].max()) + 1, True)
        d.close()
    assert nbytes == PR.poly_device_bytes(64, S, 1, 1, 1, True, [(d[2].shape[1], int(d[3][:, 1].max()) + 1) for d in ds])
    assert nbytes < single_bytes
    nb2, res2, _, _ = poly()
    assert nb2 == nb
    for j in range(3):
        for k in res[j]:
            assert np.array_equal(res[j][k], res2[j][k], equal_nan=True)


@pytest.mark.gpu
def test_one_comparison_ends_tuning_many_batches_before_another(gpu):
    """The six features of the tuning fixture, tuned to the stop rule (limit 1024): the second comparison ends more than a hundred
    batches before the third (17 and 197 batches when the fixture was chosen), so the third runs on alone for most of its tuning and
    the others start sampling at much smaller stream indices.  All equal their separate Diff handles."""
    from mmseq_amd.diff import Diff, DiffPoly
    y, e, _ = synth(6, TUNE_SEED)
    ds = [design(j) for j in range(3)]
    h = DiffPoly(y, e, ds[0][0], ds[0][1], np.zeros(S, int), [d[2] for d in ds], [d[3][:, 1] for d in ds])
    nb = drive(h, 1024, 1024, 1024)
    print("batches per comparison:", nb)
    assert max(nb) - min(nb) >= 100 and max(nb) < 1024, nb
    assert all(h.info(j)["ended"] for j in range(3))
    for j in range(3):
        d = Diff(y, e, *ds[j])
        assert drive(d, 1024, 1024, 1024) == nb[j]
        want, got = d.results(), h.results(j)
        for k in want:
            assert np.array_equal(got[k], want[k], equal_nan=True), (j, k)
        d.close()
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F", [1, 65])
def test_edges_one_feature_one_lane_past_a_block_j_at_the_cap_and_a_nil_p1(gpu, F):
    """16 comparisons (the cap): the three alternatives in turn, and one whose P1 is a constant column (nil: no etas in model 1, only
    the variance classes differ).  Every one equals its separate Diff handle after burn-in, two tuning batches and sampling."""
    from mmseq_amd.diff import Diff, DiffPoly
    y, e, _ = synth(max(F, 5), 400 + F)
    y, e = y[:F], e[:F]
    ds = [design(j % 3) for j in range(15)]
    ds.append((ds[0][0], ds[0][1], np.ones((S, 1)), ds[0][3]))
    h = DiffPoly(y, e, ds[0][0], ds[0][1], np.zeros(S, int), [d[2] for d in ds], [d[3][:, 1] for d in ds], seed=9)
    # (P0, the single constant column of "all groups equal", is nil as well, as in -de)
    assert h.J == 16 and h.info(15)["Pnil"] == (True, True) and h.info(14)["Pnil"] == (True, False)
    h.burnin(1024)
    counts = [h.tune_batch()[0] for _ in range(2)]
    h.sample(256)
    for j in (0, 1, 2, 7, 15):
        d = Diff(y, e, *ds[j], seed=9)
        d.burnin(1024)
        want_counts = [d.tune_batch() for _ in range(2)]
        assert [c[j] for c in counts] == want_counts
        d.sample(256)
        want, got = d.results(), h.results(j)
        for k in want:
            assert np.array_equal(got[k], want[k], equal_nan=True), (j, k)
        d.close()
    for j in range(3, 15):                      # the same alternative again: the same chain
        for k, v in h.results(j % 3).items():
            assert np.array_equal(h.results(j)[k], v, equal_nan=True)
    h.close()


@pytest.mark.gpu
def test_planted_structure_orders_the_posteriors(gpu, tmp_path):
    """50 features planted under each alternative and under the null; for each kind the mean posterior of the true model over its
    features is larger than the mean posterior of every other model over them (an ordering: no threshold).  Flat prior.  -nonorm:
    three quarters of these features carry a group effect, so the median-based normalisation factors would move whole groups."""
    F, per = 200, 50
    rng = np.random.default_rng(21)
    y = rng.normal(2, 1, (F, 1)) + rng.normal(0, 0.3, (F, S))
    y[per:2 * per, :3] += 3.0                       # A != B = C
    y[2 * per:3 * per, 6:] += 3.0                   # A = B != C
    y[3 * per:, :3] += 3.0                          # all differ
    y[3 * per:, 6:] -= 3.0
    e = rng.uniform(0.05, 0.5, (F, S))
    files = write_tables(tmp_path, y, e, rng.integers(1, 5, (F, S)))
    mats = write_alternatives(tmp_path)
    out, err = cli(["-nonorm", "-burnin", "1024", "-iter", "2048"] + m_args(mats) + files, timeout=900)
    assert "Warning: assuming flat prior across models" in err
    rows = [ln.split("\t") for ln in out.split("\n")[2:-1]]
    assert len(rows) == F
    post = np.array([[float(v) for v in r[-4:]] for r in rows])
    for kind in range(4):
        means = post[kind * per:(kind + 1) * per].mean(0)
        print("planted model %d: mean posteriors of models 0..3 =" % kind, means)
    for kind in range(4):
        means = post[kind * per:(kind + 1) * per].mean(0)
        assert all(means[kind] > means[o] for o in range(4) if o != kind), (kind, means)


@pytest.mark.gpu
def test_200000_features_four_alternatives(gpu, tmp_path):
    from mmseq_amd.diff import DiffPoly
    F, n = 200000, 6
    rng = np.random.default_rng(1)
    y = rng.normal(2, 1, (F, 1)) + rng.normal(0, 0.3, (F, n))
    e = rng.uniform(0.05, 0.5, (F, n))
    files = write_tables(tmp_path, y, e, rng.integers(1, 5, (F, n)))
    classes1 = [np.array(c) for c in ([0, 0, 1, 1, 1, 1], [0, 0, 0, 0, 1, 1], [0, 0, 1, 1, 2, 2], [0, 0, 1, 1, 0, 0])]
    p1rows = [np.array([[0.5], [-0.5]]), np.eye(2), np.eye(3), np.array([[0.5], [-0.5]])]
    mats = write_alternatives(tmp_path, None, classes1, p1rows)
    base = str(tmp_path / "big")
    out, err = cli(FAST + ["-polyout", base] + m_args(mats) + files, timeout=900)
    lines = out.split("\n")
    assert lines[0] == "#prior_probabilities=0.2,0.2,0.2,0.2,0.2" and len(lines) == F + 3 and lines[-1] == ""
    assert all(len(ln.split("\t")) == 1 + 2 * n + 5 for ln in lines[1:-1:997])
    for j, L1 in enumerate([1, 2, 3, 1]):
        t = read("%s.model%d.mmdiff" % (base, j + 1)).split("\n")
        assert t[0] == "#prior_probability=0.1" and len(t) == F + 3 and t[-1] == ""
        assert all(len(ln.split("\t")) == 3 + 2 + L1 + 2 * n for ln in t[1:-1:997])
    ds = [design(j, None, classes1, p1rows) for j in range(4)]
    h = DiffPoly(y, e, ds[0][0], ds[0][1], np.zeros(n, int), [d[2] for d in ds], [d[3][:, 1] for d in ds])
    want = PR.poly_device_bytes(F, n, 1, 1, 1, True, [(1, 2), (2, 2), (3, 3), (1, 2)])
    assert h.device_bytes() == want
    assert want < sum(PR.single_device_bytes(F, n, 1, 1, L1, 1, nc, True) for L1, nc in [(1, 2), (2, 2), (3, 3), (1, 2)])
    h.close()
