"""mmdiff on the device on the designs of tests/wide_designs.py, bit for bit against the numpy restatements: two and three covariate
columns (the off-diagonal loops of the beta update's Cholesky factors, triangular inverse and V = Li'Li run, and every K-strided
slot holds more than one value), a fitted model 0 with its own eta, lambda and two variance classes, both together, the host's size
caps (K = 8, 16 columns of P0 and P1, 16 classes per model), N = 512 and N = 2.  Every handle kind is driven on such a design:
Diff, the CLI with a three-column M block, traces, effects, chains, permutations and the polytomous handle.

F = 130 is two full blocks and two lanes.  The restatement costs 15 to 45 ms per iteration on these designs whatever F is, so the
runs are the shortest the other device tests of the same handle use, a design's restatement is computed once and shared
(functools.lru_cache; nothing changes it afterwards), and the traced restatement of k3_batch serves the Diff, traces and effects
tests of that design."""
import functools
import os
import time

import numpy as np
import pytest

import mmdiff_chains_ref as CR
import mmdiff_effects_ref as E
import mmdiff_perm_ref as PR
import mmdiff_poly_ref as PolyR
import mmdiff_ref as R
import mmdiff_trace_ref as TR
import wide_designs as W
from test_gpu_mmdiff import cli, write_tables

F = 130
SEED = (0x5A17 << 32) | 77          # high bits set: chains and replicas are xored into them
DATA_SEED = {name: 900 + i for i, name in enumerate(sorted(W.DESIGNS))}
PCT = (0.0, 2.5, 50.0, 97.5, 100.0)


def same_results(got, want, what=""):
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k].shape == want[k].shape, (what, k)
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, k)


def drive(h, burnin, batches, iters):
    h.burnin(burnin)
    counts = [h.tune_batch() for _ in range(batches)]
    h.sample(iters)
    return counts


def bytes_of(name, n_features):
    s = W.shape(name)
    return PolyR.single_device_bytes(n_features, s["N"], s["K"], s["L0"], s["L1"], s["nc0"], s["nc1"], s["Mnil"])


@functools.lru_cache(maxsize=None)
def ref_single(name, fixalpha=False, n_features=F, burnin=1024, batches=2, iters=256):
    """The restatement driven as the device test drives its handle: (untuned counts per batch, results, CPU seconds)."""
    y, e = W.data(name, n_features, DATA_SEED[name])
    t0 = time.process_time()
    b = R.BMS(y, e, *W.design(name), fixalpha=fixalpha, seed=SEED)
    counts = drive(b, burnin, batches, iters)
    res = b.results()
    for v in res.values():
        v.setflags(write=False)
    return counts, res, time.process_time() - t0


@functools.lru_cache(maxsize=None)
def ref_k3_batch():
    """k3_batch traced: burn-in 1100 recorded every 7th, three tuning batches (two tuning lines), 600 sampling iterations every 5th --
    neither interval divides the 512 iterations of a launch.  (TracedBMS, pseudo, untuned counts)."""
    y, e = W.data("k3_batch", F, DATA_SEED["k3_batch"])
    b = TR.TracedBMS(y, e, *W.design("k3_batch"), every_burnin=7, every_sample=5, seed=SEED)
    b.burnin(1100)
    pseudo = b.pseudo()
    counts = [b.tune_batch() for _ in range(3)]
    b.sample(600)
    return b, pseudo, counts


def make(name, n_features=F, **kw):
    from mmseq_amd.diff import Diff
    y, e = W.data(name, n_features, DATA_SEED[name])
    return Diff(y, e, *W.design(name), seed=SEED, **kw)


def check_handle(d, name, n_features):
    s = W.shape(name)
    assert d.device_bytes() == bytes_of(name, n_features)
    assert d.info()["Mnil"] == s["Mnil"] and d.info()["Pnil"] == s["Pnil"] and d.info()["n_classes"] == (s["nc0"], s["nc1"])
    assert (d.K, d.L) == (s["K"], (s["L0"], s["L1"]))


# ---- Diff ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,fixalpha", [("k2", False), ("k3", False), ("k3", True), ("batch", False), ("n2", False)])
def test_diff_equals_the_restatement(gpu, name, fixalpha):
    """Burn-in 1024, the pseudopriors, two tuning batches (the second tunes logit p' first) and 256 sampling iterations: the untuned
    counts, every key of results() and the memory.  With -fixalpha on k3 the prior variance of beta is 25."""
    want_counts, want, _ = ref_single(name, fixalpha)
    d = make(name, fixalpha=fixalpha)
    check_handle(d, name, F)
    counts = drive(d, 1024, 2, 256)
    got = d.results()
    assert d.info()["batches"] == 2 and d.device_bytes() == bytes_of(name, F)
    d.close()
    assert counts == want_counts and counts[0] == F
    assert got["beta"].shape == (2, W.shape(name)["K"], F)
    if not W.shape(name)["Mnil"]:
        assert np.isfinite(want["beta"]).all() and np.unique(want["beta"]).size == want["beta"].size       # no two columns alike
    assert 0.0 < want["gamma_mean"].mean() < 1.0 and np.unique(want["logitp"]).size > 1                    # gamma moves, tuning acted
    same_results(got, want, name)


@pytest.mark.gpu
def test_diff_on_k3_batch_equals_the_traced_restatement(gpu):
    """Three covariates and a fitted model 0 (eta, lambda and two variance classes) against three classes in model 1: burn-in 1100,
    three tuning batches, 600 sampling iterations."""
    b, _, want_counts = ref_k3_batch()
    d = make("k3_batch")
    check_handle(d, "k3_batch", F)
    d.burnin(1100)
    counts = [d.tune_batch() for _ in range(3)]
    d.sample(600)
    want, got = b.results(), d.results()
    d.close()
    assert counts == want_counts
    assert got["eta"].shape == (3, F) and np.isfinite(want["beta"]).all()
    fitted0 = np.isfinite(want["alpha"][0])
    assert fitted0.any() and np.isfinite(want["eta"][0][fitted0]).all()        # model 0's eta has a mean wherever model 0 was visited
    same_results(got, want, "k3_batch")


@pytest.mark.gpu
def test_diff_at_the_size_caps_equals_the_restatement(gpu):
    """`caps`: N = 40, K = 8, 16 columns in P0 and P1, 16 variance classes in both models, F = 66.  The shortest run in which the
    burn-in records 32 iterations (134: recording starts at 102), two tuning batches run and 128 iterations are sampled -- the
    restatement takes 0.13 to 0.16 s per iteration here: 85 CPU seconds measured for the 518 iterations.  With these random matrices
    gamma stays in model 0 (mean gamma 0.015), so model 1's alpha and eta means are NaN for most features; its state is compared
    through what it feeds: the burn-in fits both models, and their pseudopriors, log densities and beta sums reach every other key."""
    want_counts, want, secs = ref_single("caps", False, 66, 134, 2, 128)
    print("restatement of caps: %.1f CPU seconds" % secs)
    d = make("caps", 66)
    check_handle(d, "caps", 66)
    counts = drive(d, 134, 2, 128)
    got = d.results()
    d.close()
    assert counts == want_counts
    assert got["beta"].shape == (2, 8, 66) and got["eta"].shape == (32, 66)
    assert np.isfinite(want["beta"]).all() and np.isfinite(want["gamma_mean"]).all()
    same_results(got, want, "caps")


@pytest.mark.gpu
def test_diff_on_512_samples_equals_the_restatement(gpu):
    """`n512`: the largest N the host accepts, one covariate, F = 66; 134 burn-in iterations, two tuning batches, 128 sampling
    iterations as for `caps`.  The restatement takes 0.06 to 0.09 s per iteration: 40 CPU seconds measured."""
    want_counts, want, secs = ref_single("n512", False, 66, 134, 2, 128)
    print("restatement of n512: %.1f CPU seconds" % secs)
    d = make("n512", 66)
    check_handle(d, "n512", 66)
    counts = drive(d, 134, 2, 128)
    got = d.results()
    d.close()
    assert counts == want_counts and np.isfinite(want["beta"]).all()
    same_results(got, want, "n512")


# ---- the CLI ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cli_with_a_three_column_m_block_is_byte_identical(gpu, tmp_path):
    """k3_batch through the matrices file: three columns in the M block, a row of P0 per batch and a row of P1 per cell.  stdout
    against R.mmdiff; with -traces the same stdout, the files of every parameter of param_names(3, [1, 2], [2, 3]) and the
    `pseudo` header with B<m>_0 .. B<m>_2 and Vbeta<m>_0 .. Vbeta<m>_2."""
    y, e = W.data("k3_batch", F, DATA_SEED["k3_batch"] + 50)
    uh = np.random.default_rng(3).integers(1, 5, y.shape)
    files = write_tables(tmp_path, y, e, uh)
    mat = tmp_path / "design.txt"
    mat.write_text(W.matrices_text("k3_batch"))
    opts, tail = ["-burnin", "1024", "-iter", "1024", "-notune"], ["-m", str(mat)] + files        # options come before -m
    out, err = cli(opts + tail)
    hdr = out.split("\n")[1].split("\t")
    assert hdr[:14] == ["feature_id", "bayes_factor", "posterior_probability", "alpha0", "beta0_0", "beta0_1", "beta0_2", "eta0_0",
                        "alpha1", "beta1_0", "beta1_1", "beta1_2", "eta1_0", "eta1_1"] and hdr[14].startswith("mu_")
    want = R.mmdiff(files, design=W.design("k3_batch"), burnin=1024, iters=1024, tune=False)
    assert out == want
    tdir = tmp_path / "traces"
    traced, _ = cli(opts + ["-traces", str(tdir)] + tail)
    assert traced == out
    names = TR.param_names(3, [1, 2], [2, 3])
    assert set(os.listdir(tdir)) == set(names) | {n + "-burnin" for n in names} | {"logitp", "logitp-burnin", "meanLO", "meanLO-burnin", "pseudo"}
    with open(tdir / "pseudo") as f:
        lines = f.read().split("\n")
    assert lines[0] + "\n" == TR.pseudo_header(3, [1, 2], [2, 3]) and "B0_2\tVbeta0_2\t" in lines[0] and "B1_2\tVbeta1_2\t" in lines[0]
    assert len(lines) == F + 2 and all(len(l.split("\t")) == len(lines[0].split("\t")) for l in lines[1:-1])
    with open(tdir / "beta1_2") as f:
        rows = f.read().split("\n")
    assert len(rows) == 1025 and all(len(r.split(" ")) == F + 1 for r in rows[:-1])


# ---- traces and effects ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_traces_of_k3_batch_equal_the_restatement(gpu):
    """22 traced parameters: rows of both phases, the two tuning lines and the pseudopriors, `==` for `==`."""
    b, pseudo, _ = ref_k3_batch()
    d = make("k3_batch")
    names = TR.param_names(3, [1, 2], [2, 3])
    assert d.trace_names() == names == b.names() and len(names) == 22
    d.open_traces(7, 5)
    d.burnin(1100)
    got_pseudo = d.pseudo()
    tune_rows = []
    for batch in range(3):
        if batch > 0:
            tune_rows.append(d.tune_state())
        d.tune_batch()
    d.sample(600)
    burn, samp = d.traces()
    d.close()
    assert burn.shape == (158, 21, F) and samp.shape == (120, 22, F)
    assert np.array_equal(burn, b.stacked(0)) and np.array_equal(samp, b.stacked(1))
    assert got_pseudo.shape == pseudo.shape == (2 * (2 + 2 * 3 + 2) + 3 * 3 + 2 * 5, F) and np.array_equal(got_pseudo, pseudo, equal_nan=True)
    assert len(b.tune_rows) == 2
    for (lo, lp), (wlo, wlp) in zip(tune_rows, b.tune_rows):
        assert np.array_equal(lo, wlo) and np.array_equal(lp, wlp)
    for j, k in ((0, 1), (0, 2), (1, 2)):          # the beta columns are different series
        assert not np.array_equal(samp[:, 2 + j], samp[:, 2 + k]) and not np.array_equal(samp[:, 5 + j], samp[:, 5 + k])


@pytest.mark.gpu
def test_effects_of_k3_batch_equal_the_restatement_of_the_traced_rows(gpu):
    """The rows an effects handle keeps on the device, summarised there, against the restatement's summary of the restated rows: 21
    parameters, three beta columns per model, eta and lambda of model 0."""
    from test_gpu_mmdiff_effects import same
    b, _, _ = ref_k3_batch()
    names = b.names()
    want = E.effects(b.stacked(1), E.model_of_names(names[:-1]), PCT)
    d = make("k3_batch")
    d.open_effects(5, 120)
    assert d.device_bytes() == bytes_of("k3_batch", F) + 120 * 22 * F * 8 + 496
    d.burnin(1100)
    for _ in range(3):
        d.tune_batch()
    d.sample(600)
    got = d.effects(PCT)
    res = d.results()
    d.close()
    assert got["names"] == names[:-1]
    same(got, want, "k3_batch")
    same_results(res, b.results(), "k3_batch with effects open")
    assert np.all(want["n"].sum(0) == 120) and 0 < want["n"][0].sum() < 120 * F            # both models are visited


# ---- chains, permutations, the polytomous handle -------------------------------------------------------------------------------
@pytest.mark.gpu
def test_two_chains_of_k3_batch_and_their_pooled_output(gpu):
    """C = 2, 1024 + 1024 iterations without tuning: each chain's results and batch sums against the restatement with the chain in
    the stream key, the pooled columns and the pooled means (2 (2 + 2 K + L0 + L1) = 22 sums and counts per feature) bitwise, and
    the memory."""
    from mmseq_amd.diff import DiffChains
    y, e = W.data("k3_batch", F, DATA_SEED["k3_batch"])
    design = W.design("k3_batch")
    runs = CR.run_chains_untuned(2, y, e, *design, seed=SEED, burnin=1024, iters=1024)
    h = DiffChains(y, e, *design, 2, 1024, seed=SEED)
    assert h.device_bytes() == CR.chains_device_bytes(F, 12, 3, 1, 2, 2, 3, False, 2)
    h.burnin(1024)
    h.sample(1024)
    h.pool()
    for c, (_, want, gb, _) in enumerate(runs):
        same_results(h.results(c), want, "chain %d" % c)
        assert np.array_equal(h.batch_sums(c), gb)
    got = h.pooled()
    h.close()
    assert not np.array_equal(runs[0][1]["beta"], runs[1][1]["beta"])
    cols = CR.pool([b.gsum for b, _, _, _ in runs], [b.logitp for b, _, _, _ in runs], [gb for _, _, gb, _ in runs], 1024)
    for k in ("log_bf", "log_bf_sd", "log_bf_mcse"):
        assert np.array_equal(got[k], cols[k], equal_nan=True), k
    assert np.array_equal(got["chains_mixed"], cols["chains_mixed"]) and cols["chains_mixed"].max() == 2
    means = CR.pooled_means([b for b, _, _, _ in runs])
    for k in ("alpha", "beta", "eta"):
        assert got[k].shape == means[k].shape and np.array_equal(got[k], means[k], equal_nan=True), k
    assert np.isfinite(means["beta"]).all()


@pytest.mark.gpu
def test_permutation_replicas_of_k3_are_single_handles_on_the_shuffled_data(gpu):
    """B = 2 on k3: replica b against Diff on the restated shuffle of the data with seed ^ (b << 32); burn-in 1024, two tuning
    batches at the most, 256 sampling iterations."""
    from mmseq_amd.diff import DiffPerm
    from test_gpu_mmdiff_perm import assert_replica_is_single
    from test_gpu_mmdiff_perm import drive as drive_perm
    y, e = W.data("k3", F, DATA_SEED["k3"])
    design = W.design("k3")
    h = DiffPerm(y, e, *design, 2, seed=SEED)
    assert h.device_bytes() == PR.perm_device_bytes(F, 12, 3, 1, 1, 1, 2, False, 2)
    nb = drive_perm(h, 1024, 2, 256)
    assert h.info(1)["Mnil"] is False
    for b in range(3):
        assert assert_replica_is_single(h, b, y, e, design, SEED, 1024, 2, 256) == nb[b]
    assert not np.array_equal(h.results(0)["beta"], h.results(1)["beta"])
    h.close()


POLY_ALTS = 2


def poly_design(j):
    """K = 2, model 0 fitted (the batch contrast, a class per batch), and two alternatives that share it: the `batch` design's P1
    with the condition's two classes, and that P1 with a third, per-sample column and the three cells as classes."""
    M, P0, P1, C = W.design("batch")
    M = W.M3[:, :2].copy()
    if j == 1:
        P1 = np.concatenate([P1, W.M3[:, 2:3]], 1)
        C = np.stack([C[:, 0], W.CELL], 1)
    return M, P0, P1, C


@functools.lru_cache(maxsize=None)
def ref_poly(j):
    y, e = W.data("batch", F, DATA_SEED["batch"] + 50)
    b = R.BMS(y, e, *poly_design(j), seed=SEED)
    counts = drive(b, 1024, 2, 256)
    return counts, b.results()


@pytest.mark.gpu
def test_poly_with_a_fitted_model_0_shared_by_two_alternatives(gpu):
    """Each comparison of the DiffPoly handle against a separate Diff handle and against the restatement: burn-in 1024, two tuning
    batches, 256 sampling iterations; the memory of both kinds of handle."""
    from mmseq_amd.diff import Diff, DiffPoly
    y, e = W.data("batch", F, DATA_SEED["batch"] + 50)
    ds = [poly_design(j) for j in range(POLY_ALTS)]
    for d in ds[1:]:
        assert np.array_equal(d[0], ds[0][0]) and np.array_equal(d[1], ds[0][1]) and np.array_equal(d[3][:, 0], ds[0][3][:, 0])
    h = DiffPoly(y, e, ds[0][0], ds[0][1], ds[0][3][:, 0], [d[2] for d in ds], [d[3][:, 1] for d in ds], seed=SEED)
    assert h.device_bytes() == PolyR.poly_device_bytes(F, 12, 2, 1, 2, False, [(2, 2), (3, 3)])
    h.burnin(1024)
    batches = [h.tune_batch() for _ in range(2)]
    h.sample(256)
    for j, (M, P0, P1, C) in enumerate(ds):
        want_counts, want = ref_poly(j)
        assert [n[j] for n, _ in batches] == want_counts and not any(ended[j] for _, ended in batches)
        d = Diff(y, e, M, P0, P1, C, seed=SEED)
        assert d.device_bytes() == PolyR.single_device_bytes(F, 12, 2, 1, P1.shape[1], 2, int(C[:, 1].max()) + 1, False)
        assert drive(d, 1024, 2, 256) == want_counts
        assert h.info(j)["Pnil"] == (False, False) and h.info(j)["n_classes"] == (2, 2 + j)
        same_results(d.results(), want, "single %d" % j)
        same_results(h.results(j), want, "poly %d" % j)
        d.close()
    h.close()
    assert not np.array_equal(ref_poly(0)[1]["eta"][0], ref_poly(1)[1]["eta"][0])
