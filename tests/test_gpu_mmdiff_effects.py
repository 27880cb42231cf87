"""mmdiff's effect summaries on the device against the restatement (tests/mmdiff_effects_ref.py): mmg_effects_of_rows on synthetic rows
over the kernel's tile, chunk and key-count edges; the rows a chain keeps on the device against the rows a traced handle hands out; the
error paths; the statistical rule of tests/test_mmdiff_effects_exact.py on the device's own rows; and the CLI's file byte for byte."""
import functools
import subprocess

import numpy as np
import pytest

import mmdiff_effects_ref as E
import mmdiff_ref as R
from test_gpu_mmdiff import MMDIFF, write_tables
from test_gpu_mmdiff_trace import FMAX, N, cli_inputs, make

PCT = (0.0, 2.5, 50.0, 97.5, 100.0)
FS = {1: 6, 8: 0, 63: 3, 65: 0, 130: 0}      # feature count -> the first of its columns in the 130 synthetic ones


def same(got, want, what=""):
    for k in ("n", "n_gt"):
        assert got[k].dtype == np.uint32 and np.array_equal(got[k], want[k]), (what, k)
    assert np.all((got["q"] == want["q"]) | (np.isnan(got["q"]) & np.isnan(want["q"]))), (what, "q")
    for k in ("mean", "sd"):
        assert np.array_equal(got[k], want[k], equal_nan=True), (what, k)


@functools.lru_cache(maxsize=None)
def synthetic(S, P):
    """rows (S, P, 130), model_of and the restatement's answer.  By feature f % 8, gamma is: all 0; all 1; 1 in one row; 0 in one row;
    else Bernoulli(0.1 .. 0.9).  By (f + s) % 8, parameter s is: all equal; -0.0 / +0.0 / -1 / +1; signed powers of ten from 1e-300 to
    1e300; a few values with many ties; else normal draws."""
    rng = np.random.default_rng(1000 * S + P)
    F = 130
    rows = np.empty((S, P, F))
    for f in range(F):
        k = f % 8
        g = (rng.random(S) < 0.1 + 0.8 * rng.random()).astype(np.float64)
        if k == 0:
            g[:] = 0.0
        elif k == 1:
            g[:] = 1.0
        elif k in (2, 3):
            g[:] = float(k == 3)
            g[rng.integers(S)] = float(k == 2)
        rows[:, P - 1, f] = g
        for s in range(P - 1):
            k = (f + s) % 8
            if k == 0:
                x = np.full(S, rng.normal())
            elif k == 1:
                x = rng.choice(np.array([-0.0, 0.0, -1.0, 1.0]), S)
            elif k == 2:
                x = rng.choice(np.array([-1.0, 1.0]), S) * 10.0 ** rng.uniform(-300, 300, S)
                x[rng.integers(S)], x[rng.integers(S)] = 1e-300, 1e300
            elif k == 3:
                x = rng.choice(rng.normal(size=5), S)
            else:
                x = rng.normal(0.3, 1.0, S)
            rows[:, s, f] = x
    model_of = np.array([(s + S) % 2 for s in range(P - 1)], np.uint8)
    return rows, model_of, E.effects(rows, model_of, PCT)


@pytest.mark.gpu
@pytest.mark.parametrize("P", [2, 3, 14])
@pytest.mark.parametrize("S", [1, 2, 3, 600, 1024, 1025, 4096])
def test_of_rows_equals_the_restatement(gpu, S, P):
    """S: one key, the smallest sorts, a chunk edge inside a series (600), the key counts 1024 | 2048 (1025) and 4096 (half a tile per
    workgroup).  F: less than a tile, one tile, tiles with a ragged last one, more than one block of features."""
    from mmseq_amd.diff import effects_of_rows
    rows, model_of, want = synthetic(S, P)
    for F, f0 in FS.items():
        sl = slice(f0, f0 + F)
        got = effects_of_rows(rows[:, :, sl], model_of, PCT)
        same(got, {k: v[..., sl] for k, v in want.items()}, "F %d" % F)
        assert got["device_bytes"] == 8 * F + (P - 1) * F * (20 + 8 * len(PCT)) + 8 * len(PCT) + (P - 1)
    again = effects_of_rows(rows[:, :, :65], model_of, PCT)
    for k in ("n", "mean", "sd", "n_gt", "q"):
        assert np.array_equal(again[k], got[k][..., :65], equal_nan=True), k     # (got: F = 130 from column 0)


@pytest.mark.gpu
def test_of_rows_without_percentiles_and_with_32(gpu):
    from mmseq_amd.diff import effects_of_rows
    rows, model_of, want = synthetic(600, 3)
    got = effects_of_rows(rows, model_of, ())
    assert got["q"].shape == (2, 0, 130)
    same(got, dict(want, q=want["q"][:, :0]))
    pct = np.linspace(0, 100, 32)
    same(effects_of_rows(rows, model_of, pct), E.effects(rows, model_of, pct))


@pytest.mark.gpu
def test_of_rows_refusals(gpu):
    from mmseq_amd._lib import MMGError
    from mmseq_amd.diff import effects_of_rows
    rows = np.zeros((4, 3, 9))
    for kw, text in ((dict(percentiles=(-1.0,)), "between 0 and 100"), (dict(percentiles=(float("nan"),)), "between 0 and 100"),
                     (dict(percentiles=(100.5,)), "between 0 and 100"), (dict(percentiles=range(33)), "at most 32"),
                     (dict(model_of=[0, 2]), "model_of")):
        with pytest.raises(MMGError) as ex:
            effects_of_rows(rows, kw.get("model_of", [0, 1]), kw.get("percentiles", PCT))
        assert ex.value.code == 1 and text in str(ex.value), kw
    for shape in ((0, 3, 9), (4097, 3, 1), (4, 1, 9)):
        with pytest.raises(MMGError) as ex:
            effects_of_rows(np.zeros(shape), [0, 1][:max(shape[1] - 1, 0)], PCT)
        assert ex.value.code == 1
    bad = rows.copy()
    bad[2, 2, 5] = 0.5
    with pytest.raises(MMGError) as ex:
        effects_of_rows(bad, [0, 1], PCT)
    assert ex.value.code == 1 and "gamma of row 2, feature 5" in str(ex.value)
    assert effects_of_rows(rows, [0, 1], PCT)["n"][0].tolist() == [4] * 9     # the library is usable afterwards


# ---- from a chain ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("every", [1, 7, 16])
@pytest.mark.parametrize("F", [1, 65, 130])
def test_effects_of_a_chain_equal_the_restatement_of_its_traced_rows(gpu, F, every):
    """burnin(1100), sample(600): the rows a traced handle hands to the host, restated, against the summary of the rows the effects handle
    keeps on the device -- in one sampling call and in two (130 + 470: the second starts inside a launch's row interval)."""
    traced = make("covariate", F, 41)
    traced.open_traces(1100, every)
    traced.burnin(1100)
    traced.sample(600)
    rows = traced.traces()[1]
    names = traced.trace_names()
    traced.close()
    n_rows = -(-600 // every)
    assert rows.shape == (n_rows, len(names), F)
    want = E.effects(rows, E.model_of_names(names[:-1]), PCT)

    plain = make("covariate", F, 41)
    base = plain.device_bytes()
    plain.burnin(1100)
    plain.sample(600)
    res = plain.results()
    plain.close()
    for pieces in ((600,), (130, 470)):
        d = make("covariate", F, 41)
        d.open_effects(every, n_rows)
        assert d.device_bytes() == base + n_rows * len(names) * F * 8 + 496
        d.burnin(1100)
        for n in pieces:
            d.sample(n)
        got = d.effects(PCT)
        assert got["names"] == names[:-1]
        same(got, want, "pieces %r" % (pieces,))
        same(d.effects(PCT), want, "again")
        mine = d.results()
        for k in res:
            assert np.array_equal(mine[k], res[k], equal_nan=True), k
        d.close()
    assert np.all(want["n"].sum(0) == n_rows) and want["n"].min() < n_rows     # both models are visited


@pytest.mark.gpu
def test_effects_grow_with_the_sampling_calls(gpu):
    """A summary between two sampling calls is that of the rows so far; tuning batches before sampling change nothing in the rule."""
    traced = make("de22", 65, 42)
    traced.open_traces(1024, 3)
    traced.burnin(1024)
    traced.tune_batch()
    traced.sample(100)
    first = traced.traces()[1]
    traced.sample(200)
    both = traced.traces()[1]
    names = traced.trace_names()
    traced.close()
    d = make("de22", 65, 42)
    d.open_effects(3, 100)
    d.burnin(1024)
    d.tune_batch()
    d.sample(100)
    model_of = E.model_of_names(names[:-1])
    same(d.effects(PCT), E.effects(first, model_of, PCT))
    d.sample(200)
    assert both.shape[0] == 100
    same(d.effects(PCT), E.effects(both, model_of, PCT))
    d.close()


@pytest.mark.gpu
def test_effects_error_paths(gpu):
    from mmseq_amd._lib import MMGError

    def raises(code, text, fn, *a):
        with pytest.raises(MMGError) as ex:
            fn(*a)
        assert ex.value.code == code and text in str(ex.value), str(ex.value)

    d = make("de22", 65, 5)
    for every, rows in ((0, 10), (2 ** 30 + 1, 10), (1, 0), (1, 4097)):
        raises(1, "must be", d.open_effects, every, rows)
    raises(4, "without mmg_diff_effects_open", d.effects, PCT)
    d.open_effects(4, 50)
    raises(4, "already", d.open_effects, 4, 50)
    raises(4, "exclude each other", d.open_traces, 1, 1)
    d.burnin(1024)
    raises(4, "before a sampling row exists", d.effects, PCT)
    raises(1, "more rows than", d.sample, 201)                   # 201 iterations: 51 rows
    d.sample(120)                                                # the refused call launched nothing: the handle goes on
    raises(1, "more rows than", d.sample, 81)
    d.sample(80)
    raises(1, "between 0 and 100", d.effects, (101.0,))
    raises(1, "at most 32", d.effects, tuple(range(33)))
    got = d.effects(PCT)
    assert np.all(got["n"].sum(0) == 50)
    plain = make("de22", 65, 5)
    plain.burnin(1024)
    plain.sample(200)
    want = plain.results()
    mine = d.results()
    for k in want:
        assert np.array_equal(mine[k], want[k], equal_nan=True), k
    raises(1, "after the burn-in", plain.open_effects, 1, 10)     # opening late
    plain.sample(10)                                             # ... leaves the handle usable
    plain.close()
    d.close()
    t = make("de22", 1, 5)
    t.open_traces(1, 1)
    raises(4, "exclude each other", t.open_effects, 1, 10)        # opening with tracing open
    t.burnin(1024)
    t.sample(8)
    assert t.traces()[1].shape[0] == 8
    t.close()


# ---- the statistical rule on the device's own rows ------------------------------------------------------------------------------
@pytest.mark.gpu
def test_effects_of_the_device_chain_match_the_exact_posterior(gpu):
    """The inputs and the rule of tests/test_mmdiff_effects_exact.py::test_restated_effects_match_the_exact_posterior, the rows from the
    device's chain."""
    import test_mmdiff_effects_exact as X
    from mmseq_amd.diff import Diff
    y, e, M, P0, P1, classes, kw = X.stat_inputs()
    d = Diff(y, e, M, P0, P1, classes, pdash=X.PDASH, seed=X.SEED, **kw)
    d.open_effects(X.THIN, X.ITERS // X.THIN)
    d.burnin(X.BURNIN)
    d.sample(X.ITERS)
    got = d.effects(X.PCT)
    d.close()
    X.check_effects_against_exact(got, "device")


@pytest.mark.gpu
def test_effects_of_the_device_chain_match_the_exact_posterior_with_three_covariates(gpu):
    """The same on design f_cov3 (test_mmdiff_effects_exact.COV3): three covariate columns, so the summaries of six beta columns go
    through the rule beside alpha and eta.  Measured on an MI355X (and the same, bit for bit, with the restatement on the CPU): n under
    model 0 from 29 to 75 of 128 rows, under model 1 from 53 to 99; the 86 deviations lie between -1.60 s.e. (q 2.5 of beta0_2, fixture
    row 2) and +2.17 s.e. (P(> 0) of beta0_0, fixture row 2), two of them beyond 2."""
    import test_mmdiff_effects_exact as X
    from mmseq_amd.diff import Diff
    cfg = X.COV3
    y, e, M, P0, P1, classes, kw = X.stat_inputs(cfg["case"])
    d = Diff(y, e, M, P0, P1, classes, pdash=cfg["pdash"], seed=cfg["seed"], **kw)
    d.open_effects(X.THIN, X.ITERS // X.THIN)
    d.burnin(X.BURNIN)
    d.sample(X.ITERS)
    got = d.effects(X.PCT)
    d.close()
    assert [n for n in got["names"] if n.startswith("beta")] == ["beta%d_%d" % (m, j) for m in range(2) for j in range(3)]
    X.check_effects_against_exact(got, "device f_cov3", cfg)


# ---- the CLI ---------------------------------------------------------------------------------------------------------------
def format_effects(features, fx, fixalpha, Mnil, Pnil):
    """The file `mmdiff -effects` writes, from the dict of Diff.effects()."""
    def has(name):
        stem = name.split("_")[0]
        kind, m = stem[:-1], int(stem[-1])
        return {"alpha": not fixalpha, "beta": not Mnil, "eta": not Pnil[m], "lambda": not Pnil[m]}.get(kind, True)

    def g(x):
        return "nan" if np.isnan(x) else "%.9g" % x

    cols = [s for s, name in enumerate(fx["names"]) if has(name)]
    head = ["feature_id", "n0", "n1"]
    for s in cols:
        nm = fx["names"][s]
        head += [nm + "_mean", nm + "_sd", nm + "_p_gt0"] + ["%s_q%s" % (nm, g(p)) for p in fx["percentiles"]]
    lines = ["\t".join(head)]
    with np.errstate(invalid="ignore", divide="ignore"):
        for f, feat in enumerate(features):
            cells = [feat, "%d" % fx["n"][0, f], "%d" % fx["n"][1, f]]
            for s in cols:
                m = int(fx["names"][s].split("_")[0][-1])
                cells += [g(fx["mean"][s, f]), g(fx["sd"][s, f]), g(np.float64(fx["n_gt"][s, f]) / np.float64(fx["n"][m, f]))]
                cells += [g(v) for v in fx["q"][s, :, f]]
            lines.append("\t".join(cells))
    return "\n".join(lines) + "\n"


@pytest.mark.gpu
@pytest.mark.parametrize("extra,pct", [([], (2.5, 50.0, 97.5)), (["-effects_every", "3", "-effects_percentiles", "0,10,50,99.5,100"], (0.0, 10.0, 50.0, 99.5, 100.0))])
def test_cli_effects_file(gpu, tmp_path, extra, pct):
    from mmseq_amd.diff import Diff
    files = cli_inputs(tmp_path)
    out = tmp_path / "effects.txt"
    args = ["-burnin", "1024", "-iter", "1024"]
    run = lambda a: subprocess.run([MMDIFF] + a + ["-de", "2", "2"] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    plain = run(args)
    fx = run(args + ["-effects", str(out)] + extra)
    assert plain.returncode == 0 and fx.returncode == 0, fx.stderr.decode()[-2000:]
    assert fx.stdout == plain.stdout and len(plain.stdout) > 0
    # the same run through the bindings: the CLI's normalisation restated (tests/mmdiff_ref.py), its seed, p' and tuning loop
    tabs = [R.read_table(f) for f in files]
    y, e, uh = (np.stack([t[i] for t in tabs], 1) for i in (1, 2, 3))
    y, factors = R.normalise(y, uh, max(0.2, float(N - N * N // 160) / float(N)))
    assert factors is not None
    M, P0, P1, C = R.de_design([2, 2])
    every = 3 if extra else 1
    d = Diff(y, e, M, P0, P1, C, seed=1234)
    d.open_effects(every, -(-1024 // every))
    d.burnin(1024)
    nb = d.tune()
    d.sample(1024)
    want = format_effects(["f%d" % i for i in range(FMAX)], d.effects(pct), False, True, (True, False))
    d.close()
    assert ("sampling after %d tuning batches" % nb).encode() in fx.stderr
    got = out.read_bytes().decode()
    assert got == want
    head = got.split("\n")[0].split("\t")
    assert head[:6] == ["feature_id", "n0", "n1", "alpha0_mean", "alpha0_sd", "alpha0_p_gt0"]
    assert not any(h.startswith(("beta", "eta0", "lambda0")) for h in head) and "eta1_0_q50" in head and "rho1_mean" in head
    assert len(got.split("\n")) == FMAX + 2
