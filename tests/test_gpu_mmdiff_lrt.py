"""mmdiff -lrt on the device: DiffLrt against the numpy restatement with `==` on every output (p_value and q_value included: the
host side computes them with dlog / dexp / dlgamma, which the restatement has bit for bit), against the independent
grid-plus-polish optimum, the bounded loops, the CLI and the memory formula.

Which instantiation a case runs: k_lrt<4> (X'WX, its factor and theta in registers) when both models have at most 4 columns --
de33, one, n2, de34, de222 (4 columns in model 1, collinear: status 2), de222_fixalpha, fixalpha, covariate, k2, n512;
k_lrt<0> (the triangle and theta in per-lane workspace slots) otherwise -- k3 (5 columns in model 1), k3_batch (5 and 6), caps (25 and 25)."""
import numpy as np
import pytest

import lrt_optimum as O
import mmdiff_lrt_ref as L
import mmdiff_ref as R
import wide_designs as W
from test_gpu_mmdiff import FAST, cli, synth, write_tables
from test_mmdiff_lrt_ref import TOL_LOGLIK, TOL_STAT

KEYS = ("loglik", "stat", "p_value", "q_value", "theta0", "theta1", "sigmasq0", "sigmasq1", "iters", "status")


def _de(groups, F, seed, fixalpha=False):
    M, P0, P1, C = R.de_design(groups)
    y, e, _, _ = synth(F, sum(groups), seed=seed, groups=list(groups))
    y[F // 2] = y[F // 2, 0]              # identical replicates: the boundary
    return dict(y=y, e=e, M=M, P0=P0, P1=P1, C=C, fixalpha=fixalpha)


def _wide(name, F):
    M, P0, P1, C = W.design(name)
    y, e = W.data(name, F, 5)
    return dict(y=y, e=e, M=M, P0=P0, P1=P1, C=C, fixalpha=False)


def _covariate():
    c = _de((3, 3), 20, 13)
    c["M"] = O.COV6.copy()
    return c


# name -> (the case, the instantiation it must run: the largest number of columns decides)
CASES = {
    "de33": lambda: _de((3, 3), 130, 11),             # two full blocks and a tail of 2 lanes
    "one": lambda: _de((3, 3), 1, 12),                # F = 1
    "n2": lambda: _de((1, 1), 20, 14),                # N = 2: a saturated model 1, residuals exactly 0
    "de34": lambda: _de((3, 4), 20, 15),              # N = 7
    "de222": lambda: _de((2, 2, 2), 20, 16),
    "de222_fixalpha": lambda: _de((2, 2, 2), 20, 16, True),
    "fixalpha": lambda: _de((3, 3), 20, 17, True),
    "covariate": _covariate,                          # K = 1
    "k2": lambda: _wide("k2", 20),
    "n512": lambda: _wide("n512", 8),                 # N = 512
    "k3": lambda: _wide("k3", 20),                    # K = 3
    "k3_batch": lambda: _wide("k3_batch", 20),        # K = 3 with a fitted model 0
    "caps": lambda: _wide("caps", 8),                 # K = 8, 16 columns of P0 and P1, 16 classes, N = 40: p = 25
}
REGISTERS = {"de33", "one", "n2", "de34", "de222", "de222_fixalpha", "fixalpha", "covariate", "k2", "n512"}


def run_device(c, max_iters=0):
    from mmseq_amd.diff import DiffLrt
    h = DiffLrt(c["y"], c["e"], c["M"], c["P0"], c["P1"], c["C"], fixalpha=c["fixalpha"], max_iters=max_iters)
    try:
        return h.results(), h.device_bytes()
    finally:
        h.close()


def assert_equal(got, want, what=""):
    assert got["df"] == want["df"] and tuple(got["n_cols"]) == tuple(want["n_cols"]) and tuple(got["n_classes"]) == tuple(want["n_classes"])
    for k in KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k], equal_nan=got[k].dtype == np.float64), (what, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_equals_the_restatement(gpu, name):
    c = CASES[name]()
    got, nbytes = run_device(c)
    want = L.lrt(c["y"], c["e"], c["M"], c["P0"], c["P1"], c["C"], c["fixalpha"])
    assert (max(want["n_cols"]) <= 4) == (name in REGISTERS)
    assert_equal(got, want, name)
    # the memory: the formula of include/mmgibbs.h
    F, N = c["y"].shape
    p, nc = want["n_cols"], want["n_classes"]
    pm = max(p)
    W_ = 2 * max(nc) + (0 if pm <= 4 else pm * (pm + 1) // 2)
    assert nbytes == 8 * (2 * F * N + (N + F) * sum(p) + F * sum(nc) + 2 * F + F * W_) + 4 * (2 * N + 4 * F)
    if name == "de222":
        assert np.all(got["status"][1] == L.ST_SINGULAR) and np.isnan(got["stat"]).all() and np.all(got["status"][0] != L.ST_SINGULAR)
    else:
        assert np.all(got["status"] & L.ST_SINGULAR == 0) and np.isfinite(got["stat"]).all()
    if name == "n2":
        assert np.all(got["sigmasq1"] == 0.0) and np.all(got["status"][1] == L.ST_BOUNDARY)
    if name in ("de33", "one", "n2", "de34", "de222", "covariate"):       # identical replicates: model 0 ends on the boundary
        assert got["status"][0, F // 2] == L.ST_BOUNDARY and np.all(got["sigmasq0"][:, F // 2] == 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("name", O.FIXTURES)
def test_device_reaches_the_independent_optimum(gpu, name):
    """The device against the grid-plus-polish maximum directly, on the fixtures of tests/test_mmdiff_lrt_ref.py (every profile
    has a single local maximum there) and with that test's tolerance."""
    fx = O.fixture(name)
    got, _ = run_device(fx)
    ref = O.reference(name, True)
    for m in O.MODELS[name]:
        want = np.array([o["loglik"] for o in ref[m]])
        print(name, "model", m, "l - reference:", got["loglik"][m] - want)
        assert np.all(got["status"][m] & (L.ST_CAP | L.ST_SINGULAR) == 0)
        assert np.all(np.abs(got["loglik"][m] - want) <= TOL_LOGLIK)
    if O.MODELS[name] == (0, 1):
        want = 2.0 * (np.array([o["loglik"] for o in ref[1]]) - np.array([o["loglik"] for o in ref[0]]))
        assert np.all(np.abs(got["stat"] - want) <= TOL_STAT)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["de33", "k3"])
def test_max_iters_bounds_the_scoring_loop(gpu, name):
    c = CASES[name]()
    full = L.lrt(c["y"], c["e"], c["M"], c["P0"], c["P1"], c["C"], c["fixalpha"])
    for cap in (1, 3):
        got, _ = run_device(c, max_iters=cap)
        assert_equal(got, L.lrt(c["y"], c["e"], c["M"], c["P0"], c["P1"], c["C"], c["fixalpha"], max_iters=cap), (name, cap))
        needs_more = full["iters"] > cap
        assert needs_more.any() and np.array_equal((got["status"] & L.ST_CAP) != 0, needs_more) and got["iters"].max() == cap


@pytest.mark.gpu
@pytest.mark.parametrize("K", [2, 5], ids=["registers", "slots"])
def test_collinear_columns_and_unusable_weights_leave_at_once(gpu, K):
    """Through the library, which takes any M: two equal columns of M make X'WX singular in both models for every feature; an e
    of 1e200 (finite, its square is not) makes one feature's weights unusable.  Status 2 alone, NaN outputs, iters 0; df and, in
    the second case, every other feature are what they are without the fault."""
    c = _de((3, 3), 70, 21)
    rng = np.random.default_rng(3)
    M = np.round(rng.normal(0.0, 1.0, (6, K)), 3)
    good = dict(c, M=M)
    M2 = M.copy()
    M2[:, K - 1] = M2[:, 0]
    got, _ = run_device(dict(c, M=M2))
    assert np.all(got["status"] == L.ST_SINGULAR) and np.all(got["iters"] == 0) and got["df"] == 2
    for k in ("loglik", "stat", "p_value", "q_value", "theta0", "theta1", "sigmasq0", "sigmasq1"):
        assert np.isnan(got[k]).all(), k
    assert_equal(got, L.lrt(c["y"], c["e"], M2, c["P0"], c["P1"], c["C"]), "collinear")
    if K == 5:
        return                                        # (6 samples do not carry 6 and 7 columns: the weights' case runs once)
    clean, _ = run_device(good)
    e = c["e"].copy()
    e[65, 2] = 1e200
    got, _ = run_device(dict(good, e=e))
    assert_equal(got, L.lrt(c["y"], e, M, c["P0"], c["P1"], c["C"]), "weights")
    assert np.all(got["status"][:, 65] == L.ST_SINGULAR) and np.isnan(got["loglik"][:, 65]).all() and np.isnan(got["p_value"][65])
    others = np.arange(70) != 65
    assert got["df"] == clean["df"]
    for k in ("loglik", "stat", "p_value", "theta0", "theta1", "sigmasq0", "sigmasq1", "iters", "status"):
        assert np.array_equal(got[k][..., others], clean[k][..., others]), k


# ----------------------------------------------------------------------------- the CLI
def cli_input(files, fixalpha=False, permute=False, seed=1234, rng_=None):
    """y, e, features as `mmdiff` hands them to the device: -range, then the normalisation, then -permute."""
    tabs = [R.read_table(f) for f in files]
    feats = tabs[0][0]
    y, e, uh = (np.stack([t[i] for t in tabs], 1) for i in (1, 2, 3))
    if rng_:
        sl = slice(rng_[0], rng_[1] + 1)
        feats, y, e, uh = feats[sl], y[sl], e[sl], uh[sl]
    S = len(files)
    y, _ = R.normalise(y, uh, max(0.2, float(S - S * S // 160) / float(S)))
    if permute:
        y, e = y.copy(), e.copy()
        for f in range(y.shape[0]):
            idx = R.permutation(seed & 0xFFFFFFFF, f, S)
            y[f], e[f] = y[f, idx], e[f, idx]
    return feats, y, e


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    y, e, uh, _ = synth(120, 6, seed=31, groups=[3, 3])
    y[7] = y[7, 0]
    return write_tables(tmp_path_factory.mktemp("lrt_tables"), y, e, uh)


def want_file(files, groups, **kw):
    fixalpha = kw.get("fixalpha", False)
    feats, y, e = cli_input(files, **kw)
    M, P0, P1, C = R.de_design(groups)
    return L.lrt_file(feats, L.lrt(y, e, M, P0, P1, C, fixalpha), M, P0, P1, fixalpha)


@pytest.mark.gpu
def test_cli_lrt_leaves_stdout_alone_and_writes_the_restatements_file(gpu, tmp_path, tables):
    plain, _ = cli(FAST + ["-de", "3", "3"] + tables)
    out = tmp_path / "de33.lrt"
    with_lrt, err = cli(FAST + ["-lrt", str(out), "-de", "3", "3"] + tables)
    assert with_lrt == plain and "Wrote the likelihood-ratio tests of 120 features" in err
    want = want_file(tables, (3, 3))
    assert out.read_text() == want
    only = tmp_path / "only.lrt"
    stdout, err = cli(["-lrt", str(only), "-lrtonly", "-de", "3", "3"] + tables)
    assert stdout == "" and only.read_text() == want and "BURNIN" not in err


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["permute", "range", "fixalpha", "de222"])
def test_cli_lrt_sees_the_chains_input(gpu, tmp_path, tables, case):
    out = tmp_path / "out.lrt"
    args, kw, groups = [], {}, (3, 3)
    if case == "permute":
        args, kw = ["-permute", "-seed", "77"], dict(permute=True, seed=77)
    elif case == "range":
        args, kw = ["-range", "10", "49"], dict(rng_=(10, 49))
    elif case == "fixalpha":
        args, kw = ["-fixalpha"], dict(fixalpha=True)
    else:
        groups = (2, 2, 2)
    stdout, _ = cli(args + ["-lrt", str(out), "-lrtonly", "-de"] + [str(g) for g in groups] + tables)
    assert stdout == ""
    text = out.read_text()
    assert text == want_file(tables, groups, **kw)
    assert text != want_file(tables, groups) or case == "de222"
    assert len(text.split("\n")) == (40 if case == "range" else 120) + 2
    if case == "de222":
        assert "\tnan\t" in text and text.split("\n")[1].split("\t")[-1] == "2"      # the collinear model 1: status 2, NaN
