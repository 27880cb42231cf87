"""`mmdiff -permutations` on the device: every replica of a DiffPerm handle against a single Diff handle on that replica's restated
data with the seed seed ^ (b << 32) (bitwise), the log Bayes factors against numpy, the q-values against the restatement
(tests/qvalue_ref.py) applied to the handle's own statistics (bitwise), replicas that tune apart, edges, memory, reruns, call-order
errors, and the CLI's stdout and -permout tables against tests/mmdiff_perm_ref.py byte for byte."""
import numpy as np
import pytest

import mmdiff_perm_ref as PR
import mmdiff_ref as R
import qvalue_ref as Q
from test_gpu_mmdiff import cli, synth, write_tables

FAST = ["-burnin", "1024", "-iter", "1024", "-notune"]
SEED = (0x5A17 << 32) | 42          # high bits set: the replica is xored into them
COVARIATE = np.array([[0.3], [1.1], [-0.4], [0.9], [0.0], [-1.2]])


def read(path):
    with open(path) as f:
        return f.read()


def drive(h, burnin, max_batches, iters):
    h.burnin(burnin)
    nb = h.tune(max_batches) if max_batches else 0
    h.sample(iters)
    return nb


def assert_replica_is_single(h, b, y, e, design, seed, burnin, max_batches, iters, **kw):
    """Replica b of the driven handle h against Diff on the restated data of replica b with seed ^ (b << 32), driven the same way:
    batches, results and logit p' bitwise."""
    from mmseq_amd.diff import Diff
    yb, eb = PR.replica_data(y, e, seed, b)
    if b:
        assert np.array_equal(np.sort(yb, 1), np.sort(y, 1)) and np.array_equal(np.sort(eb, 1), np.sort(e, 1))
    d = Diff(yb, eb, *design, seed=seed ^ (b << 32), **kw)
    want_nb = drive(d, burnin, max_batches, iters)
    want, got = d.results(), h.results(b)
    assert h.info(b)["batches"] == d.info()["batches"] == want_nb, b
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), (b, k)
    d.close()
    return want_nb


def assert_qvalues(h):
    """The handle's statistics against numpy's log(g) - log1p(-g) - logit p' (relative 1e-12, the bar of the project's fp64
    restatements of device arithmetic; the infinities and NaN in the same places, NaN where logit p' is not finite), bitwise against
    the restatement with the library's own log; q and null_ge bitwise against the restatement applied to the handle's own statistics."""
    out = h.qvalues()
    stat = out["stat"]
    assert stat.shape == (h.R, h.F)
    for b in range(h.R):
        r = h.results(b)
        g, o = r["gamma_mean"], r["logitp"]
        with np.errstate(all="ignore"):
            want = np.where(np.isfinite(o), np.log(g) - np.log1p(-g) - o, np.nan)
        assert np.array_equal(np.isnan(stat[b]), np.isnan(want)), b
        assert np.array_equal(stat[b] == np.inf, want == np.inf) and np.array_equal(stat[b] == -np.inf, want == -np.inf), b
        assert np.array_equal(stat[b] == -np.inf, np.isfinite(o) & (g == 0.0)) and np.array_equal(stat[b] == np.inf, np.isfinite(o) & (g == 1.0))
        fin = np.isfinite(want)
        assert np.allclose(stat[b][fin], want[fin], rtol=1e-12, atol=0.0), b
        assert np.array_equal(stat[b], PR.statistic(g, o), equal_nan=True), b
    ge, q = Q.qvalues(stat[0], stat[1:].ravel())
    assert np.array_equal(out["null_ge"], ge) and np.array_equal(out["q"], q, equal_nan=True)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("covariate", [False, True])
def test_replica_b_is_a_single_handle_on_the_shuffled_data(gpu, covariate):
    """B = 3, F = 130 (two full blocks and two lanes), N = 6; burn-in 1024, tuning to its end under a cap of 64 batches, sampling 1024."""
    from mmseq_amd.diff import DiffPerm
    y, e, _, _ = synth(130, 6, seed=31)
    M, P0, P1, C = R.de_design([3, 3])
    if covariate:
        M = COVARIATE
    h = DiffPerm(y, e, M, P0, P1, C, 3, seed=SEED)
    assert h.device_bytes() == PR.perm_device_bytes(130, 6, 1, 1, 1, 1, 2, not covariate, 3)
    nb = drive(h, 1024, 64, 1024)
    print("batches per replica:", nb)
    assert h.info(0)["Mnil"] == (not covariate)
    for b in range(4):
        assert assert_replica_is_single(h, b, y, e, (M, P0, P1, C), SEED, 1024, 64, 1024) == nb[b]
    out = assert_qvalues(h)
    assert np.isfinite(out["stat"]).any() and (out["q"] <= 1).all()
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F,B", [(1, 1), (1, 31), (65, 1), (65, 31)])
def test_edges_one_feature_one_lane_past_a_block_one_shuffle_and_the_cap(gpu, F, B):
    """Burn-in, two tuning batches, 256 iterations: replicas against single handles, the q-values against the restatement, the memory
    against the documented formula."""
    from mmseq_amd.diff import DiffPerm
    y, e, _, _ = synth(max(F, 5), 6, seed=700 + F)
    y, e = y[:F], e[:F]
    design = R.de_design([3, 3])
    h = DiffPerm(y, e, *design, B, seed=SEED)
    assert h.R == B + 1 and h.device_bytes() == PR.perm_device_bytes(F, 6, 1, 1, 1, 1, 2, True, B)
    nb = drive(h, 1024, 2, 256)
    for b in sorted({0, 1, (B + 1) // 2, B}):
        assert assert_replica_is_single(h, b, y, e, design, SEED, 1024, 2, 256) == nb[b]
    assert any(not np.array_equal(h.results(0)["alpha"], h.results(b)["alpha"]) for b in range(1, B + 1))
    assert_qvalues(h)
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("groups", [[1, 1], [3, 4]], ids=["N2", "N7"])
def test_two_samples_take_one_draw_and_an_odd_number_of_samples(gpu, groups):
    from mmseq_amd.diff import DiffPerm
    N = sum(groups)
    y, e, _, _ = synth(70, N, seed=800 + N)
    design = R.de_design(groups)
    h = DiffPerm(y, e, *design, 5, seed=77)
    nb = drive(h, 1024, 2, 256)
    for b in range(6):
        assert assert_replica_is_single(h, b, y, e, design, 77, 1024, 2, 256) == nb[b]
    if N == 2:      # one draw per feature: every shuffle either keeps or swaps the two samples, and over 5 x 70 draws both happen
        swapped = [int(np.array_equal(PR.replica_data(y, e, 77, b)[0][f], y[f, ::-1])) for b in range(1, 6) for f in range(70)]
        assert 0 < sum(swapped) < len(swapped)
    assert_qvalues(h)
    h.close()


@pytest.mark.gpu
def test_statistics_that_are_infinite_and_a_pseudoprior_that_is_not_finite(gpu):
    """64 sampling iterations leave gamma means of exactly 0 (and, with the planted effects, of 1): -inf and +inf.  pdash = 0 without
    tuning: logit p' is -inf in every replica, every statistic NaN, and so is every q-value."""
    from mmseq_amd.diff import DiffPerm
    y, e, _, _ = synth(200, 6, seed=91, effect=4.0)
    design = R.de_design([3, 3])
    h = DiffPerm(y, e, *design, 2, seed=SEED)
    drive(h, 1024, 1, 64)
    out = assert_qvalues(h)
    assert (out["stat"] == -np.inf).any() and (out["stat"][0] == np.inf).any()
    h.close()
    h = DiffPerm(y[:65], e[:65], *design, 2, pdash=0.0)
    drive(h, 1024, 0, 64)
    out = assert_qvalues(h)
    assert np.isnan(out["stat"]).all() and np.isnan(out["q"]).all() and (out["null_ge"] == 0).all()
    h.close()


@pytest.mark.gpu
def test_tuning_as_driven_and_replicas_that_tune_apart(gpu):
    """The six features of test_gpu_mmdiff's tuning fixture.  Without tuning every replica has 0 batches, under a cap of 1 every replica
    has 1.  Tuned to the end, a replica that ends before the others leaves the tuning launches and
    samples from its own stream index: every replica equals the single handle, which tunes alone."""
    from mmseq_amd.diff import DiffPerm
    y, e, _, _ = synth(6, 6, seed=200)
    design = R.de_design([3, 3])
    for cap in (0, 1):
        h = DiffPerm(y, e, *design, 2, seed=1234)
        drive(h, 1024, cap, 256)
        assert [h.info(b)["batches"] for b in range(3)] == [cap] * 3
        for b in range(3):
            assert_replica_is_single(h, b, y, e, design, 1234, 1024, cap, 256)
        h.close()
    h = DiffPerm(y, e, *design, 2, seed=1234)
    nb = drive(h, 1024, 1024, 1024)
    print("batches per replica:", nb)
    for b in range(3):
        assert assert_replica_is_single(h, b, y, e, design, 1234, 1024, 1024, 1024) == nb[b]
        if nb[b] < max(nb):      # it left the tuning launches before the others, and sampled from its own stream index
            assert h.info(b)["ended"]
    h.close()


@pytest.mark.gpu
def test_reruns_of_the_whole_handle_are_bit_identical(gpu):
    from mmseq_amd.diff import DiffPerm
    y, e, _, _ = synth(130, 6, seed=91)
    design = R.de_design([3, 3])

    def run():
        h = DiffPerm(y, e, *design, 4, seed=SEED)
        nb = drive(h, 1024, 8, 512)
        out = (nb, [h.results(b) for b in range(5)], h.qvalues())
        h.close()
        return out

    a, b = run(), run()
    assert a[0] == b[0]
    for r in range(5):
        for k in a[1][r]:
            assert np.array_equal(a[1][r][k], b[1][r][k], equal_nan=True), (r, k)
    for k in a[2]:
        assert np.array_equal(a[2][k], b[2][k], equal_nan=True), k


@pytest.mark.gpu
def test_call_order_and_argument_errors(gpu):
    import ctypes as C
    from mmseq_amd._lib import MMGError, load
    from mmseq_amd.diff import DiffPerm
    y, e, _, _ = synth(10, 6, seed=5)
    design = R.de_design([3, 3])
    for n_perm in (0, 32):
        with pytest.raises(MMGError) as ex:
            DiffPerm(y, e, *design, n_perm)
        assert ex.value.code == 1 and "between 1 and 31" in str(ex.value)
    h = DiffPerm(y, e, *design, 2)
    with pytest.raises(MMGError) as ex:
        h.qvalues()
    assert ex.value.code == 4
    h.burnin(1024)
    with pytest.raises(MMGError) as ex:
        h.qvalues()
    assert ex.value.code == 4
    with pytest.raises(MMGError) as ex:
        h.results(0)
    assert ex.value.code == 4
    assert load().mmg_diff_perm_get_qvalues(h._h, None, None, None) == 4
    h.sample(64)
    assert load().mmg_diff_perm_get_qvalues(h._h, None, None, None) == 4      # sampled, but mmg_diff_perm_qvalues has not run
    for b in (3, 31, 1 << 20):
        with pytest.raises(MMGError) as ex:
            h.results(b)
        assert ex.value.code == 1
        with pytest.raises(MMGError) as ex:
            h.info(b)
        assert ex.value.code == 1
    h.qvalues()
    assert load().mmg_diff_perm_get_qvalues(h._h, None, None, None) == 0
    q = np.empty(10)
    assert load().mmg_diff_perm_get_qvalues(h._h, None, None, q.ctypes.data_as(C.c_void_p)) == 0 and ((q >= 0) & (q <= 1)).all()
    with pytest.raises(MMGError) as ex:
        h.tune_batch()
    assert ex.value.code == 4
    h.close()


@pytest.mark.gpu
def test_cli_stdout_and_permout_tables_equal_the_restatement(gpu, tmp_path):
    """F = 24, N = 6, B = 2 with -burnin 1024 -iter 1024 -notune: stdout without its last two columns is the run without the flag, byte
    for byte; the whole stdout and both -permout tables are the restatement's."""
    y, e, uh, _ = synth(24, 6, seed=41)
    files = write_tables(tmp_path, y, e, uh)
    tail = ["-de", "3", "3"] + files
    plain, plain_err = cli(FAST + tail)
    base = str(tmp_path / "null")
    out, err = cli(FAST + ["-permutations", "2", "-permout", base] + tail)
    rows = out.split("\n")
    assert rows[0] == "#prior_probability=0.1" and rows[1].split("\t")[-2:] == ["perm_ge", "q_value"] and rows[-1] == ""
    assert "\n".join([rows[0]] + ["\t".join(r.split("\t")[:-2]) for r in rows[1:-1]] + [""]) == plain
    assert [ln for ln in err.split("\n") if "did not mix" in ln] == [ln for ln in plain_err.split("\n") if "did not mix" in ln]
    for b in range(3):
        assert "replica %d: sampling after 0 tuning batches\n" % b in err
    want, tables, (stat, ge, q) = PR.mmdiff_perm(files, 2, groups=[3, 3], burnin=1024, iters=1024)
    assert out == want
    for b in (1, 2):
        t = read("%s.perm%d.mmdiff" % (base, b))
        assert t == tables[b - 1], b
        assert t.split("\n")[1] == plain.split("\n")[1] and t != plain
    assert [int(r.split("\t")[-2]) for r in rows[2:-1]] == list(ge)
