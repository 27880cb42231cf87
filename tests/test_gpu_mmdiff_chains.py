"""`mmdiff -chains` on the device: every chain of a DiffChains handle against a seed-shifted single Diff handle (bitwise), the CLI's
chain tables and pooled table against the numpy restatement (tests/mmdiff_chains_ref.py, byte for byte), -chains 1 against the plain
run, chains that tune apart, the batch sums, edges, memory and reruns."""
import re

import numpy as np
import pytest

import mmdiff_chains_ref as CR
import mmdiff_ref as R
from test_gpu_mmdiff import cli, synth, write_tables

FAST = ["-burnin", "1024", "-iter", "1024", "-notune"]
SEED = (0x5A17 << 32) | 42          # high bits set: the chain is xored into them
COVARIATE = np.array([[0.3], [1.1], [-0.4], [0.9], [0.0], [-1.2]])


def read(path):
    with open(path) as f:
        return f.read()


def drive(h, burnin, max_batches, iters):
    h.burnin(burnin)
    nb = h.tune(max_batches) if max_batches else 0
    h.sample(iters)
    return nb


def assert_chain_is_single(h, c, args, seed, burnin, max_batches, iters, **kw):
    """Chain c of the driven handle h against Diff(seed ^ (c << 32)) driven the same way: batches, results and logit p' bitwise."""
    from mmseq_amd.diff import Diff
    d = Diff(*args, seed=seed ^ (c << 32), **kw)
    want_nb = drive(d, burnin, max_batches, iters)
    want, got = d.results(), h.results(c)
    assert h.info(c)["batches"] == d.info()["batches"] == want_nb, c
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), (c, k)
    d.close()
    return want_nb


def assert_pooled_is_the_restatement(h):
    """The handle's pooled columns against the restatement of k_dfc_pool on the handle's own chain results, bitwise."""
    res = [h.results(c) for c in range(h.C)]
    gb = [h.batch_sums(c) for c in range(h.C)]
    want = CR.pool([r["gamma_mean"] * float(h.T) for r in res], [r["logitp"] for r in res], gb, h.T)
    got = h.pooled()
    for k in ("log_bf", "log_bf_sd", "log_bf_mcse"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert np.array_equal(got["chains_mixed"], want["chains_mixed"])
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("covariate", [False, True])
def test_chain_c_is_a_seed_shifted_single_handle(gpu, covariate):
    """C = 3, F = 130 (two full blocks and two lanes), N = 6; burn-in 1024, tuning to its end under a cap of 64 batches, sampling 1024."""
    from mmseq_amd.diff import DiffChains
    y, e, _, _ = synth(130, 6, seed=31)
    M, P0, P1, C = R.de_design([3, 3])
    if covariate:
        M = COVARIATE
    h = DiffChains(y, e, M, P0, P1, C, 3, 1024, seed=SEED)
    nb = drive(h, 1024, 64, 1024)
    print("batches per chain:", nb)
    assert h.info(0)["Mnil"] == (not covariate)
    for c in range(3):
        assert assert_chain_is_single(h, c, (y, e, M, P0, P1, C), SEED, 1024, 64, 1024) == nb[c]
    h.pool()
    assert_pooled_is_the_restatement(h)
    h.close()


@pytest.mark.gpu
def test_chains_1_and_no_flag_are_byte_identical(gpu, tmp_path):
    y, e, uh, _ = synth(24, 6, seed=41)
    files = write_tables(tmp_path, y, e, uh)
    tail = ["-de", "3", "3"] + files
    plain = cli(FAST + tail)
    base1, base3 = str(tmp_path / "one"), str(tmp_path / "three")
    assert cli(FAST + ["-chains", "1"] + tail) == plain
    assert cli(FAST + ["-chains", "1", "-chainout", base1] + tail) == plain
    assert read(base1 + ".chain0.mmdiff") == plain[0]
    out, err = cli(FAST + ["-chains", "3", "-chainout", base3] + tail)
    assert read(base3 + ".chain0.mmdiff") == plain[0]
    assert read(base3 + ".chain1.mmdiff") != plain[0] and out != plain[0]
    assert "did not mix" not in err
    for c in range(3):
        assert "chain %d: sampling after 0 tuning batches\n" % c in err


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["plain", "permute", "fixalpha", "covariate"])
def test_chain_tables_and_pooled_table_equal_the_restatement(gpu, tmp_path, case):
    """-chains 3 -chainout with -burnin 1024 -iter 1024 -notune on 24 features: every chain table and the pooled stdout byte for byte,
    and the mixing warnings on stderr."""
    y, e, uh, _ = synth(24, 6, seed={"plain": 501, "permute": 502, "fixalpha": 503, "covariate": 504}[case])
    files = write_tables(tmp_path, y, e, uh)
    args, kw, design = list(FAST), {}, None
    if case == "fixalpha":
        args, kw = ["-fixalpha"] + args, dict(fixalpha=True)
    if case == "permute":
        args, kw = ["-permute", "-seed", "77"] + args, dict(permute=True, seed=77)
    if case == "covariate":
        C = np.array([[0, 0], [0, 0], [0, 0], [0, 1], [0, 1], [0, 1]])
        mat = tmp_path / "design.txt"
        mat.write_text("".join("%r\n" % float(v) for v in COVARIATE[:, 0]) + "\n" + "".join("%d %d\n" % tuple(c) for c in C) + "\n1\n\n0.5\n-0.5\n")
        design = (COVARIATE, np.ones((6, 1)), np.where(C[:, 1:] == 0, 0.5, -0.5), C)
        mode = ["-m", str(mat)]
    else:
        mode = ["-de", "3", "3"]
    base = str(tmp_path / "ch")
    out, err = cli(args + ["-chains", "3", "-chainout", base] + mode + files)
    want, chains, nb, cols = CR.mmdiff_chains(files, 3, groups=None if design else [3, 3], design=design, burnin=1024, iters=1024, tune=False, **kw)
    for c in range(3):
        assert read("%s.chain%d.mmdiff" % (base, c)) == chains[c], c
    assert out == want
    hdr = out.split("\n")[1].split("\t")
    assert hdr[-4:] == ["log_bf", "log_bf_sd", "log_bf_mcse", "chains_mixed"] and hdr[-5].startswith("sd_")
    assert out.split("\n")[0] == "#prior_probability=0.1"
    warned = [int(f) for f in re.findall(r"Warning: gamma mixed in \d of 3 chains for feature (\d+)\n", err)]
    assert warned == [f for f in range(24) if cols["chains_mixed"][f] < 3]
    assert "did not mix" not in err
    if case == "permute":
        rows = [[t.split("\n")[2 + f].split("\t")[-12:] for f in range(24)] for t in chains]
        assert rows[0] == rows[1] == rows[2]                 # every chain saw the same shuffled data (mu_*, sd_*)
        assert [r.split("\t")[-16:-4] for r in out.split("\n")[2:26]] == rows[0]
    if case == "covariate":
        assert "beta0_0\t" in out.split("\n")[1]


@pytest.mark.gpu
def test_chains_tune_apart(gpu):
    """The six features of test_gpu_mmdiff's tuning fixture: the restatement (run on a CPU when this fixture was chosen) tunes chains 0, 1
    and 2 of seed 1234 in 7, 29 and 21 batches.  The test asserts from the run itself that the counts differ, since otherwise the
    per-chain stream index is not exercised."""
    from mmseq_amd.diff import DiffChains
    y, e, _, _ = synth(6, 6, seed=200)
    args = (y, e) + R.de_design([3, 3])
    h = DiffChains(*args, 3, 1024, seed=1234)
    nb = drive(h, 1024, 1024, 1024)
    print("batches per chain:", nb)
    assert len(set(nb)) >= 2 and max(nb) < 1024, nb
    assert all(h.info(c)["ended"] for c in range(3))
    for c in range(3):
        assert assert_chain_is_single(h, c, args, 1234, 1024, 1024, 1024) == nb[c]
    h.close()


@pytest.mark.gpu
def test_batch_sums(gpu):
    from mmseq_amd._lib import MMGError
    from mmseq_amd.diff import DiffChains
    y, e, _, _ = synth(70, 6, seed=61)
    args = (y, e) + R.de_design([3, 3])

    def run(pieces):
        h = DiffChains(*args, 2, 1024, seed=7)
        h.burnin(1024)
        h.tune_batch()
        for n in pieces:
            h.sample(n)
        return h

    one, two = run([1024]), run([300, 724])
    for c in range(2):
        gb, r = one.batch_sums(c), one.results(c)
        assert np.array_equal(gb, np.floor(gb)) and gb.min() >= 0 and gb.max() <= 64
        assert np.array_equal(gb.sum(0), r["gamma_mean"] * 1024.0)
        assert 0 < gb.sum() < 1024 * 70 and len(set(gb.sum(1))) > 1          # gamma moves, and not every batch alike
        assert np.array_equal(two.batch_sums(c), gb)
        for k, v in two.results(c).items():
            assert np.array_equal(v, r[k], equal_nan=True), (c, k)
    with pytest.raises(MMGError) as ex:
        one.sample(16)
    assert ex.value.code == 1 and "total sampling length" in str(ex.value)
    part = run([512])
    with pytest.raises(MMGError) as ex:
        part.sample(513)
    assert ex.value.code == 1
    with pytest.raises(MMGError) as ex:
        part.pool()
    assert ex.value.code == 4
    part.sample(512)
    part.pool()
    one.pool()
    for k, v in part.pooled().items():
        assert np.array_equal(v, one.pooled()[k], equal_nan=True), k
    for h in (one, two, part):
        h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("F,C", [(1, 2), (1, 16), (65, 2), (65, 16)])
def test_edges_one_feature_one_lane_past_a_block_two_chains_and_the_cap(gpu, F, C):
    """Burn-in, two tuning batches, 256 iterations: chains against single handles, the pooled columns against the restatement, the memory
    against the documented formula."""
    from mmseq_amd.diff import Diff, DiffChains
    y, e, _, _ = synth(max(F, 5), 6, seed=700 + F)
    y, e = y[:F], e[:F]
    args = (y, e) + R.de_design([3, 3])
    h = DiffChains(*args, C, 256, seed=SEED)
    assert h.device_bytes() == CR.chains_device_bytes(F, 6, 1, 1, 1, 1, 2, True, C)
    h.burnin(1024)
    counts = [h.tune_batch()[0] for _ in range(2)]
    h.sample(256)
    for c in sorted({0, 1, C // 2, C - 1}):
        d = Diff(*args, seed=SEED ^ (c << 32))
        d.burnin(1024)
        assert [d.tune_batch() for _ in range(2)] == [n[c] for n in counts]
        d.sample(256)
        want, got = d.results(), h.results(c)
        for k in want:
            assert np.array_equal(got[k], want[k], equal_nan=True), (c, k)
        d.close()
    assert any(not np.array_equal(h.results(0)["alpha"], h.results(c)["alpha"]) for c in range(1, C))
    h.pool()
    assert_pooled_is_the_restatement(h)
    h.close()


@pytest.mark.gpu
def test_a_nil_p1_and_a_pseudoprior_that_is_not_finite(gpu):
    """P1 a constant column (nil: no etas in model 1, only the variance classes differ), as a chains handle against single handles; and
    pdash = 0 without tuning: logit p' is -inf in every chain and the pooled statistics are NaN."""
    from mmseq_amd.diff import DiffChains
    y, e, _, _ = synth(65, 6, seed=81)
    M, P0, _, C = R.de_design([3, 3])
    args = (y, e, M, P0, np.ones((6, 1)), C)
    h = DiffChains(*args, 2, 256, seed=3)
    assert h.info(1)["Pnil"] == (True, True)
    assert h.device_bytes() == CR.chains_device_bytes(65, 6, 1, 1, 1, 1, 2, True, 2)
    drive(h, 1024, 2, 256)
    for c in range(2):
        assert_chain_is_single(h, c, args, 3, 1024, 2, 256)
    h.pool()
    assert_pooled_is_the_restatement(h)
    h.close()
    h = DiffChains(*((y, e) + R.de_design([3, 3])), 2, 256, pdash=0.0)
    drive(h, 1024, 0, 256)
    h.pool()
    got = assert_pooled_is_the_restatement(h)
    assert all(np.isnan(got[k]).all() for k in ("log_bf", "log_bf_sd", "log_bf_mcse")) and (got["chains_mixed"] == 0).all()
    h.close()


@pytest.mark.gpu
def test_reruns_of_the_whole_handle_are_bit_identical(gpu):
    from mmseq_amd.diff import DiffChains
    y, e, _, _ = synth(130, 6, seed=91)
    args = (y, e) + R.de_design([3, 3])

    def run():
        h = DiffChains(*args, 4, 512, seed=SEED)
        nb = drive(h, 1024, 8, 512)
        h.pool()
        out = (nb, [h.results(c) for c in range(4)], [h.batch_sums(c) for c in range(4)], h.pooled())
        h.close()
        return out

    a, b = run(), run()
    assert a[0] == b[0]
    for c in range(4):
        assert np.array_equal(a[2][c], b[2][c])
        for k in a[1][c]:
            assert np.array_equal(a[1][c][k], b[1][c][k], equal_nan=True), (c, k)
    for k in a[3]:
        assert np.array_equal(a[3][k], b[3][k], equal_nan=True), k
