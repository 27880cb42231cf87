"""CPU checks of tests/sim_ref.py, the restatement of mmg_sim_* and of the mmsim CLI's rules, against independent formulas on random
data: distances from explicit differences, correlations from np.corrcoef, the centre leaving the distances alone, the nearest
neighbours' counts and ties, the degenerate cases, and the rank, percentile and offset rules against the other restatements."""
import numpy as np
import pytest

import fold_ref
import mmdiff_ref
import sim_ref as R


def _traces(rng, S, F, T):
    return np.exp(rng.normal(-3.0, 2.0, F)[None, None, :] + 0.5 * rng.normal(0.0, 1.0, (S, T, F)))


@pytest.fixture(scope="module")
def five():
    rng = np.random.default_rng(1)
    S, F, T = 5, 500, 7
    v = _traces(rng, S, F, T)
    offs = list(rng.normal(0.0, 0.3, S))
    centre = rng.normal(-3.0, 1.0, F)
    ranks = [0, 3, 6, 3, 7]
    return v, offs, centre, ranks, R.sim_ref(v, offs, ranks, centre=centre)


def test_distance_is_the_rms_difference_and_correlation_is_corrcoef(five):
    v, offs, centre, ranks, ref = five
    S, T, F = v.shape
    z = ref["z"]
    assert ref["n"] == F and ref["used"].all() and ref["status"] == 0 and (ref["pair_status"] == 0).all()
    assert np.array_equal(z, ((R.dlog(v.ravel()).reshape(v.shape) + np.array(offs)[:, None, None]) - centre[None, None, :]) + 0.0)
    for p, (a, b) in enumerate(R.pairs_of(S)):
        D = np.array([np.sqrt(np.mean((z[a, t] - z[b, t]) ** 2)) for t in range(T)])
        C = np.array([np.corrcoef(z[a, t], z[b, t])[0, 1] for t in range(T)])
        assert abs(ref["mean_D"][p] - D.mean()) <= 1e-10 * D.mean()
        assert abs(ref["mean_R"][p] - C.mean()) <= 1e-10 * abs(C.mean())
        assert np.allclose(ref["q_D"][p, :3], np.sort(D)[[0, 3, 6]], rtol=1e-10, atol=0)
        assert np.allclose(ref["q_R"][p, :3], np.sort(C)[[0, 3, 6]], rtol=1e-10, atol=0)
        assert ref["q_D"][p, 1] == ref["q_D"][p, 3] and np.isnan(ref["q_D"][p, 4]) and np.isnan(ref["q_R"][p, 4])
        assert abs(ref["sd_D"][p] - D.std(ddof=1)) <= 1e-8 * D.std(ddof=1)
        assert abs(ref["sd_R"][p] - C.std(ddof=1)) <= 1e-8 * C.std(ddof=1)


def test_the_centre_leaves_the_distances_alone(five):
    v, offs, centre, ranks, ref = five
    bare = R.sim_ref(v, offs, ranks)
    assert np.allclose(bare["mean_D"], ref["mean_D"], rtol=1e-10, atol=0) and np.allclose(bare["q_D"][:, :3], ref["q_D"][:, :3], rtol=1e-10, atol=0)
    assert not np.allclose(bare["mean_R"], ref["mean_R"], rtol=1e-3, atol=0)       # the raw correlation is another number


def test_nearest_neighbour_counts(five):
    v, offs, centre, ranks, ref = five
    S, T, F = v.shape
    assert (ref["nn"].sum(axis=1) == T).all() and (np.diag(ref["nn"]) == 0).all()
    z = ref["z"]
    want = np.zeros((S, S), np.uint32)
    for t in range(T):
        for a in range(S):
            d = [np.inf if b == a else np.sum((z[a, t] - z[b, t]) ** 2) for b in range(S)]
            want[a, int(np.argmin(d))] += 1
    assert np.array_equal(ref["nn"], want)
    assert np.array_equal(ref["p_nearest"], want / float(T))


def test_ties_go_to_the_smallest_index():
    # three draws of four samples on integers: 1 and 2 are equally far from 0, 3 is a copy of 2
    z = np.zeros((4, 3, 6))
    z[1, :, 0] = 2.0
    z[2, :, 1] = 2.0
    z[3] = z[2]
    G = np.einsum("rtf,stf->trs", z, z)
    m = z.sum(axis=2).T
    out = R.summary_from_gram(G, m, 6, [])
    assert list(out["nn"][0]) == [0, 3, 0, 0]                  # 1, 2 and 3 tie: the smallest
    assert list(out["nn"][1]) == [3, 0, 0, 0]
    assert list(out["nn"][2]) == [0, 0, 0, 3] and list(out["nn"][3]) == [0, 0, 3, 0]
    p23 = R.pairs_of(4).index((2, 3))
    assert out["mean_D"][p23] == 0.0 and out["mean_R"][p23] == 1.0
    assert out["pair_status"][R.pairs_of(4).index((0, 1))] == R.PAIR_NO_R            # sample 0 is constant: no correlation with it


def test_invalid_values_and_the_mask_decide_the_used_features():
    rng = np.random.default_rng(2)
    v = _traces(rng, 3, 30, 4)
    v[0, 1, 3] = 0.0; v[1, 0, 4] = -1.0; v[2, 3, 5] = np.nan; v[0, 0, 6] = np.inf
    mask = np.ones(30, np.uint8)
    mask[[0, 3]] = 0
    z, used, n = R.values(v, [0.0, 0.0, 0.0], mask=mask)
    assert n == 25 and list(np.flatnonzero(used == 0)) == [0, 3, 4, 5, 6] and (z[:, :, used == 0] == 0.0).all()
    lz, lused, ln = R.values(np.where(v == 0.0, -2.0, v), [0.0] * 3, logged=True)   # logged: zero and negative values are in order
    assert ln == 28 and list(np.flatnonzero(lused == 0)) == [5, 6]
    G, m = R.gram(z, used)
    assert np.allclose(G.astype(np.float64), np.einsum("rtf,stf->trs", z, z), rtol=1e-12)


@pytest.mark.parametrize("keep", [0, 1])
def test_fewer_than_two_features_give_nan(keep):
    rng = np.random.default_rng(3)
    v = _traces(rng, 3, 10, 5)
    mask = np.zeros(10, np.uint8)
    mask[:keep] = 1
    out = R.sim_ref(v, [0.0] * 3, [0, 4], mask=mask)
    assert out["n"] == keep and out["status"] == R.FEW_FEATURES and (out["nn"] == 0).all() and (out["pair_status"] == 0).all()
    for k in ("mean_D", "ss_D", "q_D", "mean_R", "ss_R", "q_R", "sd_D", "sd_R"):
        assert np.isnan(out[k]).all(), k


def test_rank_percentile_and_offset_rules_match_the_other_restatements():
    from mmseq_amd import similarity
    for T in (1, 2, 16, 1000, 1024, 4096):
        for p in (0, 2.5, 12.5, 50, 97.5, 100):
            assert R.percentile_rank(p, T) == fold_ref.percentile_rank(p, T) == similarity.percentile_rank(p, T)
    assert R.percentile_rank(50, 16) == 8 and R.percentile_rank(2.5, 1024) == 26
    assert [R.default_uhfrac(S) for S in (2, 12, 13, 40, 160, 256)] == [1.0, 1.0, 12.0 / 13.0, 0.75, 0.2, 0.2]
    rng = np.random.default_rng(4)
    F, S = 150, 4
    y = rng.normal(1.0, 1.0, (F, S)) + np.array([0.0, 0.4, -0.3, 0.1])
    uh = rng.integers(0, 3, (F, S))
    for frac in (None, 0.5):
        offs, n = R.offsets(y, uh, frac)
        ny, factors = mmdiff_ref.normalise(y, uh.astype(float), R.default_uhfrac(S) if frac is None else frac)
        if factors is None:
            assert n is None and offs == [0.0] * S
        else:
            assert n >= 100 and offs == [-f for f in factors] and np.array_equal(ny, y + np.array(offs))
    offs, n = R.offsets(y, uh, 0.5)
    assert n is not None
    assert R.offsets(y[:99], np.ones((99, S)), 0.5) == ([0.0] * S, None)             # fewer than 100 features: skipped
    traced = np.ones((F, S), bool)
    traced[3, 1] = False
    y2 = y.copy()
    y2[5, 2] = np.nan
    mask = R.feature_mask(y2, uh, traced, uhmin=1)
    assert not mask[3] and not mask[5] and np.array_equal(mask, (uh >= 1).all(axis=1) & (np.arange(F) != 3) & (np.arange(F) != 5))
    c = R.centre_of(y2, offs, mask)
    assert (c[~mask] == 0.0).all() and np.allclose(c[mask], (y2[mask] + np.array(offs)).mean(axis=1), rtol=1e-14)


def test_table_and_matrix_texts(five):
    v, offs, centre, ranks, ref = five
    bases = ["s%d" % i for i in range(5)]
    out = dict(ref)
    out["q_D"], out["q_R"] = ref["q_D"][:, :1], ref["q_R"][:, :1]
    text = R.table(bases, "gene", 7, 500, 500, offs, "mean", [0.0], out).decode().splitlines()
    assert text[1:5] == ["# level: gene", "# T: 7", "# features: 500/500", "# centre: mean"] and text[5].startswith("# sample 0: s0 offset ")
    assert text[10] == "sample_a\tsample_b\tdist\tdist_sd\tdist_percentiles0\tcor\tcor_sd\tcor_percentiles0\tnearest_a\tnearest_b\tstatus"
    assert len(text) == 11 + 10 and text[11].split("\t")[:2] == ["s0", "s1"] and text[11].split("\t")[-1] == "0"
    M = [line.split("\t") for line in R.matrix(bases, out).decode().splitlines()]
    assert M[0] == [""] + bases and all(M[1 + i][1 + i] == "0" for i in range(5)) and M[1][2] == M[2][1] == R.fmt(ref["mean_D"][0])
