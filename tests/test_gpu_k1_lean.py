"""The single-chain sample launch: the lean instantiation of k_sample_sell (sell_kernels.h: LEAN -- lists of register-path and empty
tiles only) against the general one and the oracle, and the ranges of a launch cut by what a tile costs (mmgibbs.hip: RANGE_*).

Every chain comparison is exact equality with the oracle's sequential replay of the stored rows: counts, every redrawn mu (the trace
keeps all iterations), the moments.  Every test reads from mmg_problem_k1_info_get which instantiation the launch runs, so a silent
fall-back to the general kernel cannot pass.

MMG_OPT_K1_RANGES makes the ranges long on small inputs (a 256-CU device otherwise gives every tile of these problems a workgroup
of its own): the steady state of the kernel's pipeline, both tiles of the unrolled pair, slides inside a range.

The synthetic problem of the range tests, 60 000 rows x 3 000 transcripts with 1 + Poisson(19) hits: 959 tiles in 47 bands of 1 ... 118
tiles (the generator's abundances are skewed); the bands of 16 tiles and more run from at most 4 to at least 7 groups per tile, the
small ones cannot (test_range_problem_has_the_spread_the_pricing_test_needs checks it on the CPU).  56 ranges of about 17 tiles: the
cutter ends a range at the first tile that reaches its share of the total, so a range misses the mean by less than one tile -- at most
6 + 12 = 18 of a mean of 199, 9.1 %: the 10 % bound is a property of the cutter on this problem, not a measurement."""
import numpy as np
import pytest

import ladder_problem as lp

SEED = 91
N_ITER = 8
N_RANGES = 56
RANGE_OPTS = dict(sample_kernel=2, derive_order=0, k1_ranges=N_RANGES)


def _range_problem(orc):
    q, _ = orc.synth_problem(R=60000, T=3000, avg_hits=20, seed=1234, sort=False)
    return q


def test_range_problem_has_the_spread_the_pricing_test_needs(orc):
    q = _range_problem(orc)
    (rp, ci, kk), t = lp.stored_tiles(orc, q.row_ptr, q.col_idx, None)
    assert kk is None and t["fast"].all() and not t["far"].any()
    key = (orc.row_keys(rp, orc.sort_hits(rp, ci), kk)[0] >> np.uint64(18))[t["r0"]]
    big = 0
    for b in np.unique(key):
        ng = t["ng"][key == b]
        if ng.size >= 16:
            big += 1
            assert ng.min() <= 4 and ng.max() >= 7, (int(b), ng.size, int(ng.min()), int(ng.max()))
    assert big >= 10
    assert int(t["ng"].max()) <= 12                   # the bound of the docstring: a tile costs at most 18


@pytest.fixture(scope="module")
def ranged(gpu, orc):
    """The range problem on the device under RANGE_OPTS with lean forced off and on, the stored rows, the oracle's chains (lazily)."""
    q = _range_problem(orc)
    probs = {}
    for lean in (0, 1):
        with gpu.options(k1_lean=lean, **RANGE_OPTS):
            probs[lean] = gpu.Problem.from_csr(q.row_ptr, q.col_idx, q.l)
    rp, ci = probs[1].download()
    want_rp, want_ci, _, _ = orc.canonical_layout(q.row_ptr, q.col_idx)
    assert np.array_equal(rp, want_rp) and np.array_equal(ci, want_ci)
    ps = orc.Problem(rp, ci, q.l)
    mu0, _ = probs[1].start_values()
    refs = {}

    def ref(chain):
        if chain not in refs:
            refs[chain] = orc.gibbs_keyed(ps, mu0, seed=SEED, chain=chain, n_iter=N_ITER, trace_len=N_ITER)
        return refs[chain]
    return probs, mu0, ref


def _assert_chain(gpu, prob, mu0, ref, n_chains=1):
    s = gpu.Sampler(prob, mu0, seed=SEED, n_chains=n_chains, gibbs_iter=N_ITER, trace_len=N_ITER)
    s.run(N_ITER)
    for c in range(n_chains):
        r = ref(c)
        assert np.array_equal(s.counts(c), r["cnt"]), c
        assert np.array_equal(s.trace(c), r["trace"]), c
        assert np.array_equal(s.mu(c), r["mu"]), c
        sl, sl2 = s.moments(c)[:2]
        assert np.array_equal(sl, r["sum_log"]) and np.array_equal(sl2, r["sum_log2"]), c


@pytest.mark.gpu
@pytest.mark.parametrize("variant,lean", [("long", 0), ("long", 1), ("short", 0), ("short", 1)])
def test_ladder_lean_on_and_off_equal_the_oracle(gpu, orc, variant, lean):
    """Every group count from 1 to 12, tiles of 64, 63, 17 and 1 rows, window slides; 3 ranges of 2 P tiles and more.  "long" runs the
    generic walk, "short" the straight-line walk for every group count."""
    P = lp.period_tiles(variant)
    rp, ci, l, k, mu0 = lp.ladder(lp.periods_for(variant, 3 * 2 * P + P), variant, seed=11)
    assert k is None
    (srp, sci, sk), t = lp.stored_tiles(orc, rp, ci, None)
    assert set(range(1, 10)) | {12} <= set(t["ng"].tolist()) and {64, 63, 17, 1} <= set(t["nrows"].tolist()) and t["slid"].sum() > 8
    with gpu.options(sample_kernel=2, derive_order=0, k1_ranges=3, k1_lean=lean):
        prob = gpu.Problem.from_csr(rp, ci, l)
    got_rp, got_ci = prob.download()
    assert np.array_equal(got_rp, srp) and np.array_equal(got_ci, sci)
    inf, k1 = prob.info, prob.k1_info
    assert inf.sample_kernel == 2 and inf.sample_grid == 3 and inf.fast_tiles == t["r0"].size
    assert k1.lean == lean and k1.fixed_walk == (variant == "short") and k1.range_tiles_max >= 2 * P
    ps = orc.Problem(srp, sci, l)
    ref = orc.gibbs_keyed(ps, mu0, seed=SEED, chain=0, n_iter=N_ITER, trace_len=N_ITER)
    _assert_chain(gpu, prob, mu0, lambda c: ref)


@pytest.mark.gpu
@pytest.mark.parametrize("lean", [0, 1])
def test_length_spread_chain_equals_the_oracle(gpu, ranged, lean):
    probs, mu0, ref = ranged
    assert probs[lean].k1_info.lean == lean and probs[lean].info.sample_kernel == 2
    _assert_chain(gpu, probs[lean], mu0, ref)


@pytest.mark.gpu
def test_ranges_are_balanced_by_the_groups_of_their_tiles(gpu, ranged):
    prob = ranged[0][1]
    k1 = prob.k1_info
    bound, cum, grp = prob.k1_ranges()
    tiles = np.diff(bound.astype(np.int64))
    cost = np.diff(cum.astype(np.int64))
    print("\nranges %d, cost max %d mean %.1f (max / mean %.4f), tiles per range %d ... %d" %
          (k1.n_ranges, k1.range_cost_max, k1.range_cost_mean, k1.range_cost_max / k1.range_cost_mean, tiles.min(), tiles.max()))
    assert k1.lean == 1 and k1.range_tile_cost >= 1 and k1.n_ranges == N_RANGES == tiles.size
    assert np.array_equal(cost, k1.range_tile_cost * tiles + np.diff(grp.astype(np.int64)))   # v per tile + 1 per group
    assert k1.range_cost_max == cost.max() and abs(k1.range_cost_mean - cost.mean()) < 1e-9 * cost.mean()
    assert k1.range_cost_max <= 1.10 * k1.range_cost_mean
    # the pricing follows the groups: some range is not what its tile count makes of the mean tile
    per_tile = k1.list_cost / float(k1.n_list)
    dev = np.abs(cost - tiles * per_tile) / (tiles * per_tile)
    print("largest deviation of a range's cost from tiles x mean cost per tile: %.3f" % dev.max())
    assert dev.max() > 0.10
    # the constant model, for the A/B, still cuts as it did: equal tile counts
    with gpu.options(k1_range_cost=0, **RANGE_OPTS):
        q = gpu.Problem.from_csr(*_csr_of(prob))
    assert q.k1_info.range_tile_cost == 0
    t0 = np.diff(q.k1_ranges()[0].astype(np.int64))
    assert t0.max() - t0.min() <= 1


def _csr_of(prob):
    rp, ci = prob.download()
    return rp, ci, prob.l()


@pytest.mark.gpu
def test_partial_last_window(gpu, orc):
    """n = 1000 is no multiple of 64: the last band's window reaches past the transcripts."""
    q, _ = orc.synth_problem(R=20000, T=1000, avg_hits=8, seed=5, sort=False)
    with gpu.options(sample_kernel=2, derive_order=0, k1_ranges=8, k1_lean=1):
        prob = gpu.Problem.from_csr(q.row_ptr, q.col_idx, q.l)
    rp, ci = prob.download()
    assert int(ci.max()) >= 1000 - 8 and prob.k1_info.lean == 1 and prob.info.sample_grid == 8
    ps = orc.Problem(rp, ci, q.l)
    mu0, _ = prob.start_values()
    ref = orc.gibbs_keyed(ps, mu0, seed=SEED, chain=0, n_iter=N_ITER, trace_len=N_ITER)
    _assert_chain(gpu, prob, mu0, lambda c: ref)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["far", "k"])
def test_other_tiles_keep_the_general_kernel(gpu, orc, kind):
    """2 % far rows, and a k array: not lean by itself, and forcing lean is refused when the problem is built -- nothing is launched."""
    from mmseq_amd._lib import MMGError
    if kind == "far":
        q, _ = orc.synth_problem(R=20000, T=3000, avg_hits=8, seed=7, sort=False, far_fraction=0.02)
        args, k = (q.row_ptr, q.col_idx, q.l), None
    else:
        rp, ci, l, k, _ = lp.ladder(2, "k", seed=11)
        args = (rp, ci, l)
    with gpu.options(sample_kernel=2, derive_order=0):
        prob = gpu.Problem.from_csr(*args, k=k)
    inf = prob.info
    assert inf.sample_kernel == 2 and prob.k1_info.lean == 0
    if kind == "far":
        assert inf.far_tiles > 0
    def held():
        c = np.zeros(3, np.int64)
        gpu.check(gpu._lib.load().mmg_selftest_live(c.ctypes.data))
        return c.tolist()
    live = held()
    with gpu.options(sample_kernel=2, derive_order=0, k1_lean=1):
        with pytest.raises(MMGError) as e:
            gpu.Problem.from_csr(*args, k=k)
    assert e.value.code == 1 and "MMG_OPT_K1_LEAN" in str(e.value)
    assert held() == live                                                       # the refused builds gave back what they held


@pytest.mark.gpu
def test_eight_chains_in_pairs(gpu, ranged):
    """The pair kernel's ranges are cut from the same cost; the chains are the oracle's."""
    probs, mu0, ref = ranged
    assert probs[1].k1_info.lean == 1
    _assert_chain(gpu, probs[1], mu0, ref, n_chains=8)


@pytest.mark.gpu
def test_lean_instantiation_meets_its_resource_targets(gpu):
    import ctypes as C
    lib = gpu._lib.load()
    for fixed in (0, 1):
        v, lds, scr, res = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        gpu.check(lib.mmg_selftest_k1_kernel_info(0, 1, fixed, C.byref(v), C.byref(lds), C.byref(scr), C.byref(res)))
        print("\nlean, fixed walk %d: %d VGPRs, %d bytes LDS, %d bytes scratch, %d workgroups per CU" % (fixed, v.value, lds.value, scr.value, res.value))
        assert scr.value == 0 and v.value <= 72 and lds.value <= 4608
