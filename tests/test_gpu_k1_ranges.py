"""The ranges of the single-chain sample launch on every kind of tile list, against tests/k1_range_ref.py: the prices of far tiles
(an entry of the far list 2 v + 11), of CSR-walked tiles (24 v + 130), of multiplicity tiles in the main list (0), the list without
multiplicity tiles and its single empty entry, the cutter's bounds -- all exact -- and the kernel the launch runs.  Then the edges of
the lean choice, MMG_OPT_K1_RANGES above the tile count, and a launch with EMPTY ranges in its middle: one far tile dearer than
total / grid, whose neighbours the cutter leaves without a tile (two `none` descriptors in their headers).

Every problem is built under sample_kernel = 2, derive_order = 0 and MMG_OPT_K1_RANGES; every chain comparison is exact equality with
the oracle's sequential replay of the stored rows, after the count sum."""
import numpy as np
import pytest

import k1_range_ref as ref
import ladder_problem as lp

pytestmark = pytest.mark.gpu

SEED = 53
COSTS = (None, 0, 1, 12)                                               # MMG_OPT_K1_RANGE_COST: unset, the constant model, v = 1, v = 12


def _opts(ranges, cost=None, **kw):
    o = dict(sample_kernel=2, derive_order=0, k1_ranges=ranges, **kw)
    if cost is not None:
        o["k1_range_cost"] = cost
    return o


def _lean_problem(orc):
    q, _ = orc.synth_problem(R=20000, T=1000, avg_hits=8, seed=5, sort=False)
    return q.row_ptr, q.col_idx, q.l


def _all_k_problem(orc):
    """Every row on the conditional-binomial chain (k = 300000 is never stored as k rows): every tile has multiplicities."""
    q, _ = orc.synth_problem(R=3000, T=1000, avg_hits=3, seed=9, sort=False)
    return q.row_ptr, q.col_idx, q.l, np.full(q.m, 300000, np.uint32)


def _dear_problem():
    """23 bands of 40 rows of 2 ... 4 hits -- one register-path tile of one group each, price 6 + 1 -- and three far rows of home band
    10: four hits inside its window (the median hit among them, in band 11), 15 hits below the window and 15 above -- one far tile,
    price 6 + 1 + 23 * 30 = 697 of a total of 858.  16 ranges: floor(858 * 3 / 16) = 160 lies in (154, 161], so bound 3 is tile 23,
    every later bound is the end, the far tile is range 3 by itself and ranges 4 ... 15 are empty."""
    rng = np.random.default_rng(4)
    bands, T = 23, 64 * 26 + 240
    lens, cols = [], []
    for b in range(bands):
        for _ in range(40):
            L = int(rng.integers(2, 5))
            rest = np.sort(rng.choice(np.arange(64 * b + 20, 64 * b + 200), size=L - 1, replace=False))
            cols.append(np.concatenate([[64 * b + int(rng.integers(0, 20))], rest]))
            lens.append(L)
    for j in range(3):
        low = np.sort(rng.choice(np.arange(0, 576), size=15, replace=False))
        high = np.sort(rng.choice(np.arange(900, T), size=15, replace=False))
        cols.append(np.concatenate([low, [650 + j, 710 + j, 720 + j, 730 + j], high]))
        lens.append(34)
    rp = np.zeros(len(lens) + 1, np.uint64)
    rp[1:] = np.cumsum(lens)
    return rp, np.concatenate(cols).astype(np.uint32), np.linspace(0.5, 2.0, T)


def _case(orc, kind):
    """(row_ptr, col_idx, l, k, keep_rows, MMG_OPT_K1_RANGES)"""
    if kind == "lean":
        return _lean_problem(orc) + (None, False, 9)
    if kind in ("far_0.03", "far_0.5"):
        q, _ = orc.synth_problem(R=8000, T=3000, avg_hits=8, seed=7, sort=False, far_fraction=float(kind[4:]))
        return q.row_ptr, q.col_idx, q.l, None, False, 7
    if kind == "uniform":
        q, _ = orc.synth_problem(R=4000, T=2000, avg_hits=8, seed=3, sort=False, uniform=True)
        return q.row_ptr, q.col_idx, q.l, None, False, 5
    if kind == "ladder_k":
        rp, ci, l, k, _ = lp.ladder(6, "k", seed=11)
        return rp, ci, l, k, False, 4
    if kind == "keep_rows":                                            # generator order kept: most tiles span the transcriptome
        q, _ = orc.synth_problem(R=5000, T=2000, avg_hits=8, seed=13, sort=False, far_fraction=0.03)
        return q.row_ptr, q.col_idx, q.l, None, True, 6
    if kind == "all_k":
        return _all_k_problem(orc) + (False, 1)
    if kind == "dear":
        return _dear_problem() + (None, False, 16)
    raise ValueError(kind)


@pytest.fixture(scope="module")
def cases(orc):
    """kind -> (arguments, MMG_OPT_K1_RANGES, stored rows, tile table): each computed once."""
    cache = {}

    def get(kind):
        if kind not in cache:
            rp, ci, l, k, keep, ranges = _case(orc, kind)
            stored, t = ref.stored_table(orc, rp, ci, k, l.size, 0, keep)
            cache[kind] = ((rp, ci, l, k, keep), ranges, stored, t)
        return cache[kind]
    return get


def _build(gpu, args, stored):
    rp, ci, l, k, keep = args
    prob = gpu.Problem.from_csr(rp, ci, l, k=k, keep_rows=keep)
    d_rp, d_ci, d_k = prob.download(with_k=True)
    assert np.array_equal(d_rp, stored[0]) and np.array_equal(d_ci, stored[1])
    assert np.array_equal(d_k, np.ones(d_k.size, np.uint32) if stored[2] is None else stored[2])
    return prob


def _assert_ranges(prob, t, ranges, cost, want_lean=None):
    """Everything mmg_problem_info, mmg_k1_info and mmg_problem_k1_ranges say about the main list equals the restatement."""
    want = ref.main_ranges(t, ranges, cost, want_lean)
    inf, k1 = prob.info, prob.k1_info
    bound, cum, grp = (a.astype(np.int64) for a in prob.k1_ranges())
    n = bound.size - 1
    print("\ncost %r: list of %d, %d ranges, bound %s, cost per range %s" % (cost, k1.n_list, n, bound.tolist()[:41], np.diff(cum).tolist()[:40]))
    assert inf.sample_kernel == 2
    assert (inf.n_tiles, inf.fast_tiles, inf.far_tiles) == (t["r0"].size, int(t["qual"].sum()), int(t["far_tile"].sum()))
    assert bound[0] == 0 and bound[n] == k1.n_list == want["n_list"] and n == inf.sample_grid
    assert bound.tolist() == want["bound"]
    assert np.diff(cum).tolist() == np.diff(want["cum_cost"]).tolist() and k1.list_cost == want["list_cost"]
    assert np.diff(grp).tolist() == np.diff(want["cum_groups"]).tolist()
    assert (k1.n_ranges, k1.range_cost_max, k1.range_tiles_max) == (want["n_ranges"], want["range_cost_max"], want["range_tiles_max"])
    assert k1.range_cost_mean == want["range_cost_mean"]              # (one division of the same two integers)
    assert (k1.lean, k1.fixed_walk, k1.range_tile_cost) == (int(want["lean"]), int(want["fixed_walk"]), want["range_tile_cost"])
    return want


def _assert_chains(gpu, orc, prob, stored, l, n_chains, n_iter=4):
    """Count sums, then counts, trace, mu and moments of every chain = orc.gibbs_keyed of the stored rows."""
    ps = orc.Problem(stored[0], stored[1], l, k=stored[2])
    total_k = ref.total_k_hit(stored[0], stored[2])                     # (of the rows with a hit: an empty row draws nothing)
    mu0, _ = prob.start_values()
    s = gpu.Sampler(prob, mu0, seed=SEED, n_chains=n_chains, gibbs_iter=n_iter, trace_len=n_iter)
    s.sample()
    for c in range(n_chains):
        assert int(s.counts(c).astype(np.int64).sum()) == total_k, c
    s.update()
    s.run(n_iter - 1)
    for c in range(n_chains):
        r = orc.gibbs_keyed(ps, mu0, seed=SEED, chain=c, n_iter=n_iter, trace_len=n_iter)
        cnt = s.counts(c)
        assert int(cnt.astype(np.int64).sum()) == total_k, c
        assert np.array_equal(cnt, r["cnt"]), c
        assert np.array_equal(s.trace(c), r["trace"]), c
        assert np.array_equal(s.mu(c), r["mu"]), c
        sl, sl2 = s.moments(c)[:2]
        assert np.array_equal(sl, r["sum_log"]) and np.array_equal(sl2, r["sum_log2"]), c
    s.close()


@pytest.mark.parametrize("kind", ["lean", "far_0.03", "far_0.5", "uniform", "ladder_k", "keep_rows", "all_k"])
def test_prices_and_cuts(gpu, cases, kind):
    args, ranges, stored, t = cases(kind)
    # the problem is of its kind: the price under test is in the list
    nf = int(t["far_nf"].max())                                         # (-1: no far tile)
    mixed = t["far_tile"].sum() >= 8 and t["qual"].sum() >= 8 and nf >= 2
    has = {"lean": t["qual"].all(), "far_0.03": mixed, "far_0.5": mixed, "uniform": t["far_tile"].sum() > 0.8 * t["r0"].size and nf >= 5,
           "ladder_k": t["hask"].sum() >= 6 and (~t["hask"]).sum() >= 6, "keep_rows": t["slow"].sum() >= 8 and not t["hask"].any(),
           "all_k": t["hask"].all()}
    assert has[kind], kind
    for cost in COSTS:
        with gpu.options(**_opts(ranges, cost)):
            prob = _build(gpu, args, stored)
        want = _assert_ranges(prob, t, ranges, cost)
        assert want["lean"] == (kind == "lean")
        if kind == "all_k":                                            # the list without multiplicity tiles: its single empty entry
            assert want["bound"] == [0, 1] and want["list_cost"] == 0 and want["n_ranges"] == 0
        elif kind == "ladder_k":                                       # bounds are entries of that list, not tiles
            assert want["n_list"] == int((~t["hask"]).sum()) < t["r0"].size
        got = prob.k1_lists()
        lists = ref.lists(t, ranges, cost)
        for name in ref.LISTS:
            assert got[name] == ref.list_shape(lists[name]), name
        prob.close()


def test_lean_survives_a_k_array_of_ones_and_tiles_of_empty_rows(gpu, orc):
    rp, ci, l = _lean_problem(orc)
    rp = np.concatenate([np.zeros(200, np.uint64), rp])                # 200 empty rows: stored first, three tiles without a hit
    k = np.ones(rp.size - 1, np.uint32)
    for kk in (None, k):
        stored, t = ref.stored_table(orc, rp, ci, kk, l.size)
        assert int((t["nnz"] == 0).sum()) >= 3 and t["qual"][t["nnz"] > 0].all()
        with gpu.options(**_opts(5)):
            prob = _build(gpu, (rp, ci, l, kk, False), stored)
        want = _assert_ranges(prob, t, 5, None)
        assert want["lean"] and prob.k1_info.lean == 1
        if kk is not None:
            _assert_chains(gpu, orc, prob, stored, l, 1, n_iter=2)
        prob.close()


def test_one_far_row_among_twenty_thousand_turns_lean_off(gpu, orc):
    from mmseq_amd._lib import MMGError
    rp, ci, l = _lean_problem(orc)
    rp = np.concatenate([rp, [rp[-1] + 2]]).astype(np.uint64)
    ci = np.concatenate([ci, [3, 900]]).astype(np.uint32)               # 900 - 0 >= 240: a far row
    stored, t = ref.stored_table(orc, rp, ci, None, l.size)
    assert rp.size - 1 == 20001 and int(t["far_tile"].sum()) == 1 and int(t["qual"].sum()) == t["r0"].size - 1
    with gpu.options(**_opts(5)):
        prob = _build(gpu, (rp, ci, l, None, False), stored)
    want = _assert_ranges(prob, t, 5, None)
    assert not want["lean"] and prob.k1_info.lean == 0 and prob.info.far_tiles == 1

    def held():
        c = np.zeros(3, np.int64)
        gpu.check(gpu._lib.load().mmg_selftest_live(c.ctypes.data))
        return c.tolist()
    live = held()
    with gpu.options(**_opts(5, k1_lean=1)):
        with pytest.raises(MMGError) as e:
            gpu.Problem.from_csr(rp, ci, l)
    assert e.value.code == 1 and "MMG_OPT_K1_LEAN" in str(e.value)
    assert held() == live                                               # the refused build gave back what it held
    prob.close()


def test_more_ranges_than_entries(gpu, orc, cases):
    """MMG_OPT_K1_RANGES above the entries of a list clamps its ranges to the entries.  Where the entries cost the same (a lean
    problem under the constant model: 2 each) that is one entry per range; where they do not, the cutter still cuts by cost -- a dear
    tile's neighbour shares a range, another range stays empty -- as the restatement says.  Either way the chains are the oracle's."""
    for kind, cost in (("lean", 0), ("far_0.03", None)):
        args, _, stored, t = cases(kind)
        nt = t["r0"].size
        with gpu.options(**_opts(1 << 20, cost)):
            prob = _build(gpu, args, stored)
        want = _assert_ranges(prob, t, 1 << 20, cost)
        assert prob.info.sample_grid == nt
        for name, (entries, ranges, longest) in prob.k1_lists().items():
            assert ranges == entries and (longest >= 1) == (entries > 0), name
        if kind == "lean":
            assert want["bound"] == list(range(nt + 1))
            assert {v[2] for v in prob.k1_lists().values()} == {0, 1}
        else:
            assert max(np.diff(want["bound"])) <= 2 and 0 in np.diff(want["bound"])
        _assert_chains(gpu, orc, prob, stored, args[2], 3, n_iter=3)   # a pair (register-path list, far list) and a single chain
        prob.close()


def test_default_ranges_cover_the_list(gpu, cases):
    """Without MMG_OPT_K1_RANGES the number of ranges follows the occupancy the runtime reports and the end may be tapered: only that
    the bounds cover the list, ascend, and that no range exceeds a full share by a whole entry (a tapered launch of n ranges has at
    least 2 n / 3 full shares)."""
    args, _, stored, t = cases("lean")
    with gpu.options(sample_kernel=2, derive_order=0):
        prob = _build(gpu, args, stored)
    k1 = prob.k1_info
    bound, cum, _ = (a.astype(np.int64) for a in prob.k1_ranges())
    n = bound.size - 1
    assert n == prob.info.sample_grid and bound[0] == 0 and bound[n] == k1.n_list == t["r0"].size and (np.diff(bound) >= 0).all()
    dearest = int(ref.tile_prices(t).max())
    assert k1.list_cost == int(ref.tile_prices(t).sum()) and (np.diff(cum) * 2 * n < 3 * k1.list_cost + 2 * n * dearest).all()
    prob.close()


@pytest.mark.parametrize("n_chains", [1, 3])
@pytest.mark.parametrize("kind", ["dear", "all_k"])
def test_empty_ranges_inside_a_launch(gpu, orc, cases, kind, n_chains):
    """dear: a far tile of 30 list entries against neighbours of one group -- interior ranges without a tile, the far tile a range of
    its own.  all_k: the main list is the single empty entry, one range at cost 0.  One chain, and a pair plus a single chain."""
    args, ranges, stored, t = cases(kind)
    with gpu.options(**_opts(ranges)):
        prob = _build(gpu, args, stored)
    _assert_ranges(prob, t, ranges, None)
    bound, cum, _ = (a.astype(np.int64) for a in prob.k1_ranges())
    if kind == "dear":
        nt = t["r0"].size
        assert nt == 24 and t["far_tile"].tolist() == [False] * 23 + [True] and int(t["far_nf"][-1]) == 30 and bound.size == 17
        tiles = np.diff(bound)
        assert (tiles[1:-1] == 0).any()                                 # an interior range is empty
        alone = np.flatnonzero((bound[:-1] == nt - 1) & (bound[1:] == nt))
        assert alone.size == 1 and 0 < alone[0] < 15                    # the far tile alone fills a range, and not the last one
        assert np.diff(cum)[alone[0]] == 6 + 1 + (2 * 6 + 11) * 30
    else:
        assert bound.tolist() == [0, 1] and cum.tolist() == [0, 0]
    _assert_chains(gpu, orc, prob, stored, args[2], n_chains, n_iter=4)
    prob.close()
