"""The kernels that read the sliced-ELL stream -- k_sample_sell (fixed and generic walk, far-list and multiplicity instantiations),
k_sample_sell_multi<2> / <4>, the EM stream kernel -- on LONG tile ranges and across a change of the row stream's key.

Every one of them is a persistent single-wave workgroup that owns a contiguous range of tiles and runs a software pipeline over it
(two register buffers refilled one trip ahead, one Philox block per pair of tiles, a window that slides in front of tile A or between
A and B, a last trip without a tile B).  The number of ranges is min(tiles, CUs x waves per CU) and MMG_OPT_SELL_WAVES_PER_CU cannot
go below 1, so on a 256-CU device the other parity tests hand a workgroup 1 ... 4 tiles: the steady state of the pipeline -- a refill
that is followed by a second walk -- only runs in test_gpu_fullsize.py, on generator rows.  Here tests/ladder_problem.py repeats a
period of P (odd) tiles that holds every tile shape the kernels branch on until a range is at least 2 P (and at least 24) tiles long:
each shape is then walked as tile A and as tile B in most ranges, wherever the ranges were cut.  tests/test_ladder_problem.py proves
on the CPU that the periods are what they claim; the sizes are asserted from mmg_problem_info below.

Second hole: the key of a row's Philox block is stream2_key(seed, chain, TAG_ROW, row id >> 33), and no other test puts row id 2^33
inside a problem: the per-lane keys of pair_rng (sell_kernels.h, sell_multi_kernels.h) and the key of bigk_kernels.h only ever saw
one value per wave.  test_row_ids_across_2_to_the_33 puts the change inside a tile, at a tile's first row and behind a slide.

Every comparison is exact equality with the oracle's sequential replay of the stored rows.
P = 13 for the "short" and "k" problems: the factor there is 26 = 2 P instead of 24."""
import numpy as np
import pytest

import ladder_problem as lp

pytestmark = pytest.mark.gpu

SEED = 77
BASE_OPTS = dict(sample_kernel=2, sell_waves_per_cu=1)


@pytest.fixture(scope="module")
def cu_count(gpu):
    p = gpu.Problem.from_csr(np.array([0, 2], np.uint64), np.array([0, 1], np.uint32), np.ones(2))   # a throw-away problem
    n = int(p.info.cu_count)
    p.close()
    assert n >= 1
    return n


class _Built:
    """A ladder problem, its stored order and tile table per row_id_base, and the oracle's replays -- each computed once."""

    def __init__(self, orc, variant, cu):
        self.orc, self.variant = orc, variant
        self.P = lp.period_tiles(variant)
        self.factor = max(24, 2 * self.P)
        self.rp, self.ci, self.l, self.k, self.mu0 = lp.ladder(lp.periods_for(variant, self.factor * cu), variant, seed=11)
        self._tiles, self._refs, self._first = {}, {}, {}

    def stored(self, base=0):
        """(oracle Problem of the stored rows, tile table).  The cut of the tiles depends on the base's parity only."""
        if base & 1 not in self._tiles:
            (rp, ci, k), t = lp.stored_tiles(self.orc, self.rp, self.ci, self.k, base & 1)
            self._tiles[base & 1] = (self.orc.Problem(rp, ci, self.l, k=k), t)
        return self._tiles[base & 1]

    def first_counts(self, chain, base=0):
        key = (chain, base)
        if key not in self._first:
            self._first[key] = self.orc.sample_counts(self.stored(base)[0], self.mu0, SEED, chain, 0, row_id_base=base)
        return self._first[key]

    def ref(self, chain, n_iter, base=0):
        key = (chain, n_iter, base)
        if key not in self._refs:
            self._refs[key] = self.orc.gibbs_keyed(self.stored(base)[0], self.mu0, seed=SEED, chain=chain, n_iter=n_iter, trace_len=n_iter,
                                                   row_id_base=base)
        return self._refs[key]


@pytest.fixture(scope="module")
def built(orc, cu_count):
    cache = {}

    def get(variant):
        if variant not in cache:
            cache[variant] = _Built(orc, variant, cu_count)
        return cache[variant]
    return get


def _upload(gpu, b, base=0):
    """The device problem (created under the options in force), checked: stored order = the oracle's, the sizes that make the ranges
    long, the walk the variant names."""
    ps, t = b.stored(base)
    prob = gpu.Problem.from_csr(b.rp, b.ci, b.l, k=b.k, row_id_base=base)
    rp, ci, k = prob.download(with_k=True)
    assert np.array_equal(rp, ps.row_ptr) and np.array_equal(ci, ps.col_idx) and (ps.k is None or np.array_equal(k, ps.k))
    inf = prob.info
    print("\n%s base %d: n_tiles %d fast_tiles %d far_tiles %d cu_count %d sample_grid %d padded_slots %d rows %d hits %d n %d" % (
        b.variant, base, inf.n_tiles, inf.fast_tiles, inf.far_tiles, inf.cu_count, inf.sample_grid, inf.padded_slots, inf.m, inf.nnz, inf.n))
    assert inf.sample_kernel == 2 and inf.row_id_base == base
    assert inf.n_tiles == t["r0"].size and inf.fast_tiles == int(t["fast"].sum()) and inf.far_tiles == int(t["far"].sum())
    plain = int((t["fast"] & ~t["hask"]).sum())                                # the tile list of the pair kernels
    assert inf.fast_tiles >= 24 * inf.cu_count and plain >= b.factor * inf.cu_count
    if b.variant == "far":
        assert inf.far_tiles >= 4 * inf.cu_count
    if b.variant == "short":
        assert inf.padded_slots < 5 * 256 * inf.fast_tiles                     # k1_fixed_walk
    else:
        assert inf.padded_slots >= 5 * 256 * inf.fast_tiles                    # the generic walk
    return prob, ps, t


def _chains_match(gpu, b, prob, ps, n_chains, chain_base, n_iter, base=0):
    """First sweep = orc.sample_counts; counts and traces after n_iter iterations = orc.gibbs_keyed of every chain, bit for bit."""
    s = gpu.Sampler(prob, b.mu0, seed=SEED, n_chains=n_chains, chain_base=chain_base, gibbs_iter=n_iter, trace_len=n_iter)
    s.sample()
    for c in range(n_chains):
        cnt = s.counts(c)
        assert int(cnt.astype(np.int64).sum()) == ps.total_k(), c
        bad = np.flatnonzero(cnt != b.first_counts(chain_base + c, base))
        assert bad.size == 0, (c, bad[:8], bad.size)
    s.update()
    s.run(n_iter - 1)
    for c in range(n_chains):
        ref = b.ref(chain_base + c, n_iter, base)
        cnt = s.counts(c)
        assert int(cnt.astype(np.int64).sum()) == ps.total_k(), c
        assert np.array_equal(cnt, ref["cnt"]), c
        assert np.array_equal(s.trace(c), ref["trace"]), c
    s.close()


@pytest.mark.parametrize("variant,idx64", [("short", 0), ("short", 1), ("long", 0)])
def test_single_chain_on_long_ranges(gpu, built, variant, idx64):
    """k_sample_sell, fixed walk ("short": also with 64-bit row offsets) and generic walk ("long"), 24 tiles or more per workgroup."""
    b = built(variant)
    opts = dict(BASE_OPTS, force_idx64=1) if idx64 else BASE_OPTS
    with gpu.options(**opts):
        prob, ps, _ = _upload(gpu, b)
        assert prob.info.index_bits == (64 if idx64 else 32)
        _chains_match(gpu, b, prob, ps, 1, 0, 4)
    prob.close()


@pytest.mark.parametrize("replicas", [8, 1])
@pytest.mark.parametrize("fuse,n_chains", [(2, 5), (4, 7)])
@pytest.mark.parametrize("variant", ["short", "long"])
def test_chain_pairs_and_fours_on_long_ranges(gpu, built, variant, fuse, n_chains, replicas):
    """k_sample_sell_multi<2> / <4>: 5 chains in pairs are two pairs and a single chain, 7 chains in fours a four, a pair and a single
    chain; every chain equals the oracle's single-chain replay under its global index, with replicated count vectors and without."""
    b = built(variant)
    with gpu.options(fuse_chains=fuse, cnt_replicas=replicas, **BASE_OPTS):
        prob, ps, _ = _upload(gpu, b)
        _chains_match(gpu, b, prob, ps, n_chains, 3, 4)
    prob.close()


@pytest.mark.parametrize("variant", ["far", "k"])
def test_far_list_and_multiplicity_instantiations_on_long_ranges(gpu, built, variant):
    """Three chains: a pair on the register-path tiles plus a single chain; the pair's far tiles ("far") go through the far-list
    instantiation and every chain's tiles with multiplicities ("k") through the multiplicity instantiation, as grid.y launches; the rows
    on the binomial chain come from their list."""
    b = built(variant)
    with gpu.options(**BASE_OPTS):
        prob, ps, t = _upload(gpu, b)
        if variant == "k":
            L = np.diff(ps.row_ptr.astype(np.int64))
            on_list = (L >= 2) & (ps.k > np.minimum(64, 16 * (L - 1)))
            assert int(on_list.sum()) >= 4 * prob.info.cu_count and int(t["hask"].sum()) >= 2 * prob.info.cu_count
        _chains_match(gpu, b, prob, ps, 3, 0, 3)
    prob.close()


@pytest.mark.parametrize("variant", ["long", "far"])
def test_em_on_the_same_tiles(gpu, orc, built, variant):
    """The EM stream kernel on five ranges of a thousand tiles and more: mu and the log-likelihood after 3 sweeps equal the oracle's."""
    b = built(variant)
    live = lp.mu_live(b.mu0)
    with gpu.options(em_grid=5, **BASE_OPTS):
        prob, ps, _ = _upload(gpu, b)
        g_mu, g_it, g_ll = prob.em(live, max_iter=3, epsilon=-1e308)
    o_mu, o_it, o_ll = orc.em(ps, live, max_iter=3, epsilon=-1e308)
    assert g_it == o_it == 3
    assert np.array_equal(g_mu, o_mu) and g_ll == o_ll
    prob.close()


def test_odd_row_id_base_on_long_ranges(gpu, built):
    """row_id_base = 1: every run starts on the other parity, so the tiles that took the DPP hand-out of the Philox words take
    ds_bpermute and the other way round, and the 63-row tile moves."""
    b = built("short")
    _, t0 = b.stored(0)
    _, t1 = b.stored(1)
    assert t1["odd"].any() and (~t1["odd"]).any()
    same0, same1 = np.isin(t0["r0"], t1["r0"]), np.isin(t1["r0"], t0["r0"])
    assert same1.sum() >= t1["r0"].size // 2 and (t0["odd"][same0] != t1["odd"][same1]).all()
    with gpu.options(**BASE_OPTS):
        prob, ps, _ = _upload(gpu, b, base=1)
        _chains_match(gpu, b, prob, ps, 3, 0, 4, base=1)
    prob.close()


def _key_change_row(t, ps, where):
    """The stored row that gets row id 2^33, from the tile table at an even base (the row is even, so the base's parity is 0):
    even / odd: inside a 64-row tile at an even offset / inside the 63-row tile, which starts on an odd row id, at an odd offset (2^33 is
    even and a 64-row tile starts on an even row id: there it can only sit at an even offset); first: a tile's first row;
    slide: inside the first tile of a band that follows a single-tile band."""
    nt = t["r0"].size
    band = t["call"] // 64
    alone = np.ones(nt, bool)                                                  # the only tile of its band
    alone[1:] &= band[1:] != band[:-1]
    alone[:-1] &= band[:-1] != band[1:]
    lead = np.concatenate([[True], band[1:] != band[:-1]])                     # the first tile of its band
    ok = ~t["far"] & ~t["hask"] & (t["r0"] > ps.m // 2)
    prev_alone = np.concatenate([[False], alone[:-1]])
    if where == "even":
        i = np.flatnonzero(ok & (t["nrows"] == 64) & ~t["odd"])[0]
        return int(t["r0"][i]) + 20, i
    if where == "odd":
        i = np.flatnonzero(ok & (t["nrows"] == 63) & t["odd"])[0]
        return int(t["r0"][i]) + 21, i
    if where == "first":
        i = np.flatnonzero(ok & lead & ~t["odd"] & (t["nrows"] >= 3))[0]
        return int(t["r0"][i]), i
    i = np.flatnonzero(ok & lead & prev_alone & t["slid"] & (t["nrows"] >= 5) & (t["nrows"] < 63))[0]
    return int(t["r0"][i]) + 2 + int(t["r0"][i] & 1), i


@pytest.mark.parametrize("where", ["even", "odd", "first", "slide"])
@pytest.mark.parametrize("variant", ["short", "k"])
def test_row_ids_across_2_to_the_33(gpu, orc, built, variant, where):
    """row_id_base = 2^33 - r: the rows from stored row r on take the key of id >> 33 = 1.  A pair and a single chain, 2 iterations."""
    b = built(variant)
    ps, t = b.stored(0)
    r, i = _key_change_row(t, ps, where)
    base = (1 << 33) - r
    assert base % 2 == 0 and t["r0"][i] <= r < t["r0"][i] + t["nrows"][i] and 0 < r < ps.m
    off = r - int(t["r0"][i])
    assert {"even": off % 2 == 0 and off > 0 and t["nrows"][i] == 64, "odd": off % 2 == 1 and t["odd"][i], "first": off == 0,
            "slide": off > 0 and bool(t["slid"][i])}[where]
    # the oracle itself changes the key there: the rows from r on, replayed as row ids 2^33 ... and as row ids 0 ... (same counters,
    # same words of the block, id >> 33 = 0), must differ; the rows below r, replayed with their ids and 2^33 higher, as well
    hi = orc.Problem(ps.row_ptr[r:] - ps.row_ptr[r], ps.col_idx[int(ps.row_ptr[r]):], ps.l, k=None if ps.k is None else ps.k[r:])
    mu1 = lp.mu_live(b.mu0)
    assert not np.array_equal(orc.sample_counts(hi, mu1, SEED, 0, 0, row_id_base=1 << 33), orc.sample_counts(hi, mu1, SEED, 0, 0, row_id_base=0))
    if variant == "k":                                                          # rows on the binomial chain on both sides of 2^33
        L = np.diff(ps.row_ptr.astype(np.int64))
        on_list = (L >= 2) & (ps.k > np.minimum(64, 16 * (L - 1)))
        assert on_list[:r].sum() >= 100 and on_list[r:].sum() >= 100
    with gpu.options(**BASE_OPTS):
        prob, ps, _ = _upload(gpu, b, base=base)
        _chains_match(gpu, b, prob, ps, 3, 1, 2, base=base)
    prob.close()
