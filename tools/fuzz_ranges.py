"""Differential fuzz of the stream kernels on LONG tile ranges (GPU box): the random problems of fuzz_parity.py under
MMG_OPT_K1_RANGES, so that a workgroup walks eight to several thousand tiles of every list a sample call launches over -- the main
list under the lean and the general instantiation, the list of tiles with multiplicities, the pair and four lists, the far / CSR
list of paired chains -- and every chain is compared with the oracle bit for bit.  tests/k1_range_ref.py predicts on the CPU which
kernel runs and how every list is cut; a case asserts that the device built exactly that before it looks at a chain.
usage: fuzz_ranges.py [n_cases] [first_seed] [--census]      (--census: no device, only what the cases would cover)"""
import functools
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import fuzz_parity
import k1_range_ref as ref

MAX_ROWS = 60000                       # the generator's row bound: fuzz_parity's own
FIRST_SEED, N_SEEDS = 3064, 48         # the cases of tests/test_gpu_fuzz_ranges.py; their census meets CENSUS_FLOORS (test_census_of_the_fixed_seeds)
RANGE_CHOICES = (1, 2, 3, 5, 8, 13, 40)
LONG = 8                               # entries per range, on average, from which a list counts as walked on long ranges
KINDS = ("main_lean", "main_general", "pairs", "far_csr", "multiplicity", "main_with_csr_tiles")
CENSUS_FLOORS = dict(main_lean=6, main_general=6, pairs=6, far_csr=6, multiplicity=6, main_with_csr_tiles=3)


@functools.lru_cache(maxsize=None)
def _plan(seed, orc):
    return _make_plan(seed, orc)


def plan(seed, orc):
    """A case without the device: the generator's problem, this tool's own draws, the stored rows and what the restatement predicts."""
    return _plan(int(seed), orc)


def _make_plan(seed, orc):
    _, g = fuzz_parity.generate(seed, orc, max_rows=MAX_ROWS)
    pk = g["pk"]
    stored, t = ref.stored_table(orc, pk.row_ptr, pk.col_idx, pk.k, g["T"], g["row_id_base"], g["keep_rows"], g["tx_order"])
    rng = np.random.default_rng([seed, 0x6b315f72])                       # this tool's own stream
    ranges = int(rng.choice(RANGE_CHOICES))
    cost = int(rng.choice([-1, 0, 1, 12]))
    can_lean = ref.kernel_choice(t)[0]
    lean = int(rng.choice([-1, 0, 1] if can_lean else [-1, 0]))
    # derive_order = 0: the library keeps the transcript order it was given, which is what the restatement can predict
    opts = dict(sample_kernel=2, derive_order=0, k1_ranges=ranges, fuse_chains=int(rng.choice([1, 2, 4])), cnt_replicas=int(rng.choice([1, 8])),
                em_grid=int(rng.choice([1, 2, 5])))
    if cost >= 0: opts["k1_range_cost"] = cost
    if lean >= 0: opts["k1_lean"] = lean
    chains = int(rng.choice([1, 2, 3, 5]))
    if rng.integers(0, 3) == 0: opts["force_idx64"] = 1
    if rng.integers(0, 3) == 0: opts["bigk_per_wave"] = int(rng.choice([1, 5, 64, 300]))
    if rng.integers(0, 3) == 0: opts["bigk_side_stream"] = 0
    n_it = int(rng.integers(2, 5))
    alpha, beta = float(rng.choice([0.1, 1.0])), float(rng.choice([0.1, 2.0]))
    lists = ref.lists(t, ranges, cost)
    want = ref.main_ranges(t, ranges, cost, lean)
    # which lists the sample calls walk: chains in groups of fuse_chains (fours leave a pair where two are left) over the register-path
    # tiles without multiplicities and, in one launch for all of them, over the far / CSR list; a chain left over walks the main list
    fuse = opts["fuse_chains"] if lists["pairs"] is not None else 1
    fused = (chains // fuse) * fuse if fuse > 1 else 0
    paired = fused + ((chains - fused) // 2) * 2 if fuse == 4 else fused
    shape = {name: ref.list_shape(lists[name]) for name in ref.LISTS}
    long_ = {name: shape[name][1] > 0 and shape[name][0] >= LONG * shape[name][1] for name in ref.LISTS}
    single = chains > paired
    kinds = dict(main_lean=single and long_["main"] and want["lean"], main_general=single and long_["main"] and not want["lean"],
                 pairs=paired > 0 and long_["pairs"], far_csr=paired > 0 and long_["far_csr"], multiplicity=long_["multiplicity"],
                 main_with_csr_tiles=single and long_["main"] and bool(t["slow"][lists["main"]["tiles"][lists["main"]["tiles"] >= 0]].any()))
    return dict(seed=seed, g=g, stored=stored, table=t, opts=opts, chains=chains, n_it=n_it, alpha=alpha, beta=beta, lists=lists, shape=shape,
                want=want, kinds=kinds)


def census(seeds, orc):
    """{kind: the cases among `seeds` that walk a list of that kind at LONG entries per range or more} -- from the restatement alone."""
    count = dict.fromkeys(KINDS, 0)
    for seed in seeds:
        for kind, hit in plan(seed, orc)["kinds"].items():
            count[kind] += bool(hit)
    return count


def _equal(a, b):
    return np.array_equal(a, b, equal_nan=True)                            # (a NaN is equal to the same NaN)


def one_case(seed, gpu, orc, verbose=True):
    pl = plan(seed, orc)
    g, t, want, opts = pl["g"], pl["table"], pl["want"], pl["opts"]
    pk0, mu0, rid0, chains, n_it = g["pk"], g["mu0"], g["row_id_base"], pl["chains"], pl["n_it"]
    with gpu.options(**opts):
        prob = gpu.Problem.from_csr(pk0.row_ptr, pk0.col_idx, pk0.l, k=pk0.k, row_id_base=rid0, keep_rows=g["keep_rows"], tx_order=g["tx_order"])
        d_rp, d_ci, d_k = prob.download(with_k=True)
        s_rp, s_ci, s_k = pl["stored"]
        assert np.array_equal(d_rp, s_rp) and np.array_equal(d_ci, s_ci), "stored rows"
        assert np.array_equal(d_k, np.ones(d_k.size, np.uint32) if s_k is None else s_k), "stored k"
        pk = orc.Problem(d_rp, d_ci, pk0.l, k=(d_k if g["k"] is not None else None))
        inf, k1, got_lists = prob.info, prob.k1_info, prob.k1_lists()
        assert inf.sample_kernel == 2 and inf.tx_renumbered in (0, 1), (inf.sample_kernel, inf.tx_renumbered)
        assert (inf.n_tiles, inf.fast_tiles, inf.far_tiles) == (t["r0"].size, int(t["qual"].sum()), int(t["far_tile"].sum())), "tile counts"
        assert (k1.lean, k1.fixed_walk) == (int(want["lean"]), int(want["fixed_walk"])), "kernel: lean %d fixed walk %d" % (k1.lean, k1.fixed_walk)
        for name in ref.LISTS:
            assert got_lists[name][1] <= opts["k1_ranges"], "%s list: %d ranges" % (name, got_lists[name][1])
            assert got_lists[name] == pl["shape"][name], "%s list: %r, restated %r" % (name, got_lists[name], pl["shape"][name])
        bound = prob.k1_ranges()[0]
        assert inf.sample_grid == len(want["bound"]) - 1 and bound.tolist() == want["bound"], "ranges of the main list"
        g_mu0, g_uh = prob.start_values()
        assert np.array_equal(g_uh, g["uh"]), "unique hits"
        assert np.array_equal(g_mu0, orc.start_values_exact(pk)), "start values"
        kw = dict(alpha=pl["alpha"], beta=pl["beta"], seed=seed)
        total_k = ref.total_k_hit(pk.row_ptr, pk.k)                          # (total_k of the rows with a hit: the fuzz has empty rows)
        s = gpu.Sampler(prob, mu0, n_chains=chains, chain_base=2, gibbs_iter=n_it, trace_len=n_it, **kw)
        s.sample()
        for c in range(chains):
            cnt = s.counts(c)
            assert int(cnt.astype(np.int64).sum()) == total_k, "count sum after the first sweep, chain %d" % c
            assert np.array_equal(cnt, orc.sample_counts(pk, mu0, seed, 2 + c, 0, row_id_base=rid0)), "counts after the first sweep, chain %d" % c
        s.update()
        s.run(n_it - 1)
        for c in range(chains):
            r = orc.gibbs_keyed(pk, mu0, n_iter=n_it, trace_len=n_it, chain=2 + c, row_id_base=rid0, **kw)
            cnt = s.counts(c)
            assert int(cnt.astype(np.int64).sum()) == total_k, "count sum, chain %d" % c
            assert np.array_equal(cnt, r["cnt"]), "counts chain %d" % c
            assert np.array_equal(s.trace(c), r["trace"]), "trace chain %d" % c
            assert _equal(s.mu(c), r["mu"]), "mu chain %d" % c
            sl, sl2 = s.moments(c)[:2]
            assert _equal(sl, r["sum_log"]) and _equal(sl2, r["sum_log2"]), "moments chain %d" % c
        s.close()
        live = np.isfinite(mu0) & (mu0 > 0)
        if live.any():
            mu_g, it_g, ll_g = prob.em(mu0, max_iter=2, epsilon=-1e308)
            mu_o, it_o, ll_o = orc.em(pk, mu0, max_iter=2, epsilon=-1e308)
            assert np.array_equal(mu_g, mu_o, equal_nan=True), "EM mu"
            assert ll_g == ll_o or (np.isnan(ll_g) and np.isnan(ll_o)), "EM loglik %r %r" % (ll_g, ll_o)
        prob.close()
    if verbose:
        print("seed %d ok: rows %d T %d keep=%s tx=%s chains %d x %d it, lists %s, kinds %s, opts %s" % (
            seed, pk.m, g["T"], g["keep_rows"], g["tx_order"] is not None, chains, n_it, pl["shape"],
            [k for k, v in pl["kinds"].items() if v], opts), flush=True)


if __name__ == "__main__":
    from oracle import binding as orc
    argv = [a for a in sys.argv[1:] if a != "--census"]
    n = int(argv[0]) if len(argv) > 0 else N_SEEDS
    s0 = int(argv[1]) if len(argv) > 1 else FIRST_SEED
    if "--census" in sys.argv:
        print(census(range(s0, s0 + n), orc))
        sys.exit(0)
    from mmseq_amd import gibbs as gpu
    for seed in range(s0, s0 + n):
        one_case(seed, gpu, orc)
    print("all %d cases bit-identical" % n)
