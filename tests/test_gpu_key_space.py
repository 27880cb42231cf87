"""The keyed streams over their whole key space, on the device.  First the checks of tests/test_key_space.py again, in kernels
(mmg_selftest_keyed and the older self tests with device = 0); then the sample and update kernels, the simulated isoforms of the
summaries, the generator, mmdiff and the CLI with the keys the rest of the suite never uses: seeds with a high word, chains up to the
Gamma stream's 24 bits, stream ids with a high word (the key space).  Everything is compared with the CPU oracle
bit for bit."""
import functools
import gzip

import numpy as np
import pytest

import key_space_checks as K

pytestmark = pytest.mark.gpu

SEEDS = [2 ** 32, 2 ** 32 + 1234, 2 ** 63, 2 ** 64 - 7, 0x9E3779B97F4A7C15]
TOP = 2 ** 24 - 3                       # three chains from here are the last three the Gamma stream can tell apart


# ------------------------------------------------------------------------------------------ streams and math, pointwise
def test_streams_over_the_key_space_equal_the_spec(gpu, orc):
    K.check_streams(gpu, orc, 0)


def test_stream_identities_of_the_key_derivation(gpu):
    K.check_stream_identities(gpu, 0)


@pytest.mark.parametrize("shape", K.GAMMA_SHAPES)
def test_gamma_shapes_equal_oracle(gpu, orc, shape):
    K.check_gamma_shape(gpu, orc, 0, shape)


@pytest.mark.parametrize("nn,p", K.BINOMIALS)
def test_binomial_edges_equal_oracle(gpu, orc, nn, p):
    K.check_binomial(gpu, orc, 0, nn, p)


def test_normal_equals_oracle(gpu, orc):
    K.check_normal(gpu, orc, 0)


def test_probit_equals_as241_transcription(gpu, orc):
    K.check_probit(gpu, orc, 0)


def test_lgamma_equals_numpy_restatement(gpu):
    K.check_lgamma(gpu, 0)


def test_stirling_tail_and_ilogb(gpu):
    host = K.check_stirling(gpu, -1)
    assert K.same(K.check_stirling(gpu, 0), host)       # (the accuracy of these bits: tests/test_key_space.py)
    K.check_ilogb(gpu, 0)


def test_word_maps_at_the_extreme_words_are_exact(gpu):
    K.check_word_maps(gpu, 0)


# ------------------------------------------------------------------------------------------ the chains
class Case:
    pass


@pytest.fixture(scope="module")
def case(gpu, orc):
    """One small problem for every chain test: rows in generator order, a fifth of them with a hit far from their window, multiplicities
    from single reads to the conditional-binomial chain; stored once per sample kernel, replayed by the oracle in the stored order."""
    p, _ = orc.synth_problem(R=8000, T=2000, avg_hits=6, seed=17, sort=False, far_fraction=0.2)
    rng = np.random.default_rng(4)
    k = rng.choice([1, 1, 1, 2, 9, 40, 700, 300000], size=p.m).astype(np.uint32)
    pk = orc.Problem(p.row_ptr, p.col_idx, p.l * 50, k=k)
    c = Case()
    c.mu0, _ = orc.start_values(pk)
    c.prob = {}
    for kern in (2, 0):
        with gpu.options(sample_kernel=kern):
            c.prob[kern] = gpu.Problem.from_csr(pk.row_ptr, pk.col_idx, pk.l, k=pk.k)
        assert c.prob[kern].info.sample_kernel == kern
    rp, ci, kk = c.prob[2].download(with_k=True)
    rp0, ci0, kk0 = c.prob[0].download(with_k=True)
    assert np.array_equal(rp, rp0) and np.array_equal(ci, ci0) and np.array_equal(kk, kk0)     # one stored order: one reference
    c.stored = orc.Problem(rp, ci, pk.l, k=kk)
    inf = c.prob[2].info
    L = np.diff(rp.astype(np.int64))
    on_chain = (L >= 2) & (kk > np.minimum(64, 16 * (L - 1)))
    tile_has_k = np.add.reduceat((kk > 1).astype(np.int64), np.arange(0, kk.size, 64)) > 0
    assert inf.fast_tiles > 0 and inf.far_tiles > 0 and inf.n_tiles > 500                         # register-path tiles, far tiles
    assert 0 < tile_has_k.sum() < tile_has_k.size                                                 # 64-row stretches with and without multiplicities
    assert on_chain.sum() >= 100 and ((kk > 1) & ~on_chain).any()                                 # the binomial chain; k kept on rows of one hit
    assert int(kk.astype(np.int64).sum()) == int(k.astype(np.int64).sum())

    @functools.lru_cache(maxsize=None)
    def first_sweep(seed, chain):
        r = orc.sample_counts(c.stored, c.mu0, seed, chain, 0)
        r.setflags(write=False)
        return r

    @functools.lru_cache(maxsize=None)
    def chain4(seed, chain):
        r = orc.gibbs_keyed(c.stored, c.mu0, seed=seed, chain=chain, n_iter=4, trace_len=4)
        for v in r.values():
            v.setflags(write=False)
        return r

    c.first_sweep, c.chain4 = first_sweep, chain4
    yield c
    for prob in c.prob.values():
        prob.close()


def _run_chains(gpu, case, kern, seed, base, n_chains, **opts):
    """n_chains chains from chain index `base` for 4 iterations: the first sweep's counts, then counts, trace, mu and moments after the
    fourth, each against the oracle's chain of the same (seed, chain)."""
    with gpu.options(**opts):
        s = gpu.Sampler(case.prob[kern], case.mu0, seed=seed, n_chains=n_chains, chain_base=base, gibbs_iter=4, trace_len=4)
        s.sample()
        first = [s.counts(c) for c in range(n_chains)]
        s.update()
        s.run(3)
        for c in range(n_chains):
            assert np.array_equal(first[c], case.first_sweep(seed, base + c)), ("first sweep", c)
            ref = case.chain4(seed, base + c)
            assert np.array_equal(s.counts(c), ref["cnt"]), ("counts", c)
            assert np.array_equal(s.trace(c), ref["trace"]), ("trace", c)
            assert np.array_equal(s.mu(c), ref["mu"]), ("mu", c)
            sl, sl2, ns = s.moments(c)
            assert ns == 4 and np.array_equal(sl, ref["sum_log"]) and np.array_equal(sl2, ref["sum_log2"]), ("moments", c)
        s.close()
    return first


@pytest.mark.parametrize("kern", [2, 0])
@pytest.mark.parametrize("base", [0, TOP])
@pytest.mark.parametrize("seed", SEEDS)
def test_chains_with_high_seed_words_and_the_last_chain_indices(gpu, case, seed, base, kern):
    """Three chains of one sampler, a fused pair and a single chain: every site that builds a row key (the sliced-ELL kernel, its pair
    and far-list instantiations, the multiplicity and binomial-chain kernels, the CSR kernel) and K2's Gamma key, with a seed whose high
    word is set and with chain indices up to 2^24 - 1."""
    _run_chains(gpu, case, kern, seed, base, 3, fuse_chains=2)


def test_five_chains_fused_in_fours(gpu, case):
    _run_chains(gpu, case, 2, SEEDS[2], 2 ** 24 - 5, 5, fuse_chains=4)


def test_one_count_replica(gpu, case):
    _run_chains(gpu, case, 2, SEEDS[3], TOP, 3, fuse_chains=2, cnt_replicas=1)


def test_the_high_seed_word_changes_the_first_sweep(gpu, case):
    lo = _run_chains(gpu, case, 2, 1234, 0, 1)
    hi = _run_chains(gpu, case, 2, 2 ** 32 + 1234, 0, 1)
    assert not np.array_equal(lo[0], hi[0])


# ------------------------------------------------------------------------------------------ 64-bit stream ids
VID = np.array([2 ** 32, 2 ** 32 + 7, 2 ** 63 + 1, 2 ** 64 - 1, 7], np.uint64)
VSCALE = np.array([0.5, 1.0, 0.01, 2.0, 1.0])


@pytest.fixture(scope="module")
def small(gpu, orc):
    """70 transcripts, two chains, 64 kept samples, seed with a high word; V[c]: the oracle's simulated isoforms keyed by chain c.
    (The high word is not 1: XORed with the chains 0 and 1 that would only swap them, which the pooled and rank-based checks cannot see.)"""
    S, seed = 64, (0xABCD << 32) + 31
    p, _ = orc.synth_problem(R=3000, T=70, avg_hits=4, seed=12, sort=False)
    prob = gpu.Problem.from_csr(p.row_ptr, p.col_idx, p.l)
    mu0, _ = prob.start_values()
    s = gpu.Sampler(prob, mu0, seed=seed, n_chains=2, gibbs_iter=S, trace_len=S)
    s.run(S)
    V = np.stack([np.stack([orc.simu_gamma_trace_keyed(seed, c, orc.TAG_SIMU, int(VID[v]), 0.1, VSCALE[v], S) for v in range(VID.size)])
                  for c in range(2)])
    assert np.array_equal(V[0], np.stack([orc.simu_gamma_trace(seed, int(VID[v]), 0.1, VSCALE[v], S) for v in range(VID.size)]))
    assert not np.array_equal(V[0][1], V[0][4] * VSCALE[1] / VSCALE[4]) and not np.array_equal(V[0], V[1])     # ids 2^32 + 7 and 7; the chains
    yield dict(prob=prob, s=s, n=p.n, S=S, seed=seed, V=V)
    s.close(); prob.close()


def test_summary_simulates_isoforms_with_64_bit_ids(gpu, small):
    s, n, S, V = small["s"], small["n"], small["S"], small["V"]
    own = [[n + v] for v in range(VID.size)]                        # a set of one member: its trace is the member's
    for chain in (0, 1):                                            # (the summary keys its isoforms by chain 0 whichever chain it reads)
        q = gpu.Summary(s, chain=chain, virtual_id=VID, virtual_scale=VSCALE, identical=own, genes=own, percentile_index=list(range(S)))
        assert np.array_equal(q.rows(gpu.SERIES_IDENTICAL).T, V[0]) and np.array_equal(q.rows(gpu.SERIES_GENE).T, V[0])
        assert np.array_equal(q.series(gpu.SERIES_VIRTUAL)["percentiles"], np.sort(V[0], axis=1))
        q.close()
    assert not np.array_equal(V[0][1], V[0][4])


def test_convergence_and_pooled_simulate_isoforms_with_64_bit_ids(gpu, small):
    s, S, V = small["s"], small["S"], small["V"]
    cv = gpu.Convergence(s, virtual_id=VID, virtual_scale=VSCALE)
    want = gpu.convergence_of_traces(np.ascontiguousarray(V.transpose(0, 2, 1)))         # the same kernel on the oracle's draws
    got = cv.series(gpu.SERIES_VIRTUAL)
    for k in ("rhat", "ess_bulk", "ess_tail"):
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert len({float(v) for v in got["rhat"]}) == VID.size
    cv.close()
    ps = gpu.PooledSummary(s, virtual_id=VID, virtual_scale=VSCALE, percentile_index=list(range(2 * S)))
    pooled = np.concatenate([V[0], V[1]], axis=1)                    # per-chain keys: the draws of both chains, sorted
    assert np.array_equal(ps.series(gpu.SERIES_VIRTUAL)["percentiles"], np.sort(pooled, axis=1))
    ps.close()


def test_contrasts_simulate_isoforms_with_64_bit_ids(gpu, orc, small):
    from mmseq_amd import Contrast
    from test_gpu_contrast import _host_gamma_trace
    s, n, S, seed, V = small["s"], small["n"], small["S"], small["seed"], small["V"]
    host = np.stack([_host_gamma_trace(seed, int(VID[v]), 0.1, VSCALE[v], S) for v in range(VID.size)])
    assert np.array_equal(host, V[0])                               # mmg_host_gamma_trace is the oracle's
    q = gpu.Summary(s, chain=0, virtual_id=VID, virtual_scale=VSCALE, percentile_index=[0])
    full = np.concatenate([s.trace(0), host])
    cs = [([n + v], [n + (v + 1) % VID.size]) for v in range(VID.size)] + [([n + v], [v]) for v in range(VID.size)]
    log = gpu.selftest_math(V[0].ravel(), 0)["log"].reshape(V[0].shape)
    with Contrast.from_sampler(s, q, cs) as a, Contrast.from_traces(full, cs) as b:
        rows = a.rows()
        assert np.array_equal(rows, b.rows())
        assert np.array_equal(rows[:VID.size], log - np.roll(log, -1, axis=0))         # log N - log D of two simulated isoforms
    q.close()


# ------------------------------------------------------------------------------------------ generator, mmdiff, CLI
def test_generator_with_a_64_bit_seed_and_row_ids_across_2_32(gpu, orc):
    """tests/test_gpu_parity.py::test_device_generator_matches_oracle_generator with a seed whose high word is set; the row ids cross
    2^32 (counter word c1 of the generator's stream)."""
    for seed, row0, far in ((2 ** 63 + 12345, 0, 0.0), (2 ** 64 - 7, 2 ** 32 - 1500, 0.2)):
        R, T, avg = 4000, 1500, 6
        prob = gpu.Problem.synthetic(R, T, avg, seed=seed, row0=row0, mapped_reads=R, sort=False, far_fraction=far)
        rp, ci = prob.download()
        p, _ = orc.synth_problem(R=R, T=T, avg_hits=avg, seed=seed, row0=row0, sort=False, far_fraction=far)
        assert np.array_equal(rp, p.row_ptr) and np.array_equal(ci, p.col_idx) and np.array_equal(prob.l(), p.l)
        low, _ = orc.synth_problem(R=R, T=T, avg_hits=avg, seed=seed & 0xFFFFFFFF, row0=row0, sort=False, far_fraction=far)
        assert not np.array_equal(low.col_idx[:200], p.col_idx[:200])
        prob.close()


def test_mmdiff_with_a_high_seed_word_equals_the_restatement(gpu):
    """The smallest design of tests/test_gpu_mmdiff.py (-de 3 3) on 12 features: burn-in, one tuning batch, sampling -- every key of
    results() against tests/mmdiff_ref.py's BMS with the same 64-bit seed (its CLI wrapper masks the seed; the class does not)."""
    import mmdiff_ref as R
    from mmseq_amd.diff import Diff
    from test_gpu_mmdiff import synth
    seed = (0xC0FFEE << 32) | 5
    y, e, _, _ = synth(12, 6, seed=101, groups=[3, 3])
    design = R.de_design([3, 3])
    res = []
    for s, h in ((seed, Diff(y, e, *design, seed=seed)), (seed, R.BMS(y, e, *design, seed=seed)), (5, Diff(y, e, *design, seed=5))):
        h.burnin(160)
        assert h.tune_batch() == 12
        h.sample(96)
        res.append(h.results())
    got, want, low = res
    assert set(got) == set(want)
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert not np.array_equal(got["gamma_mean"], low["gamma_mean"])          # the high word reaches mmdiff's streams


def test_cli_sign_extends_a_negative_seed(gpu, tmp_path):
    """`mmseq -seed -7` is the library's seed 2^64 - 7 (the int is sign-extended): not the chain of -seed 7, and every table and the
    trace equal the Python pipeline's with that seed, compared as tests/test_cli.py::test_full_run_matches_python_pipeline compares."""
    from oracle import host_oracle as H
    from test_cli import _same_number, _table, _trace_file, dataset, run
    h = dataset()
    p = tmp_path / "in.hits"
    p.write_bytes(H.write_hits_text(h))
    neg, pos = str(tmp_path / "neg"), str(tmp_path / "pos")
    for seed, out in (("-7", neg), ("7", pos)):
        r = run(["-gibbs_iter", "1024", "-seed", seed, str(p), out], timeout=300)
        assert r.returncode == 0, r.stderr.decode()
    for ext in (".mmseq", ".identical.mmseq", ".gene.mmseq"):
        assert open(neg + ext).read() != open(pos + ext).read(), ext
    assert gzip.open(neg + ".trace_gibbs.gz").read() != gzip.open(pos + ".trace_gibbs.gz").read()
    e = H.expected_run(h, seed=2 ** 64 - 7, gibbs_iter=1024)
    ids, rows = _trace_file(neg + ".trace_gibbs.gz")
    assert ids == e["ingest"]["index_sid"] and rows == [[H.fmt6(v) for v in e["trace"][:, s]] for s in range(1024)]
    _, hdr, tab = _table(neg + ".mmseq")
    assert [t["feature_id"] for t in tab] == h.names
    for got, exp in zip(tab, e["transcripts"]):
        for col in hdr[1:14]:
            assert _same_number(got[col], exp[col]), (got["feature_id"], col, got[col], exp[col])
        for a, b in zip(got[hdr[14]].split(","), exp["percentiles"]):
            assert _same_number(a, b)
        for a, b in zip(got[hdr[15]].split(","), exp["percentiles_proportion"]):
            assert _same_number(a, b)
    _, hdr, tab = _table(neg + ".identical.mmseq")
    for got, exp in zip(tab, e["identical"]):
        assert got["feature_id"] == exp["feature_id"]
        for col in hdr[1:10]:
            assert _same_number(got[col], exp[col]), (got["feature_id"], col, got[col], exp[col])
    _, hdr, tab = _table(neg + ".gene.mmseq")
    assert [t["feature_id"] for t in tab] == e["gene_ids"]
    for got, exp in zip(tab, e["genes"]):
        for col in hdr[1:10]:
            assert _same_number(got[col], exp[col]), (got["feature_id"], col, got[col], exp[col])
