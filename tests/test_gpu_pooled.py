"""The posterior summary over all chains on the device (mmg_pooled_*) against tests/pooled_ref.py: traces from the host (every shape
edge, ties, constant, NaN and +inf series, slab edges), a four-chain sampler with simulated isoforms, identical sets and genes (the
chains' own columns against gibbs.Summary, the pooled columns and the proportions against the reference), the memory formula, the error
paths and the CLI's -pool tables."""
import ctypes as C
import gc
import gzip
import math

import numpy as np
import pytest

import pooled_ref as R
from key_space_checks import probit_as241
from oracle import host_oracle as H
from test_cli import dataset
from test_gpu_convergence import _ids, _mixed, _run, _same6, _sampler_case

pytestmark = pytest.mark.gpu
COLS = ("log_mean", "var", "tau", "mcse2", "rc", "percentiles")


def _dlog(gpu):
    return lambda x: gpu.selftest_math(x, 0)["log"]        # mmg_math.h: dlog, evaluated on the device


def _same(got, ref, keys, label=""):
    for k in keys:
        assert got[k].shape == ref[k].shape, (label, k)
        assert np.array_equal(got[k], ref[k], equal_nan=True), (label, k, np.flatnonzero(~((got[k] == ref[k]) | (np.isnan(got[k]) & np.isnan(ref[k])))))


def _positive(rng, C_, S, count):
    """_mixed of the convergence test made positive (iid, AR(1), a shifted and an inflated chain, heavy ties, one constant series), with a
    NaN in one series and a +inf in another where there are series to spare"""
    x = np.exp(_mixed(rng, C_, S, count))
    if count >= 2:
        x[C_ - 1, S // 2, 0] = np.nan
    if count >= 3:
        x[0, S - 1, count - 1] = np.inf
    return x


@pytest.mark.parametrize("C_,S,count", [(1, 1024, 5), (3, 100, 60), (2, 4, 40), (2, 5, 12), (8, 1024, 3), (3, 4096, 2), (5, 256, 1), (2, 64, 257)])
def test_traces_match_the_reference(gpu, C_, S, count):
    rng = np.random.default_rng(C_ * 1000 + S + count)
    x = _positive(rng, C_, S, count)
    N = C_ * S
    pidx = [0, N - 1, -1, N, N // 2, N // 3]
    got = gpu.pooled_of_traces(x, pidx)
    ref = R.pooled_of_traces(x, pidx, log=_dlog(gpu))
    _same(got, ref, COLS, "C=%d S=%d count=%d" % (C_, S, count))
    assert np.isnan(got["percentiles"][:, 2:4]).all()
    assert (got["rc"] == (0 if S & (S - 1) == 0 and S >= 4 else 201)).all()
    if C_ == 1:                                                # the copy rule: the chain's own columns
        _same(got, dict(log_mean=ref["c_mean"][:, 0], var=ref["c_var"][:, 0], tau=ref["c_tau"][:, 0]), ("log_mean", "var", "tau"))
    none = gpu.pooled_of_traces(x)                               # np = 0
    assert none["percentiles"].shape == (count, 0)
    _same(none, ref, COLS[:5], "np = 0")
    again = gpu.pooled_of_traces(x, pidx)
    _same(again, got, COLS, "rerun")                             # bit-identical reruns


@pytest.mark.parametrize("slab", [1, 2, 5, 64])
def test_slab_edges(gpu, slab):
    rng = np.random.default_rng(77)
    for C_, S, count in ((3, 50, 11), (4, 3072, 5)):             # (the second: C S = 12288, the workspace path)
        x = _positive(rng, C_, S, count)
        pidx = [0, C_ * S - 1, C_ * S // 2]
        whole = gpu.pooled_of_traces(x, pidx)
        with gpu.options(pool_slab=slab):
            part = gpu.pooled_of_traces(x, pidx)
        _same(part, whole, COLS, "slab %d C=%d S=%d" % (slab, C_, S))


# ------------------------------------------------------------------------------------------ from a sampler
PIDX = [0, 51, 512, 1023, -1, 1024]


@pytest.fixture(scope="module")
def case(gpu, orc):
    """the four-chain sampler of the convergence test, one gene taken away so that its members are outside every gene, the host copies
    of every series [C, count, S] and the proportions"""
    S = 256
    prob, s, n, desc = _sampler_case(gpu, orc, S)
    drop = max(g for g, ms in enumerate(desc["genes"]) if min(ms) < n)      # the last gene with a transcript: its members end up outside
    outside = desc["genes"][drop]
    desc = dict(desc, genes=desc["genes"][:drop] + desc["genes"][drop + 1:])
    vid, vscale = desc["virtual_id"], desc["virtual_scale"]
    nv = len(vid)
    full = []
    for c in range(4):
        V = np.stack([orc.simu_gamma_trace_keyed(31, c, orc.TAG_SIMU, int(vid[v]), 0.1, vscale[v], S) for v in range(nv)])
        full.append(np.concatenate([s.trace(c), V]))            # member index -> trace of chain c, [n + nv, S]
    full = np.stack(full)                                        # [C, n + nv, S]

    def groups(gs):
        out = np.zeros((4, len(gs), S))
        for g, ms in enumerate(gs):
            for m in ms:
                out[:, g] += full[:, m]                          # members added in the given order
        return out

    t_gene = groups(desc["genes"])
    series = {gpu.SERIES_TRANSCRIPT: full[:, :n], gpu.SERIES_VIRTUAL: full[:, n:], gpu.SERIES_IDENTICAL: groups(desc["identical"]),
              gpu.SERIES_GENE: t_gene}
    gene_of = np.full(n + nv, -1)
    for g, ms in enumerate(desc["genes"]):
        gene_of[ms] = g
    with np.errstate(invalid="ignore", divide="ignore"):
        prop = np.where(gene_of[None, :, None] >= 0, full / t_gene[:, gene_of], np.nan)
    multi = np.array([g >= 0 and len(desc["genes"][g]) > 1 for g in gene_of])
    pooled = gpu.PooledSummary(s, percentile_index=PIDX, **desc)
    return dict(prob=prob, s=s, n=n, nv=nv, S=S, desc=desc, series=series, prop=prop, multi=multi, gene_of=gene_of, outside=outside, pooled=pooled)


def test_chain_columns_are_the_single_chain_summaries(gpu, case):
    """the plumbing: the chains' columns come from the summary's own kernel on the slab layout"""
    s, ps, desc = case["s"], case["pooled"], case["desc"]
    for c in range(4):
        q = gpu.Summary(s, chain=c)
        _same(ps.chain_series(gpu.SERIES_TRANSCRIPT, c), q.series(gpu.SERIES_TRANSCRIPT), ("log_mean", "var", "tau", "rc"), "chain %d" % c)
        q.close()
    q = gpu.Summary(s, chain=0, **desc)
    for kind in range(4):
        _same(ps.chain_series(kind, 0), q.series(kind), ("log_mean", "var", "tau", "rc"), "kind %d" % kind)
    q.close()


def test_pooled_columns_match_the_reference(gpu, case):
    ps = case["pooled"]
    for kind, tr in case["series"].items():
        ref = R.pooled_of_traces(tr.transpose(0, 2, 1), PIDX, log=_dlog(gpu))
        _same(ps.series(kind), ref, COLS, "kind %d" % kind)
        for c in range(4):
            _same(ps.chain_series(kind, c), dict(log_mean=ref["c_mean"][:, c], var=ref["c_var"][:, c], tau=ref["c_tau"][:, c], rc=ref["c_rc"][:, c]),
                  ("log_mean", "var", "tau", "rc"), "kind %d chain %d" % (kind, c))
    again = gpu.PooledSummary(case["s"], percentile_index=PIDX, **case["desc"])
    for kind in range(4):
        _same(again.series(kind), ps.series(kind), COLS, "rerun, kind %d" % kind)


def test_pooled_proportions_match_the_reference(gpu, case):
    ps, n, prop, multi, gene_of = case["pooled"], case["n"], case["prop"], case["multi"], case["gene_of"]
    assert (gene_of[:n] < 0).any() and (~multi[:n] & (gene_of[:n] >= 0)).any()       # both special cases occur among the transcripts
    for kind, sl in ((gpu.SERIES_TRANSCRIPT, slice(0, n)), (gpu.SERIES_VIRTUAL, slice(n, None))):
        got = ps.proportions(kind)
        ref = R.pooled_proportions(prop[:, sl].transpose(0, 2, 1), multi[sl], PIDX)
        _same(got, ref, ("mean", "percentiles"), "kind %d" % kind)
        mu, out = multi[sl], gene_of[sl] < 0
        # the probit columns: bit for bit against AS 241 transcribed on the device's own logarithm, sums in sample order ...
        exact = R.pooled_proportions(prop[:, sl].transpose(0, 2, 1), multi[sl], PIDX, probit=lambda p: probit_as241(p, _dlog(gpu)))
        assert np.array_equal(got["probit_mean"][mu], exact["probit_mean"][mu]) and np.array_equal(got["probit_sd"][mu], exact["probit_sd"][mu])
        assert mu.sum() > 30
        # ... and to the accuracy of that algorithm against scipy's ndtri, as before
        np.testing.assert_allclose(got["probit_mean"][mu], ref["probit_mean"][mu], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(got["probit_sd"][mu], ref["probit_sd"][mu], rtol=1e-7)
        assert np.isinf(got["probit_mean"][~mu]).all() and (got["probit_mean"][~mu] > 0).all() and np.isnan(got["probit_sd"][~mu]).all()
        assert np.isnan(got["mean"][out]).all() and np.isnan(got["percentiles"][out]).all()          # outside every gene
        assert np.isfinite(got["mean"][~out]).all()


def _formula(C_, S, n, nv, identical, genes, np_, slab=0):
    """mmg_pooled_device_bytes as include/mmgibbs.h states it"""
    ni, ng = len(identical), len(genes)
    cap = max(1, min(max(n, nv, ni, ng), (256 << 20) // (8 * C_ * S)))
    if slab:
        cap = min(cap, slab)
    gene_of = {}
    for g, ms in enumerate(genes):
        for m in ms:
            gene_of[m] = g
    L = 0
    for lo, hi in ((0, n), (n, n + nv)):
        for t0 in range(lo, hi, cap):
            L = max(L, sum(len(genes[g]) for g in {gene_of[m] for m in range(t0, min(t0 + cap, hi)) if m in gene_of}))
    b = 16 * max(nv, 1) + 8 * (ni + 1 if ni else 1) + 4 * max(sum(map(len, identical)), 1) + 8 * (ng + 1 if ng else 1) + 4 * max(sum(map(len, genes)), 1)
    b += 8 * C_ * S * max(nv, 1)
    b += 8 * cap * C_ * S + 16 * cap * S
    b += 8 * (cap + 1) + 4 * max(L, 1) + 5 * cap
    b += 28 * cap * C_ + 36 * cap + 8 * cap * max(np_, 1) + 4 * max(np_, 1) + 16 * max(S, 1)
    if S > 8192:
        b += 24 * 1024 * (1 << (S - 1).bit_length())
    if C_ * S > 8192:
        PP = 1 << (C_ * S - 1).bit_length()
        b += 8 * PP * max(1, min(1024, cap, (256 << 20) // (8 * PP)))
    return b


@pytest.mark.parametrize("slab", [0, 7, 100])
def test_memory_formula_and_slabs_of_a_sampler(gpu, case, slab):
    ps, desc, n, nv = case["pooled"], case["desc"], case["n"], case["nv"]
    assert ps.device_bytes() == _formula(4, case["S"], n, nv, desc["identical"], desc["genes"], len(PIDX))
    if not slab:
        return
    with gpu.options(pool_slab=slab):
        sl = gpu.PooledSummary(case["s"], percentile_index=PIDX, **desc)
    assert sl.device_bytes() == _formula(4, case["S"], n, nv, desc["identical"], desc["genes"], len(PIDX), slab)
    assert sl.device_bytes() < ps.device_bytes()
    for kind in range(4):
        _same(sl.series(kind), ps.series(kind), COLS, "slab %d kind %d" % (slab, kind))
    for kind in range(2):
        _same(sl.proportions(kind), ps.proportions(kind), ("mean", "probit_mean", "probit_sd", "percentiles"), "slab %d kind %d" % (slab, kind))


def test_argument_errors(gpu, orc):
    from mmseq_amd._lib import MMGError
    prob, s, n, desc = _sampler_case(gpu, orc, S=64, keep_trace=False)
    with pytest.raises(MMGError) as e:
        gpu.PooledSummary(s, **desc)
    assert e.value.code == 1 and "keep_trace" in str(e.value)
    for shape in ((0, 8, 4), (2, 0, 4)):
        with pytest.raises(MMGError) as e:
            gpu.pooled_of_traces(np.ones(shape))
        assert e.value.code == 1 and str(e.value).split(": ", 1)[1]


def test_failed_acquisitions_give_back_everything(gpu, orc):
    from mmseq_amd import _lib
    from mmseq_amd._lib import MMGError
    lib = _lib.load()
    prob, s, n, desc = _sampler_case(gpu, orc, S=64)

    def live():
        c = (C.c_int64 * 3)()
        _lib.check(lib.mmg_selftest_live(c))
        return list(c)

    first = gpu.PooledSummary(s, percentile_index=[0, 100], **desc)
    want, want_p = first.series(gpu.SERIES_GENE), first.proportions(gpu.SERIES_TRANSCRIPT)
    first.close()
    gc.collect()                                                 # handles of earlier tests that only a collection frees must not go mid-sweep
    base = live()
    v = 0
    try:
        while True:
            _lib.check(lib.mmg_selftest_option(_lib.OPT_FAIL_ALLOC, v))
            try:
                ps = gpu.PooledSummary(s, percentile_index=[0, 100], **desc)
            except MMGError as e:
                assert e.code == 3 and str(e)
                assert live() == base, v
                v += 1
                continue
            break
    finally:
        lib.mmg_selftest_option(_lib.OPT_FAIL_ALLOC, -1)
    assert v >= 20                                               # the stream and every buffer of the pass
    assert live() == base                                        # nothing is held after create
    _same(ps.series(gpu.SERIES_GENE), want, COLS)
    _same(ps.proportions(gpu.SERIES_TRANSCRIPT), want_p, ("mean", "probit_mean", "probit_sd", "percentiles"))
    ps.close()
    assert live() == base


# ------------------------------------------------------------------------------------------ the CLI
def _table(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    return lines[1].split("\t"), [ln.split("\t") for ln in lines[2:-1]]


def _same6_list(txt, vals):
    parts = txt.split(",")
    return len(parts) == len(vals) and all(_same6(t, v) for t, v in zip(parts, vals))


def test_cli_pool_writes_the_columns_of_pooled_summary(tmp_path):
    from mmseq_amd import gibbs
    h = dataset()
    p = tmp_path / "in.hits"
    p.write_bytes(H.write_hits_text(h))
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    r = _run(["-gibbs_iter", "2048", "-seed", "77", "-chains", "3", "-pool", str(p), a])
    assert r.returncode == 0, r.stderr.decode()
    r2 = _run(["-gibbs_iter", "2048", "-seed", "77", "-chains", "3", str(p), b])
    assert r2.returncode == 0, r2.stderr.decode()
    # every output but the three tables is what a run without the flag writes
    for ext in (".k", ".M"):
        assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), ext
    for ext in (".trace_gibbs.gz", ".identical.trace_gibbs.gz", ".gene.trace_gibbs.gz", ".prop.trace_gibbs.gz"):
        assert gzip.open(a + ext).read() == gzip.open(b + ext).read(), ext
    assert open(a + ".mmseq", "rb").read() != open(b + ".mmseq", "rb").read()
    for ext in (".mmseq", ".identical.mmseq", ".gene.mmseq"):
        assert _ids(a + ext) == _ids(b + ext) and open(a + ext).readline() == open(b + ext).readline()
    # the values: gibbs.PooledSummary on the problem the CLI builds (oracle.host_oracle's restatement of the CLI's ingest)
    g = H.ingest(h)
    sid, rows_, k = g["index_sid"], g["rows"], g["k"]
    n, N = len(sid), g["mapped"]
    l = np.array([h.efflen[s_] * float(N) / 1e9 for s_ in sid])
    hdr_pos = {name: i for i, name in enumerate(h.names)}
    gene_first, gene_of_t = {}, {}
    for gid, ts in h.genes.items():
        gene_first[gid] = min([hdr_pos[t] for t in ts if t in hdr_pos] or [0xffffffff])
        for t in ts:
            gene_of_t[t] = gid
    tkey = np.array([((min(gene_first[gene_of_t[s_]], hdr_pos[s_]) if s_ in gene_of_t else hdr_pos[s_]) << 32) | hdr_pos[s_] for s_ in sid], np.uint64)
    rp = np.cumsum([0] + [len(r_) for r_ in rows_]).astype(np.uint64)
    ci = np.array([c for r_ in rows_ for c in r_], np.uint32)
    prob = gibbs.Problem.from_csr(rp, ci, l, k=np.asarray(k, np.uint32), tx_order=tkey)
    mu0, _ = prob.start_values()
    mu_em = prob.em(mu0, max_iter=1000, epsilon=0.1)[0]
    s = gibbs.Sampler(prob, mu_em, alpha=0.1, beta=0.1, seed=77, n_chains=3, gibbs_iter=2048, trace_len=1024)
    s.run(2048)
    obs = g["sid_index"]
    vid, vscale, simu, genes = [], [], {}, []
    for gid, ts in h.genes.items():
        ms = []
        for name in ts:
            if name in obs:
                ms.append(obs[name])
            else:
                simu[name] = len(vid)
                ms.append(n + len(vid))
                vid.append(hdr_pos[name])
                vscale.append(1.0 / (0.1 + h.efflen[name] * float(N) / 1e9))
        genes.append(ms)
    identical = [[obs[name] for name in st if name in obs] for st in h.identical]
    NS = 3 * 1024
    pidx = [int(math.floor(q / 100.0 * (NS - 1) + 0.5)) for q in (5, 25, 50, 75, 95)]
    ps = gibbs.PooledSummary(s, virtual_id=vid, virtual_scale=vscale, identical=identical, genes=genes, percentile_index=pidx)
    T, V, I, G = (ps.series(kind) for kind in range(4))
    pT, pV = ps.proportions(0), ps.proportions(1)

    def log_cols(src, i):
        assert src["rc"][i] == 0
        return [src["log_mean"][i], math.sqrt(src["var"][i]), math.sqrt(src["mcse2"][i]), src["tau"][i]]

    hdr, rows = _table(a + ".mmseq")
    col = {name: j for j, name in enumerate(hdr)}
    pc, ppc = len(hdr) - 2, len(hdr) - 1
    seen = [0, 0]
    for row in rows:
        if row[0] in obs:
            i = obs[row[0]]
            assert row[col["observed"]] == "1"
            for txt, val in zip(row[1:5], log_cols(T, i)):
                assert _same6(txt, val), (row, val)
            src, pr = T, pT
            seen[0] += 1
        else:
            i = simu[row[0]]
            assert row[col["observed"]] == "0"
            src, pr = V, pV
            seen[1] += 1
        for name, key in (("mean_proportion", "mean"), ("mean_probit_proportion", "probit_mean"), ("sd_probit_proportion", "probit_sd")):
            assert _same6(row[col[name]], pr[key][i]), (row, name, pr[key][i])
        assert _same6_list(row[pc], src["percentiles"][i]) and _same6_list(row[ppc], pr["percentiles"][i]), row
    assert seen[0] == n and seen[1] == len(vid) > 0
    hdr, rows = _table(a + ".identical.mmseq")
    assert len(rows) == len(identical)
    for i, row in enumerate(rows):
        if not identical[i]:                                     # a set that was never hit: the closed-form row
            assert row[8] == "0"
            continue
        for txt, val in zip(row[1:5], log_cols(I, i)):
            assert _same6(txt, val), (row, val)
        assert _same6_list(row[-1], I["percentiles"][i]), row
    hdr, rows = _table(a + ".gene.mmseq")
    assert len(rows) == len(genes)
    unobserved = 0
    for i, row in enumerate(rows):
        if any(m < n for m in genes[i]):
            want = log_cols(G, i)
        else:                                                    # simulated isoforms only: independent draws, mcse = sd / sqrt(all draws)
            sd = math.sqrt(G["var"][i])
            want = [G["log_mean"][i], sd, sd / math.sqrt(NS), 1.0]
            unobserved += 1
        for txt, val in zip(row[1:5], want):
            assert _same6(txt, val), (row, val)
        assert _same6_list(row[-1], G["percentiles"][i]), row
    assert unobserved > 0


def test_cli_pool_with_one_chain_writes_the_bytes_of_one_chain(tmp_path):
    h = dataset(n_reads=1500)
    p = tmp_path / "in.hits"
    p.write_bytes(H.write_hits_text(h))
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    r = _run(["-gibbs_iter", "1024", "-chains", "1", "-pool", str(p), a])
    assert r.returncode == 0, r.stderr.decode()
    r2 = _run(["-gibbs_iter", "1024", "-chains", "1", str(p), b])
    assert r2.returncode == 0, r2.stderr.decode()
    for ext in (".mmseq", ".identical.mmseq", ".gene.mmseq", ".k", ".M"):
        assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), ext
