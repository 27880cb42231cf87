"""The convergence diagnostics across chains on the device (mmg_convergence_*) against tests/convergence_ref.py: traces from the host
(every shape edge, ties, constant series, slab edges), a four-chain sampler with simulated isoforms, identical sets and genes, the
CLI's -convergence tables, and the error paths."""
import ctypes as C
import gzip
import math
import os
import subprocess

import numpy as np
import pytest

import convergence_ref as R
from oracle import host_oracle as H
from test_cli import MMSEQ, dataset

pytestmark = pytest.mark.gpu
KINDS = ("rhat", "ess_bulk", "ess_tail")


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.abs(a - b) / np.maximum(np.abs(b), 1e-300)
    same = (np.isnan(a) & np.isnan(b)) | (a == b)
    return np.where(same, 0.0, r)


def _check(got, ref, label=""):
    """rhat to 1e-10, ESS to 1e-8; an ESS outside is allowed only where the reference's Geyer truncation was decided within rounding
    of 0 (reported: expected 0)"""
    assert np.all(_rel(got["rhat"], ref["rhat"]) <= 1e-10), (label, got["rhat"], ref["rhat"])
    outliers = 0
    for k, m in (("ess_bulk", "margin_bulk"), ("ess_tail", "margin_tail")):
        bad = _rel(got[k], ref[k]) > 1e-8
        assert not np.any(bad & (ref[m] > 1e-9)), (label, k, np.flatnonzero(bad), got[k][bad], ref[k][bad])
        outliers += int(bad.sum())
    print("%s: %d Geyer truncations decided within rounding of 0" % (label, outliers))
    return outliers


def _ar1(rng, C_, S, count, phi):
    x = np.empty((C_, S, count))
    x[:, 0] = rng.normal(size=(C_, count)) / math.sqrt(1 - phi * phi)
    for s in range(1, S):
        x[:, s] = phi * x[:, s - 1] + rng.normal(size=(C_, count))
    return x


def _mixed(rng, C_, S, count):
    """iid, AR(1), a shifted chain, an inflated chain, heavy ties and one constant series, by turns"""
    x = rng.normal(size=(C_, S, count))
    x[:, :, 1::6] = _ar1(rng, C_, S, x[:, :, 1::6].shape[2], 0.9)
    x[C_ - 1, :, 2::6] += 3.0
    x[0, :, 3::6] *= 4.0
    x[:, :, 4::6] = rng.integers(0, 4, size=x[:, :, 4::6].shape)
    x[:, :, 5::6] = np.exp(x[:, :, 5::6])
    x[:, :, count // 2] = 1.25
    return x


@pytest.mark.parametrize("C_,S,count", [(4, 200, 60), (1, 101, 30), (3, 4, 40), (2, 5, 12), (4, 2048, 7), (6, 2048, 5), (1, 8192, 3),
                                        (3, 4096, 2), (4, 64, 1), (2, 64, 257)])
def test_traces_match_the_reference(gpu, C_, S, count):
    rng = np.random.default_rng(C_ * 1000 + S + count)
    x = _mixed(rng, C_, S, count)
    got = gpu.convergence_of_traces(x)
    ref = R.diagnostics_of_traces(x)
    _check(got, ref, "C=%d S=%d count=%d" % (C_, S, count))
    assert np.isnan(got["rhat"][count // 2]) and np.isnan(got["ess_bulk"][count // 2]) and np.isnan(got["ess_tail"][count // 2])
    again = gpu.convergence_of_traces(x)
    for k in KINDS:
        assert np.array_equal(got[k], again[k], equal_nan=True)        # bit-identical reruns


@pytest.mark.parametrize("slab", [1, 2, 5, 64])
def test_slab_edges(gpu, slab):
    rng = np.random.default_rng(77)
    for C_, S, count in ((3, 50, 11), (4, 3072, 5)):             # (the second: C S = 12288, the workspace path)
        x = _mixed(rng, C_, S, count)
        whole = gpu.convergence_of_traces(x)
        with gpu.options(conv_slab=slab):
            part = gpu.convergence_of_traces(x)
        for k in KINDS:
            assert np.array_equal(whole[k], part[k], equal_nan=True), (slab, C_, S, k)
        if S == 3072:
            _check(part, R.diagnostics_of_traces(x), "slab %d, C S = 12288" % slab)


def test_argument_errors(gpu):
    from mmseq_amd._lib import MMGError
    with pytest.raises(MMGError) as e:
        gpu.convergence_of_traces(np.ones((2, 3, 4)))
    assert e.value.code == 1 and "S >= 4" in str(e.value)
    with pytest.raises(MMGError) as e:
        gpu.convergence_of_traces(np.ones((0, 8, 4)))
    assert e.value.code == 1


def _sampler_case(gpu, orc, S=256, keep_trace=True):
    p, _ = orc.synth_problem(R=30000, T=900, avg_hits=5, seed=9, sort=False)
    n = p.n
    rng = np.random.default_rng(9)
    txo = (rng.permutation(n).astype(np.uint64) // np.uint64(3)) << np.uint64(32)
    prob = gpu.Problem.from_csr(p.row_ptr, p.col_idx, p.l, tx_order=txo)
    mu0, _ = prob.start_values()
    s = gpu.Sampler(prob, mu0, seed=31, n_chains=4, gibbs_iter=2 * S, trace_len=S, keep_trace=keep_trace)
    s.run(2 * S)
    nv = 40
    vid = (10_000 + np.arange(nv) * 7).astype(np.uint64)
    vscale = rng.uniform(0.01, 2.0, nv)
    members = rng.permutation(n + nv)
    genes, i = [], 0
    while i < members.size:
        sz = int(rng.integers(1, 6))
        genes.append([int(m) for m in members[i:i + sz]])
        i += sz
    identical = [[3, 4], [10, 11, 12], [700], [n + 5, 8]]
    return prob, s, n, dict(virtual_id=vid, virtual_scale=vscale, identical=identical, genes=genes)


def test_sampler_series_match_the_reference(gpu, orc):
    S = 256
    prob, s, n, desc = _sampler_case(gpu, orc, S)
    mu_before = [s.mu(c) for c in range(4)]
    cv = gpu.Convergence(s, **desc)
    vid, vscale = desc["virtual_id"], desc["virtual_scale"]
    full = []
    for c in range(4):
        V = np.stack([orc.simu_gamma_trace_keyed(31, c, orc.TAG_SIMU, int(vid[v]), 0.1, vscale[v], S) for v in range(len(vid))])
        full.append(np.concatenate([s.trace(c), V]))            # member index -> trace of chain c, [n + nv, S]
    full = np.stack(full)                                        # [C, n + nv, S]

    def groups(gs):
        out = np.zeros((4, len(gs), S))
        for g, ms in enumerate(gs):
            for m in ms:
                out[:, g] += full[:, m]                          # members added in the given order
        return out

    series = {gpu.SERIES_TRANSCRIPT: full[:, :n], gpu.SERIES_VIRTUAL: full[:, n:], gpu.SERIES_IDENTICAL: groups(desc["identical"]),
              gpu.SERIES_GENE: groups(desc["genes"])}
    total = 0
    for kind, tr in series.items():
        ref = R.diagnostics_of_traces(tr.transpose(0, 2, 1))
        total += _check(cv.series(kind), ref, "kind %d" % kind)
    print("sampler: %d outliers in all" % total)
    again = gpu.Convergence(s, **desc)
    for kind in series:
        for k in KINDS:
            assert np.array_equal(cv.series(kind)[k], again.series(kind)[k], equal_nan=True)
    with gpu.options(conv_slab=7):
        sl = gpu.Convergence(s, **desc)
    for kind in series:
        for k in KINDS:
            assert np.array_equal(cv.series(kind)[k], sl.series(kind)[k], equal_nan=True)
    for c in range(4):
        assert np.array_equal(s.mu(c), mu_before[c])              # the sampler's state is untouched


def test_keep_trace_0_is_refused(gpu, orc):
    from mmseq_amd._lib import MMGError
    prob, s, n, desc = _sampler_case(gpu, orc, S=64, keep_trace=False)
    with pytest.raises(MMGError) as e:
        gpu.Convergence(s, **desc)
    assert e.value.code == 4 and "keep_trace" in str(e.value)


def test_failed_acquisitions_give_back_everything(gpu, orc):
    from mmseq_amd import _lib
    from mmseq_amd._lib import MMGError
    lib = _lib.load()
    prob, s, n, desc = _sampler_case(gpu, orc, S=64)

    def live():
        c = (C.c_int64 * 3)()
        _lib.check(lib.mmg_selftest_live(c))
        return list(c)

    want = gpu.Convergence(s, **desc).series(gpu.SERIES_GENE)
    base = live()
    v = 0
    try:
        while True:
            _lib.check(lib.mmg_selftest_option(_lib.OPT_FAIL_ALLOC, v))
            try:
                cv = gpu.Convergence(s, **desc)
            except MMGError as e:
                assert e.code == 3 and str(e)
                assert live() == base, v
                v += 1
                continue
            break
    finally:
        lib.mmg_selftest_option(_lib.OPT_FAIL_ALLOC, -1)
    assert v >= 5
    got = cv.series(gpu.SERIES_GENE)
    for k in KINDS:
        assert np.array_equal(got[k], want[k], equal_nan=True)
    cv.close()
    assert live() == base


# ------------------------------------------------------------------------------------------ the CLI
def _run(args):
    return subprocess.run([MMSEQ] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)


def _conv_table(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    return lines[0], lines[1].split("\t"), [ln.split("\t") for ln in lines[2:-1]]


def _ids(path):
    return [ln.split("\t")[0] for ln in open(path).read().split("\n")[2:-1]]


def _same6(txt, val):
    if math.isnan(val):
        return txt in ("nan", "-nan")
    if math.isinf(val):
        return txt == ("inf" if val > 0 else "-inf")
    return float(txt) == float("%.6g" % val)


def test_cli_writes_the_tables_of_gibbs_convergence(tmp_path):
    from mmseq_amd import gibbs
    h = dataset()
    p = tmp_path / "in.hits"
    p.write_bytes(H.write_hits_text(h))
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    r = _run(["-gibbs_iter", "2048", "-seed", "77", "-chains", "4", "-convergence", str(p), a])
    assert r.returncode == 0, r.stderr.decode()
    r2 = _run(["-gibbs_iter", "2048", "-seed", "77", "-chains", "4", str(p), b])
    assert r2.returncode == 0, r2.stderr.decode()
    # every other output is what a run without the flag writes
    for ext in (".mmseq", ".identical.mmseq", ".gene.mmseq", ".k", ".M"):
        assert open(a + ext, "rb").read() == open(b + ext, "rb").read(), ext
    for ext in (".trace_gibbs.gz", ".identical.trace_gibbs.gz", ".gene.trace_gibbs.gz", ".prop.trace_gibbs.gz"):
        assert gzip.open(a + ext).read() == gzip.open(b + ext).read(), ext
    for ext in (".convergence", ".identical.convergence", ".gene.convergence"):
        assert not os.path.exists(b + ext)
    # ids and order: the rows of the three tables
    for tab, conv in ((".mmseq", ".convergence"), (".identical.mmseq", ".identical.convergence"), (".gene.mmseq", ".gene.convergence")):
        first, hdr, rows = _conv_table(a + conv)
        assert first == "# chains 4, samples per chain 1024" and hdr == ["feature_id", "rhat", "ess_bulk", "ess_tail"]
        assert [row[0] for row in rows] == _ids(a + tab)
    # the values: gibbs.Convergence on the problem the CLI builds (oracle.host_oracle's restatement of the CLI's ingest)
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
    s = gibbs.Sampler(prob, mu_em, alpha=0.1, beta=0.1, seed=77, n_chains=4, gibbs_iter=2048, trace_len=1024)
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
    cv = gibbs.Convergence(s, virtual_id=vid, virtual_scale=vscale, identical=identical, genes=genes)
    T, V, I, G = (cv.series(kind) for kind in range(4))
    _, _, rows = _conv_table(a + ".convergence")
    for row in rows:
        src, i = (T, obs[row[0]]) if row[0] in obs else (V, simu[row[0]])
        for txt, key in zip(row[1:], KINDS):
            assert _same6(txt, src[key][i]), (row, key, src[key][i])
    for path, src in ((".identical.convergence", I), (".gene.convergence", G)):
        _, _, rows = _conv_table(a + path)
        for i, row in enumerate(rows):
            for txt, key in zip(row[1:], KINDS):
                assert _same6(txt, src[key][i]), (path, row, key, src[key][i])


def test_cli_one_chain(tmp_path):
    h = dataset(n_reads=1500)
    p = tmp_path / "in.hits"
    p.write_bytes(H.write_hits_text(h))
    out = str(tmp_path / "o")
    r = _run(["-gibbs_iter", "1024", "-chains", "1", "-convergence", str(p), out])
    assert r.returncode == 0, r.stderr.decode()
    first, hdr, rows = _conv_table(out + ".convergence")
    assert first == "# chains 1, samples per chain 1024" and len(rows) == len(h.names)
    assert any(np.isfinite(float(row[1])) for row in rows)
