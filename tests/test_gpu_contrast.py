"""mmg_contrast_* on the device (mmseq_amd.Contrast, mmseq -contrasts) against tests/contrast_ref.py: the series bit for bit with the
library's own logarithm, the summaries against numpy and the pinned Sokal, slab edges, the sampler's trace taken on the device with
simulated isoforms, the handle's memory formula and error codes, and the CLI's table through mmdiff."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

from oracle import host_oracle as H
from test_cli import BIN_DIR, dataset, run
import contrast_ref as R

pytestmark = pytest.mark.gpu


def _dlog(gpu):
    return lambda x: gpu.selftest_math(x, 0)["log"]        # mmg_math.h: dlog, evaluated on the device


def _traces(rng, n, S):
    return np.exp(rng.normal(0.0, 3.0, (n, S)))


def _edge_contrasts(rng, n):
    """sides of 1, 2, 63, 64, 65, 257 and 5 000 members; a member on both sides; the first and the last series; lists in an order
    unrelated to the members' (shuffled), contrasts in an order unrelated to their sizes"""
    pick = lambda k: [int(m) for m in rng.choice(n, k, replace=False)]
    cs = [(pick(5000), pick(257)), ([0], [n - 1]), (pick(63), pick(2)), ([n - 1, 0], pick(64)), (pick(65), [7]),
          ([11], [3, 11, 4999]), (pick(2), pick(5000)), ([n - 1], [n - 1]), (pick(257), pick(63)), (pick(64), pick(65))]
    return cs


def _check_summary(got, ref, S, pidx, orc):
    assert np.array_equal(got["p_gt"], ref["p_gt"])
    assert np.array_equal(got["percentiles"], ref["percentiles"], equal_nan=True)
    np.testing.assert_allclose(got["log_ratio"], ref["log_ratio"], rtol=1e-12, atol=1e-12)
    pow2 = S >= 4 and S & (S - 1) == 0
    assert (got["rc"] == (0 if pow2 else 200 if S < 4 else 201)).all()
    for c in range(ref["R"].shape[0]):
        if pow2 and ref["R"][c].any():
            rc, var, tau, m = orc.sokal(ref["R"][c])          # pinned to the reference's compiled sokal.cc (test_oracle_sokal.py)
            assert rc == 0
            np.testing.assert_allclose([got["var"][c], got["tau"][c]], [var, tau], rtol=1e-9)
        elif not pow2:
            assert got["var"][c] == 0.0 and got["tau"][c] == 0.0


@pytest.fixture
def slab_option(gpu):
    from mmseq_amd import _lib
    lib = _lib.load()
    yield lambda v: lib.mmg_selftest_option(_lib.OPT_CONTRAST_SLAB, v)
    lib.mmg_selftest_option(_lib.OPT_CONTRAST_SLAB, -1)


@pytest.mark.parametrize("S", [4, 63, 64, 65, 1024])
def test_series_bit_identity_and_summaries_at_the_edges(gpu, orc, S):
    from mmseq_amd import Contrast
    rng = np.random.default_rng(20 + S)
    n = 5003
    tr = _traces(rng, n, S)
    cs = _edge_contrasts(rng, n)
    pidx = [0, S // 2, S - 1]
    with Contrast.from_traces(tr, cs, pidx) as h:
        rows, got = h.rows(), h.summary()
        assert np.array_equal(h.rows(3, 4), rows[3:7])
    ref = R.contrast_ref(tr, cs, pidx, log=_dlog(gpu))
    assert np.array_equal(rows, ref["R"]), int((rows != ref["R"]).sum())
    np.testing.assert_allclose(rows, R.series(tr, cs)[0], rtol=1e-12, atol=1e-12)       # ... and np.log's
    assert (rows[7] == 0.0).all() and got["p_gt"][7] == 0.0 and got["var"][7] == 0.0 and got["log_ratio"][7] == 0.0
    _check_summary(got, ref, S, pidx, orc)


@pytest.mark.parametrize("S", [3, 1000, 16384])
def test_trace_lengths_sokal_refuses_and_the_global_workspace(gpu, orc, S):
    """3 samples: rc 200; 1 000: rc 201 with the mean and the order statistics still there; 16 384: sorted and transformed in the
    global workspace"""
    from mmseq_amd import Contrast
    rng = np.random.default_rng(S)
    tr = _traces(rng, 6, S)
    cs = [([0], [1]), ([2, 3], [4]), ([5], [0, 5]), ([1], [0])]
    pidx = [0, S // 2, S - 1, S]                               # (S: outside the series, NaN)
    with Contrast.from_traces(tr, cs, pidx) as h:
        rows, got = h.rows(), h.summary()
    ref = R.contrast_ref(tr, cs, pidx, log=_dlog(gpu))
    assert np.array_equal(rows, ref["R"])
    assert np.isnan(got["percentiles"][:, 3]).all() and np.isfinite(got["percentiles"][:, :3]).all() and np.isfinite(got["log_ratio"]).all()
    _check_summary(got, ref, S, pidx, orc)


@pytest.mark.parametrize("S", [4, 6, 8, 1024])
def test_contrast_summary_and_log_summary_share_their_bits(gpu, S):
    """k_contrast_summary on y = R and k_series_summary<., true> on y = log x run the same device functions: with R = dlog(x) - dlog(1)
    = dlog(x) the mean, Sokal's var and tau and the return code (6 samples: 201) are the same bits, not merely close"""
    from mmseq_amd import Contrast
    from mmseq_amd.collapse import summarize
    rng = np.random.default_rng(900 + S)
    n = 5
    x = _traces(rng, n, S)
    tr = np.vstack([x, np.ones((1, S))])
    with Contrast.from_traces(tr, [([j], [n]) for j in range(n)]) as h:
        got = h.summary()
    log_mean, var, tau, rc = summarize(np.ascontiguousarray(x.T), [[j] for j in range(n)])
    assert (rc == (201 if S == 6 else 0)).all() and np.array_equal(got["rc"], rc)
    assert np.array_equal(got["log_ratio"], log_mean)
    assert np.array_equal(got["var"], var) and np.array_equal(got["tau"], tau)
    assert S == 6 or (var > 0.0).all()                             # (not equal because both are zero)


def test_slab_edges_and_reruns_give_the_same_bits(gpu, slab_option):
    from mmseq_amd import Contrast
    rng = np.random.default_rng(3)
    n, S = 40, 64
    tr = _traces(rng, n, S)
    cs = [([int(m) for m in rng.choice(n, int(rng.integers(1, 6)), replace=False)], [int(m) for m in rng.choice(n, int(rng.integers(1, 6)), replace=False)])
          for _ in range(15)]
    pidx = [0, 31, 63]
    with Contrast.from_traces(tr, cs, pidx) as h:
        whole, rows = h.summary(), h.rows()
        again = h.summary()                                    # a second _get on the same handle
        for k in whole:
            assert np.array_equal(whole[k], again[k], equal_nan=True), k
    with Contrast.from_traces(tr, cs, pidx) as h2:             # a second handle over the same input
        for k, v in h2.summary().items():
            assert np.array_equal(whole[k], v, equal_nan=True), k
    for cap in (1, 2, 7):
        assert slab_option(cap) == 0
        with Contrast.from_traces(tr, cs, pidx) as h:
            got = h.summary()
            for k in whole:
                assert np.array_equal(whole[k], got[k], equal_nan=True), (cap, k)
            assert np.array_equal(h.rows(), rows) and np.array_equal(h.rows(5, 6), rows[5:11]) and np.array_equal(h.rows(14, 1), rows[14:])


def _host_gamma_trace(seed, vid, shape, scale, n):
    from mmseq_amd import _lib
    out = np.empty(n)
    _lib.check(_lib.load().mmg_host_gamma_trace(int(seed), int(vid), float(shape), float(scale), int(n), out.ctypes.data_as(C.c_void_p)))
    return out


def test_sampler_path_equals_host_traces_and_the_gene_summaries(gpu, orc, slab_option):
    """a small generated problem, transcripts renumbered on the device, 9 isoforms without hits, 64 iterations: the device's gather of
    the chain's trace and its simulated traces against mmg_contrast_of_traces fed mmg_sampler_get_trace + mmg_host_gamma_trace"""
    from mmseq_amd import Contrast
    S, seed = 64, 3
    p, _ = orc.synth_problem(R=4000, T=150, avg_hits=4, seed=11, sort=False)
    n = p.n
    rng = np.random.default_rng(2)
    txo = (rng.permutation(n).astype(np.uint64) // np.uint64(4)) << np.uint64(32)
    prob = gpu.Problem.from_csr(p.row_ptr, p.col_idx, p.l, tx_order=txo)
    mu0, _ = prob.start_values()
    nv = 9
    vid = (500 + np.arange(nv) * 3).astype(np.uint64)
    vscale = rng.uniform(0.1, 1.0, nv)
    members = rng.permutation(n + nv)
    genes = [[int(m) for m in members[i:i + 3]] for i in range(0, members.size, 3)]
    smp = gpu.Sampler(prob, mu0, seed=seed, n_chains=2, gibbs_iter=S, trace_len=S)
    smp.run(S)
    q = gpu.Summary(smp, chain=0, virtual_id=vid, virtual_scale=vscale, genes=genes, percentile_index=[0])
    full = np.concatenate([smp.trace(0), np.stack([_host_gamma_trace(seed, vid[v], 0.1, vscale[v], S) for v in range(nv)])])
    G = len(genes)
    cs = [(genes[g], genes[(g + 1) % G]) for g in range(G)]                  # gene against gene
    cs += [([genes[g][0]], genes[g]) for g in range(G)]                      # first isoform / its gene
    cs += [([n + v], [int(rng.integers(0, n))]) for v in range(nv)]          # every simulated isoform against a transcript
    cs += [([0], [n - 1]), (list(range(n + nv - 1, -1, -1)), [n + nv - 1])]  # everything, backwards
    pidx = [0, 32, 63]
    for cap in (-1, 2):
        slab_option(cap)
        with Contrast.from_sampler(smp, q, cs, pidx) as a, Contrast.from_traces(full, cs, pidx) as b:
            sa, sb = a.summary(), b.summary()
            for k in sa:
                assert np.array_equal(sa[k], sb[k], equal_nan=True), (cap, k)
            rows = a.rows()
            assert np.array_equal(rows, b.rows(), equal_nan=True) and np.array_equal(a.rows(G - 1, 5), rows[G - 1:G + 4], equal_nan=True)
            if cap < 0:
                distinct = len(set(m for c in cs for side in c for m in side))
                assert a.device_bytes() == 16 * (len(cs) + 1) + 4 * sum(len(c[0]) + len(c[1]) for c in cs) + 4 * distinct + 16 * nv
    lm = q.series(gpu.SERIES_GENE)["log_mean"]
    np.testing.assert_allclose(sa["log_ratio"][:G], lm - np.roll(lm, -1), rtol=1e-12, atol=1e-12)
    ref = R.contrast_ref(full, cs, pidx, log=_dlog(gpu))
    assert np.array_equal(rows, ref["R"], equal_nan=True) and np.array_equal(sa["p_gt"], ref["p_gt"])
    q.close(); smp.close(); prob.close()


def test_the_memory_formula_and_the_argument_errors(gpu, slab_option):
    from mmseq_amd import Contrast, _lib
    from mmseq_amd._lib import MMGError
    lib = _lib.load()
    rng = np.random.default_rng(9)
    n, S = 12, 16
    tr = _traces(rng, n, S)
    cs = [([0, 1], [2]), ([3], [3, 4, 5]), ([6], [7])]
    with Contrast.from_traces(tr, cs, [0]) as h:
        assert h.device_bytes() == 16 * 4 + 4 * 9 + 8 * n * S
        good = h.summary()
    bad = [[], [([], [0])], [([0], [])], [([0, 1, 0], [2])], [([0], [2, 2])], [([0], [n])], [([n + 5], [0])]]
    for b in bad:
        with pytest.raises(MMGError) as e:
            Contrast.from_traces(tr, b, [0])
        assert e.value.code == 1 and str(e.value).split(": ", 1)[1], b
    with pytest.raises(MMGError) as e:
        Contrast.from_traces(tr, [([0], [1]), ([2], [])])
    assert e.value.code == 1 and "empty denominator of contrast 1" in str(e.value)
    with pytest.raises(MMGError) as e:
        Contrast.from_traces(tr, [([0], [1, 4, 1])])
    assert e.value.code == 1 and "member 1 twice in the denominator of contrast 0" in str(e.value)
    # null pointers: the description, the output handle, an array of the description
    hnd = C.c_void_p()
    d, keep = Contrast._desc(cs, [0])
    ptr = tr.ctypes.data_as(C.c_void_p)
    assert lib.mmg_contrast_of_traces(0, S, n, ptr, None, C.byref(hnd)) == 1 and b"NULL" in lib.mmg_last_error()
    assert lib.mmg_contrast_of_traces(0, S, n, None, C.byref(d), C.byref(hnd)) == 1
    assert lib.mmg_contrast_of_traces(0, S, n, ptr, C.byref(d), None) == 1
    d.den_member = None
    assert lib.mmg_contrast_of_traces(0, S, n, ptr, C.byref(d), C.byref(hnd)) == 1 and b"NULL" in lib.mmg_last_error()
    assert lib.mmg_contrast_get(None, None, None, None, None, None, None) == 1
    with Contrast.from_traces(tr, cs, [0]) as h:               # the device is as usable as before
        with pytest.raises(MMGError) as e:
            h.rows(2, 2)
        assert e.value.code == 1
        for k, v in h.summary().items():
            assert np.array_equal(v, good[k], equal_nan=True)
    # a summary that is not finished: MMG_ERR_STATE
    q = gpu.Problem.from_csr(np.array([0, 2], np.uint64), np.array([0, 1], np.uint32), np.ones(2))
    smp = gpu.Sampler(q, np.ones(2), gibbs_iter=4, trace_len=4)
    smp.run(4)
    smp.sync()
    staged = gpu.Summary(smp, staged=True)
    with pytest.raises(MMGError) as e:
        Contrast.from_sampler(smp, staged, [([0], [1])])
    assert e.value.code == 4
    staged.advance(4); staged.finish()
    with pytest.raises(MMGError) as e:
        Contrast.from_sampler(smp, staged, [([0], [2])])       # 2 transcripts, no simulated isoform
    assert e.value.code == 1
    with Contrast.from_sampler(smp, staged, [([0], [1]), ([1], [0, 1])]) as h:
        np.testing.assert_allclose(h.rows()[0], np.log(smp.trace(0)[0]) - np.log(smp.trace(0)[1]), rtol=1e-12, atol=1e-12)
    staged.close(); smp.close(); q.close()


def test_cli_writes_the_contrast_table_and_mmdiff_reads_it(gpu, tmp_path):
    """mmseq -contrasts: one row per contrast in file order under the stated columns; every other file and stdout are the bytes of a
    run without the flag; the tables of a 2-vs-2 generated experiment go through mmdiff -nonorm -de 2 2."""
    data = [dataset(seed=s, n_reads=1500) for s in (3, 4, 5, 6)]
    seen = [set(H.ingest(h)["sid_index"]) for h in data]
    common = sorted(set.intersection(*seen))
    assert "T0000005" in common and "T0000006" in common and len(common) >= 8 and all("T0000040" not in s for s in seen)
    others = [t for t in common if t not in ("T0000005", "T0000006")]
    lines = ["# a comment, then a blank line", "",
             "allele\tT0000005\tT0000006",
             "switch\t%s,%s\t%s,%s" % tuple(others[:4]),
             "share\tT0000005\tT0000006,T0000005",
             "with_unobserved\t%s\t%s,T0000040" % (others[4], others[5])]
    names = ["allele", "switch", "share", "with_unobserved"]
    tables = []
    for i, h in enumerate(data):
        d = tmp_path / ("s%d" % i)
        d.mkdir()
        (d / "in.hits").write_bytes(H.write_hits_text(h))
        (d / "c.txt").write_text("\n".join(lines) + "\n")
        r = run(["-gibbs_iter", "1024", "-seed", "5", "-contrasts", "c.txt", "in.hits", "out"], timeout=300, cwd=str(d))
        assert r.returncode == 0, r.stderr.decode()
        tables.append(str(d / "out.contrasts.mmseq"))
        if i == 0:
            flag = r
    plain_dir = tmp_path / "plain"
    plain_dir.mkdir()
    (plain_dir / "in.hits").write_bytes(H.write_hits_text(data[0]))
    plain = run(["-gibbs_iter", "1024", "-seed", "5", "in.hits", "out"], timeout=300, cwd=str(plain_dir))
    assert plain.returncode == 0
    listed = b"  out.contrasts.mmseq\n\n"
    assert flag.stdout.count(listed) == 1 and flag.stdout.replace(listed, b"") == plain.stdout
    with_names, plain_names = sorted(os.listdir(tmp_path / "s0")), sorted(os.listdir(plain_dir))
    assert sorted(set(with_names) - set(plain_names)) == ["c.txt", "out.contrasts.mmseq"]
    for name in plain_names:
        opener = gzip.open if name.endswith(".gz") else open
        assert opener(tmp_path / "s0" / name, "rb").read() == opener(plain_dir / name, "rb").read(), name

    text = open(tables[0]).read().split("\n")
    assert text[0].startswith("# ") and "log-ratio" in text[0].lower() and "-nonorm" in text[0] and text[-1] == ""
    assert text[1].split("\t") == ["feature_id", "log_mu", "sd", "mcse", "iact", "unique_hits", "p_gt", "n_num", "n_den", "observed",
                                   "percentiles5,25,50,75,95"]
    rows = [dict(zip(text[1].split("\t"), ln.split("\t"))) for ln in text[2:-1]]
    assert [r["feature_id"] for r in rows] == names
    assert [(r["n_num"], r["n_den"], r["observed"]) for r in rows] == [("1", "1", "1"), ("2", "2", "1"), ("1", "2", "1"), ("1", "2", "1")]
    for r in rows:
        pct = [float(v) for v in r["percentiles5,25,50,75,95"].split(",")]
        assert pct == sorted(pct) and pct[0] <= float(r["log_mu"]) <= pct[-1] and float(r["sd"]) > 0 and 0.0 <= float(r["p_gt"]) <= 1.0
        assert float(r["mcse"]) > 0 and float(r["iact"]) > 0 and int(r["unique_hits"]) >= 0
    assert float(rows[2]["log_mu"]) < 0 and float(rows[2]["p_gt"]) == 0.0 and max(float(v) for v in rows[2]["percentiles5,25,50,75,95"].split(",")) < 0

    r = subprocess.run([os.path.join(BIN_DIR, "mmdiff"), "-nonorm", "-burnin", "1024", "-iter", "1024", "-de", "2", "2"] + tables,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    out = [ln for ln in r.stdout.decode().split("\n") if ln and not ln.startswith("#")]
    assert out[0].startswith("feature_id\t") and [ln.split("\t")[0] for ln in out[1:]] == names
