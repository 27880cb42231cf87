"""mmg_isoform_* on the device (mmseq_amd.Isoforms, mmseq -isoforms) against tests/isoforms_ref.py fed the library's own logarithm:
every output with ==, at the wave, block and list-length edges, with ties, zeros and draws that are not valid, across slab cuts and
reruns, from a sampler's resident trace with simulated isoforms, the handle's memory formula and error codes, and the CLI's tables."""
import ctypes as C
import gc
import gzip
import os

import numpy as np
import pytest

from oracle import host_oracle as H
from test_cli import dataset, run
import isoforms_ref as R

pytestmark = pytest.mark.gpu

MEMBER_KEYS = ("n_top", "n_second", "n_above")
GROUP_KEYS = ("status", "major", "n_distinct", "mean_H", "ss_H", "mean_P", "ss_P", "q_H", "q_P")
ROW_KEYS = ("top", "second", "H", "P")


def _dlog(gpu):
    return lambda x: gpu.selftest_math(x, 0)["log"]        # mmg_math.h: dlog, evaluated on the device


def _all(h):
    out = {}
    out.update({k: v for k, v in h.members().items() if k in MEMBER_KEYS})
    out.update({k: v for k, v in h.groups().items() if k in GROUP_KEYS})
    out.update(h.rows())
    return out


def _same(got, want, groups=None, what=""):
    """every device output with ==; groups: (positions in got, positions in want) to compare, default all"""
    ptr_g, ptr_w = got["ptr"], want["ptr"]
    pairs = list(zip(*groups)) if groups is not None else [(g, g) for g in range(ptr_w.size - 1)]
    for a, b in pairs:
        for k in GROUP_KEYS + ROW_KEYS:
            assert np.array_equal(got[k][a], want[k][b], equal_nan=True), (what, k, a, b)
        for k in MEMBER_KEYS:
            assert np.array_equal(got[k][ptr_g[a]:ptr_g[a + 1]], want[k][ptr_w[b]:ptr_w[b + 1]]), (what, k, a, b)


def _run(tr, groups, thresholds, ranks):
    from mmseq_amd import Isoforms
    with Isoforms.from_traces(tr, groups, thresholds, ranks) as h:
        out = _all(h)
        out["ptr"] = h.ptr.astype(np.int64)
    return out


@pytest.fixture
def slab_option(gpu):
    from mmseq_amd import _lib
    lib = _lib.load()
    yield lambda v: lib.mmg_selftest_option(_lib.OPT_ISO_SLAB, v)
    lib.mmg_selftest_option(_lib.OPT_ISO_SLAB, -1)


def _edge_groups(rng, n, S):
    """groups of 1, 2, 63, 64, 65, 257 and (S <= 65) 5 000 members in an order unrelated to their sizes; the first and the last series;
    shuffled lists; members in two groups"""
    pick = lambda k: [int(m) for m in rng.choice(n, k, replace=False)]
    gs = [pick(257), [0], pick(63), [n - 1, 0], pick(64), [n - 1], pick(2), pick(65), [7, 0, n - 1, 11], [11, 7]]
    if S <= 65:
        gs.insert(3, pick(5000))
    return gs


@pytest.mark.parametrize("S", [1, 63, 64, 65, 1024])
def test_every_output_bit_for_bit_at_the_edges(gpu, S):
    from mmseq_amd import Isoforms
    rng = np.random.default_rng(180 + S)
    n = 5003
    tr = np.exp(rng.normal(0.0, 3.0, (n, S)))
    groups = _edge_groups(rng, n, S)
    th, ranks = [0.1, 0.5, 0.0], [0, S // 2, S - 1, S]
    ref = R.isoforms_ref(tr, groups, th, ranks, log=_dlog(gpu))
    with Isoforms.from_traces(tr, groups, th, ranks) as h:
        got = _all(h)
        got["ptr"] = h.ptr.astype(np.int64)
        some = h.rows(3, 4)
        for k in ROW_KEYS:
            assert np.array_equal(some[k], got[k][3:7]), k
        d = h.groups()
        assert h.device_bytes() == 8 * (len(groups) + 1) + 4 * sum(len(g) for g in groups) + 8 * n * S
    _same(got, ref)
    assert (got["status"] == 0).all()
    assert np.isnan(got["q_H"][:, 3]).all() and np.isnan(got["q_P"][:, 3]).all() and np.isfinite(got["q_H"][:, :3]).all()   # a rank = S
    np.testing.assert_allclose(got["H"], R.isoforms_ref(tr, groups)["H"], rtol=1e-12, atol=1e-12)                              # ... and np.log's
    for g, mem in enumerate(groups):
        sl = slice(got["ptr"][g], got["ptr"][g + 1])
        assert got["n_top"][sl].sum() == S and got["n_second"][sl].sum() == (S if len(mem) > 1 else 0)
        assert (got["n_above"][sl, 2] == S).all()                                        # theta = 0: every positive draw is above
    assert np.array_equal(d["p_top"], got["n_top"][got["ptr"][:-1] + got["major"]] / float(S))
    assert np.array_equal(d["eff_isoforms"], np.exp(got["mean_H"]))
    if S > 1:
        assert np.array_equal(d["sd_P"], np.sqrt(got["ss_P"] / float(S - 1)))


def _six_digits(x):
    return np.array([float("%.6g" % v) for v in x.ravel()]).reshape(x.shape)


def test_ties_zeros_and_draws_that_are_not_valid(gpu):
    rng = np.random.default_rng(77)
    n, S = 40, 130
    tr = _six_digits(rng.gamma(0.7, 2.0, (n, S)))                # what a text trace carries
    tr[3] = 0.0                                                  # a member identically 0
    tr[1, ::2] = tr[0, ::2] = np.maximum(tr[0, ::2], tr[2, ::2]) + 1.0          # exact ties for the top: 0 wins over 1
    tr[6, ::3] = tr[5, ::3] = np.minimum(tr[4, ::3], 1.0) * 0.5                 # exact ties for the second, below member 4
    tr[4, ::3] = tr[4, ::3] + 1.0
    good = [[0, 1, 2], [1, 0, 2], [4, 5, 6], [6, 5, 4], [3, 7], [3], [8, 3, 9, 10], list(range(11, 30))]
    # the draws that are not valid sit in series of their own groups only
    bad_tr = tr.copy()
    bad_tr[30, 5] = np.nan
    bad_tr[31, S - 1] = np.inf
    bad_tr[32, 64] = -1e-300
    bad_tr[33, 100] = bad_tr[34, 100] = 0.0                      # an all-zero sample
    bad = [[30, 12], [13, 31, 14], [32], [33, 34]]
    mixed = [good[0], bad[0], good[1], good[2], bad[1], bad[2], good[3], good[4], good[5], bad[3], good[6], good[7]]
    where_good = [0, 2, 3, 6, 7, 8, 10, 11]
    where_bad = [1, 4, 5, 9]
    th, ranks = [0.1, 0.5], [0, 64, 129]
    a = _run(bad_tr, mixed, th, ranks)
    b = _run(tr, good, th, ranks)
    _same(a, b, groups=(where_good, list(range(len(good)))), what="beside groups that are not valid")
    _same(a, R.isoforms_ref(bad_tr, mixed, th, ranks, log=_dlog(gpu)), what="reference")
    for g in where_bad:
        sl = slice(a["ptr"][g], a["ptr"][g + 1])
        assert a["status"][g] == 1 and a["n_distinct"][g] == 0
        assert not a["n_top"][sl].any() and not a["n_second"][sl].any() and not a["n_above"][sl].any()
        for k in ("mean_H", "ss_H", "mean_P", "ss_P", "q_H", "q_P", "H", "P"):
            assert np.isnan(a[k][g]).all(), (g, k)
        assert (a["top"][g] == R.NONE).all() and (a["second"][g] == R.NONE).all()
    assert np.array_equal(b["status"], [0, 0, 0, 0, 0, 1, 0, 0])  # (the zero member alone: T = 0)
    # the tie rule on the draws: the earlier position wins, whatever the member
    assert (b["top"][0][::2] == 0).all() and (b["second"][0][::2] == 1).all() and (b["top"][1][::2] == 0).all() and (b["second"][1][::2] == 1).all()
    assert (b["top"][2][::3] == 0).all() and (b["second"][2][::3] == 1).all() and (b["second"][3][::3] == 0).all() and (b["top"][3][::3] == 2).all()
    assert b["n_top"][b["ptr"][4]] == 0 and b["n_top"][b["ptr"][4] + 1] == S and (b["H"][4] == 0.0).all() and not np.signbit(b["H"][4]).any()


def test_slab_cuts_and_reruns_give_the_same_bits(gpu, slab_option):
    from mmseq_amd import Isoforms
    rng = np.random.default_rng(5)
    n, S = 60, 70
    tr = _six_digits(rng.gamma(0.5, 1.0, (n, S)))
    groups = [[int(m) for m in rng.choice(n, int(rng.integers(1, 9)), replace=False)] for _ in range(17)]
    th, ranks = [0.1, 0.5], [0, 35, 69, 70]
    with Isoforms.from_traces(tr, groups, th, ranks) as h:
        whole = _all(h)
        again = _all(h)                                          # a second get on the same handle
        for k in whole:
            assert np.array_equal(whole[k], again[k], equal_nan=True), k
    with Isoforms.from_traces(tr, groups, th, ranks) as h2:      # a second handle over the same input
        for k, v in _all(h2).items():
            assert np.array_equal(whole[k], v, equal_nan=True), k
    for cap in (1, 2, 7):
        assert slab_option(cap) == 0
        with Isoforms.from_traces(tr, groups, th, ranks) as h:
            for k, v in _all(h).items():
                assert np.array_equal(whole[k], v, equal_nan=True), (cap, k)
            for first, count in ((5, 6), (16, 1), (0, 17), (6, 2)):
                part = h.rows(first, count)
                for k in ROW_KEYS:
                    assert np.array_equal(part[k], whole[k][first:first + count], equal_nan=True), (cap, first, k)


def _host_gamma_trace(seed, vid, shape, scale, n):
    from mmseq_amd import _lib
    out = np.empty(n)
    _lib.check(_lib.load().mmg_host_gamma_trace(int(seed), int(vid), float(shape), float(scale), int(n), out.ctypes.data_as(C.c_void_p)))
    return out


def test_sampler_path_equals_host_traces_and_the_summary_proportions(gpu, orc, slab_option):
    """a small generated problem, transcripts renumbered on the device, 9 isoforms without hits, 64 iterations, genes of 3"""
    from mmseq_amd import Isoforms
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
    th, ranks = [0.1, 0.5], [0, 32, 63]
    G = len(genes)
    for cap in (-1, 2):
        slab_option(cap)
        with Isoforms.from_sampler(smp, q, genes, th, ranks) as a, Isoforms.from_traces(full, genes, th, ranks) as b:
            sa, sb = _all(a), _all(b)
            for k in sa:
                assert np.array_equal(sa[k], sb[k], equal_nan=True), (cap, k)
            part = a.rows(G - 4, 3)
            for k in ROW_KEYS:
                assert np.array_equal(part[k], sa[k][G - 4:G - 1], equal_nan=True), (cap, k)
            if cap < 0:
                assert a.device_bytes() == 8 * (G + 1) + 4 * (n + nv) + 4 * (n + nv) + 16 * nv      # every member is in one gene: one slab, n + nv distinct
                assert b.device_bytes() == 8 * (G + 1) + 4 * (n + nv) + 8 * (n + nv) * S
    assert (sa["status"] == 0).all()
    ref = R.isoforms_ref(full, genes, th, ranks, log=_dlog(gpu))
    ref_keys = dict(sa, ptr=ref["ptr"])
    _same(ref_keys, ref)
    # T and the division are the summary's: P is the largest of the gene's proportion rows
    prop = q.rows(gpu.SERIES_TRANSCRIPT)                        # (S, n): the transcripts' proportions of their genes
    checked = 0
    for g, mem in enumerate(genes):
        real = [m for m in mem if m < n]
        if len(real) == len(mem):
            assert np.array_equal(sa["P"][g], prop[:, mem].max(axis=1)), g
            checked += 1
        for s in range(S):
            m = mem[sa["top"][g][s]]
            if m < n:
                assert sa["P"][g][s] == prop[s, m], (g, s)
    assert checked >= G - nv and checked > 0
    q.close(); smp.close(); prob.close()


def _live(lib):
    from mmseq_amd import _lib
    c = (C.c_int64 * 3)()
    _lib.check(lib.mmg_selftest_live(c))
    return list(c)


def test_the_argument_errors_leave_the_library_usable(gpu):
    from mmseq_amd import Isoforms, _lib
    from mmseq_amd._lib import MMGError
    lib = _lib.load()
    rng = np.random.default_rng(9)
    n, S = 12, 16
    tr = rng.gamma(1.0, 1.0, (n, S))
    groups = [[0, 1, 2], [3], [4, 5]]
    good = _run(tr, groups, [0.1], [0, 15])
    gc.collect()
    base = _live(lib)
    cases = [(dict(groups=[]), "n_groups"), (dict(groups=[[0], [], [1]]), "empty group 1"),
             (dict(groups=[[0], [4, 5, 4]]), "member 4 (position 2 of group 1) twice"),
             (dict(groups=[[0, n]]), "member %d (position 1 of group 0) out of range" % n),
             (dict(thresholds=[0.1, 1.0]), "threshold 1"), (dict(thresholds=[-0.1]), "threshold 0"), (dict(thresholds=[np.nan]), "threshold 0"),
             (dict(thresholds=[np.inf]), "threshold 0"), (dict(thresholds=[0.1] * 9), "n_thresholds = 9"), (dict(ranks=[0] * 65), "n_ranks = 65"),
             (dict(tr=np.ones((2, 4097)), groups=[[0, 1]]), "S = 4097")]
    for kw, msg in cases:
        args = dict(tr=tr, groups=groups, thresholds=[0.1], ranks=[0])
        args.update(kw)
        with pytest.raises(MMGError) as e:
            Isoforms.from_traces(args["tr"], args["groups"], args["thresholds"], args["ranks"])
        assert e.value.code == 1 and msg in str(e.value), (kw, str(e.value))
    # null pointers: the description, the traces, the output handle, an array of the description
    hnd = C.c_void_p()
    d, keep = Isoforms._desc(groups, [0.1], [0])
    ptr = tr.ctypes.data_as(C.c_void_p)
    assert lib.mmg_isoform_of_traces(0, S, n, ptr, None, C.byref(hnd)) == 1 and b"NULL" in lib.mmg_last_error()
    assert lib.mmg_isoform_of_traces(0, S, n, None, C.byref(d), C.byref(hnd)) == 1
    assert lib.mmg_isoform_of_traces(0, S, n, ptr, C.byref(d), None) == 1
    assert lib.mmg_isoform_of_traces(0, 0, n, ptr, C.byref(d), C.byref(hnd)) == 1 and b"S = 0" in lib.mmg_last_error()
    assert lib.mmg_isoform_create(None, None, C.byref(d), C.byref(hnd)) == 1
    for field in ("member", "ptr", "threshold", "rank"):
        d, keep = Isoforms._desc(groups, [0.1], [0])
        setattr(d, field, None)
        assert lib.mmg_isoform_of_traces(0, S, n, ptr, C.byref(d), C.byref(hnd)) == 1 and b"NULL" in lib.mmg_last_error(), field
    assert lib.mmg_isoform_get_members(None, None, None, None) == 1 and lib.mmg_isoform_device_bytes(None, None) == 1
    assert lib.mmg_isoform_get_rows(None, 0, 0, None, None, None, None) == 1
    assert _live(lib) == base
    with Isoforms.from_traces(tr, groups, [0.1], [0, 15]) as h:      # the device is as usable as before
        with pytest.raises(MMGError) as e:
            h.rows(2, 2)
        assert e.value.code == 1
        got = _all(h)
        for k in got:
            assert np.array_equal(got[k], good[k], equal_nan=True), k
        assert lib.mmg_isoform_get_groups(h._h, *([None] * 9)) == 0 and lib.mmg_isoform_get_rows(h._h, 0, 3, None, None, None, None) == 0
    # a summary that is not finished: MMG_ERR_STATE
    q = gpu.Problem.from_csr(np.array([0, 2], np.uint64), np.array([0, 1], np.uint32), np.ones(2))
    smp = gpu.Sampler(q, np.ones(2), gibbs_iter=4, trace_len=4)
    smp.run(4)
    smp.sync()
    staged = gpu.Summary(smp, staged=True)
    with pytest.raises(MMGError) as e:
        Isoforms.from_sampler(smp, staged, [[0, 1]])
    assert e.value.code == 4
    staged.advance(4); staged.finish()
    with pytest.raises(MMGError) as e:
        Isoforms.from_sampler(smp, staged, [[0, 2]])               # 2 transcripts, no simulated isoform
    assert e.value.code == 1 and "out of range" in str(e.value)
    with Isoforms.from_sampler(smp, staged, [[0, 1], [1]]) as h:
        t = smp.trace(0)
        assert np.array_equal(h.rows()["P"][0], np.maximum(t[0], t[1]) / (t[0] + t[1]))
    staged.close(); smp.close(); q.close()


def test_a_failed_acquisition_leaves_nothing_behind(gpu):
    from mmseq_amd import Isoforms, _lib
    from mmseq_amd._lib import MMGError
    lib = _lib.load()
    rng = np.random.default_rng(10)
    tr = rng.gamma(1.0, 1.0, (20, 70))
    groups = [[int(m) for m in rng.choice(20, 3, replace=False)] for _ in range(9)]
    want = _run(tr, groups, [0.1], [0, 5])
    gc.collect()
    base = _live(lib)
    v = 0
    try:
        with gpu.options(iso_slab=4):
            while True:
                _lib.check(lib.mmg_selftest_option(_lib.OPT_FAIL_ALLOC, v))
                try:
                    h = Isoforms.from_traces(tr, groups, [0.1], [0, 5])
                except MMGError as e:
                    assert e.code == 3 and str(e)
                    assert _live(lib) == base, v
                    v += 1
                    continue
                break
    finally:
        lib.mmg_selftest_option(_lib.OPT_FAIL_ALLOC, -1)
    assert v == 11                                             # the traces, the stream, the two lists and the seven buffers of creation
    live = _live(lib)
    assert live[0] == base[0] + 3 and live[1] == base[1] + 1   # the handle keeps the traces, the lists and its stream
    got = _all(h)
    h.close()
    assert _live(lib) == base
    for k in got:
        assert np.array_equal(got[k], want[k], equal_nan=True), k


def _table(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == ""
    comments = [ln for ln in lines if ln.startswith("#")]
    body = [ln for ln in lines[:-1] if not ln.startswith("#")]
    cols = body[0].split("\t")
    return comments, cols, [dict(zip(cols, ln.split("\t"))) for ln in body[1:]]


def test_cli_writes_the_transcript_and_the_gene_table(gpu, tmp_path):
    """mmseq -isoforms at 1 024 iterations: the two new files under the stated columns, in the row order of .mmseq and .gene.mmseq;
    every other file and stdout are the bytes of a run without the flag"""
    data = dataset(seed=3, n_reads=1500)
    runs = {}
    for name, extra in (("plain", []), ("iso", ["-isoforms"])):
        d = tmp_path / name
        d.mkdir()
        (d / "in.hits").write_bytes(H.write_hits_text(data))
        runs[name] = run(["-gibbs_iter", "1024", "-seed", "5"] + extra + ["in.hits", "out"], timeout=300, cwd=str(d))
        assert runs[name].returncode == 0, runs[name].stderr.decode()
    listed = b"  out.isoforms\n  out.gene.isoforms\n\n"
    assert runs["iso"].stdout.count(listed) == 1 and runs["iso"].stdout.replace(listed, b"") == runs["plain"].stdout
    with_names, plain_names = sorted(os.listdir(tmp_path / "iso")), sorted(os.listdir(tmp_path / "plain"))
    assert sorted(set(with_names) - set(plain_names)) == ["out.gene.isoforms", "out.isoforms"]
    for name in plain_names:
        opener = gzip.open if name.endswith(".gz") else open
        assert opener(tmp_path / "iso" / name, "rb").read() == opener(tmp_path / "plain" / name, "rb").read(), name

    ct, cols_t, rows_t = _table(tmp_path / "iso" / "out.isoforms")
    cg, cols_g, rows_g = _table(tmp_path / "iso" / "out.gene.isoforms")
    assert cols_t == ["feature_id", "gene_id", "n_isoforms", "rank_in_gene", "p_major", "p_second", "p_above_0.1", "p_above_0.5"]
    assert cols_g == ["gene_id", "n_isoforms", "major_id", "p_major", "n_distinct", "entropy", "entropy_sd", "eff_isoforms", "max_prop", "max_prop_sd",
                      "percentiles_entropy5,25,50,75,95", "percentiles_max_prop5,25,50,75,95", "status"]
    for c in (ct, cg):
        assert len(c) == 1 and "S = 1024" in c[0] and "chain 0" in c[0] and c[0].endswith("thresholds: 0.1,0.5")
    _, _, mm = _table(tmp_path / "iso" / "out.mmseq")
    _, _, gm = _table(tmp_path / "iso" / "out.gene.mmseq")
    assert [r["feature_id"] for r in rows_t] == [r["feature_id"] for r in mm]
    assert [r["gene_id"] for r in rows_g] == [r["feature_id"] for r in gm]
    by_gene = {}
    for r in rows_t:
        by_gene.setdefault(r["gene_id"], []).append(r)
    singles = 0
    for g in rows_g:
        mine = by_gene[g["gene_id"]]
        k = int(g["n_isoforms"])
        assert g["status"] == "0" and k == len(mine) and all(int(r["n_isoforms"]) == k for r in mine)
        assert abs(sum(float(r["p_major"]) for r in mine) - 1.0) < 1e-5 * k                    # (six digits each)
        assert sorted(int(r["rank_in_gene"]) for r in mine) == list(range(1, k + 1))
        top = [r for r in mine if r["rank_in_gene"] == "1"][0]
        assert top["feature_id"] == g["major_id"] and top["p_major"] == g["p_major"] and float(top["p_major"]) == max(float(r["p_major"]) for r in mine)
        assert 1 <= int(g["n_distinct"]) <= k
        assert -1e-12 <= float(g["entropy"]) <= np.log(k) * (1 + 1e-5) + 1e-12 and float(g["max_prop"]) >= 1.0 / k * (1 - 1e-5)
        assert abs(float(g["eff_isoforms"]) - np.exp(float(g["entropy"]))) <= 1e-4 * k
        for col in ("percentiles_entropy5,25,50,75,95", "percentiles_max_prop5,25,50,75,95"):
            pct = [float(v) for v in g[col].split(",")]
            assert pct == sorted(pct) and len(pct) == 5
        for r in mine:
            assert float(r["p_above_0.5"]) <= float(r["p_above_0.1"]) and 0.0 <= float(r["p_second"]) <= 1.0
            assert float(r["p_above_0.5"]) <= float(r["p_major"]) + 1e-9                       # above half of the gene: the top
        if k == 1:
            singles += 1
            assert g["p_major"] == "1" and float(g["entropy"]) == 0.0 and g["max_prop"] == "1" and g["n_distinct"] == "1" and mine[0]["p_second"] == "0"
    assert singles >= 3
    # the gene whose four isoforms never get a hit is there with its simulated draws, and so is every isoform without hits
    none = [r for r in rows_t if r["feature_id"] in ("T0000040", "T0000041", "T0000042", "T0000043")]
    assert len(none) == 4 and len(set(r["gene_id"] for r in none)) == 1 and all(r["n_isoforms"] == "4" for r in none)
    unobserved = [r["feature_id"] for r in mm if r["observed"] == "0"]
    assert len(unobserved) >= 4 and all(any(t["feature_id"] == u and t["gene_id"] != "NA" for t in rows_t) for u in unobserved)
