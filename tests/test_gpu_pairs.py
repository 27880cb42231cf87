"""mmg_pairs_* on the device (mmseq_amd.Pairs, mmseq -pairs) against tests/pairs_ref.py: every column bit for bit with the library's
own logarithm, slab edges, the sampler's trace taken on the device, the statistical reading of the columns on the device's chain,
the memory formula, the error codes and the failed acquisitions, and the CLI's table end to end."""
import ctypes as C
import gc
import gzip
import os

import numpy as np
import pytest

from oracle import host_oracle as H
from test_cli import _table, _trace_file, dataset, run
from test_pairs_cli import restate
import pairs_ref as R

pytestmark = pytest.mark.gpu


def _dlog(gpu):
    return lambda x: gpu.selftest_math(x, 0)["log"]        # mmg_math.h: dlog, evaluated on the device


def _same_bits(got, ref, what=None):
    for k in R.DEVICE_COLUMNS:
        assert np.array_equal(got[k], ref[k], equal_nan=True), (what, k, np.flatnonzero(~((got[k] == ref[k]) | (np.isnan(got[k]) & np.isnan(ref[k]))))[:5])


def _edge_case(S, seed):
    """40 series; 30 .. 37 hold a 0, a subnormal, 1e-300, 1e300, 1e308, inf, NaN and 1.7e308 in one sample (S = 1: their only one);
    series 0 against every other (a hub), (a, b) with (b, a), one pair twice, 1e300 + 1e308 (finite) and 1e308 + 1.7e308 (overflow)"""
    rng = np.random.default_rng(seed)
    n = 40
    tr = np.exp(rng.normal(-8.0, 3.0, n)[:, None] + rng.uniform(1e-3, 3.0, n)[:, None] * rng.normal(0.0, 1.0, (n, S)))
    at = (S - 1) // 2
    for m, v in zip(range(30, 38), (0.0, 5e-324, 1e-300, 1e300, 1e308, np.inf, np.nan, 1.7e308)):
        tr[m, at] = v
    pairs = [(0, m) for m in range(1, n)] + [(5, 9), (9, 5), (12, 3), (12, 3), (33, 34), (34, 37), (37, 34), (35, 36), (30, 31), (39, 0)]
    return tr, pairs


@pytest.mark.parametrize("S", [1, 2, 63, 64, 65, 1024, 4096])
def test_every_column_is_the_references_bits_at_the_edges(gpu, S):
    """4096: beyond 1024 samples the logarithms of the sums do not stay in registers between the passes"""
    from mmseq_amd import Pairs
    tr, pairs = _edge_case(S, 50 + S)
    with Pairs.from_traces(tr, pairs) as h:
        got = h.summary()
    ref = R.summary_ref(tr, pairs, log=_dlog(gpu))
    _same_bits(got, ref, S)
    for k in ("cor", "sd_a", "sd_b", "sd_sum", "p_gt"):       # IEEE sqrt and division on both sides
        assert np.array_equal(got[k], ref[k], equal_nan=True), k
    i, j = pairs.index((5, 9)), pairs.index((9, 5))
    assert got["mean_a"][i] == got["mean_b"][j] and got["saa"][i] == got["sbb"][j] and got["sab"][i] == got["sab"][j] and got["sss"][i] == got["sss"][j]
    hub = np.arange(39)
    assert (got["mean_a"][hub] == got["mean_a"][0]).all() and (got["saa"][hub] == got["saa"][0]).all()
    if S > 1:
        q = pairs.index((34, 37))
        assert got["mean_sum"][q] == np.inf and np.isnan(got["sss"][q]) and np.isfinite([got["saa"][q], got["sbb"][q], got["sab"][q]]).all()
        assert np.isfinite(got["sss"][pairs.index((33, 34))])


def test_slab_edges_and_reruns_give_the_same_bits(gpu):
    from mmseq_amd import Pairs
    tr, pairs = _edge_case(65, 7)
    with Pairs.from_traces(tr, pairs) as h:
        whole = h.summary()
        again = h.summary()                                    # a second _get on the same handle
    with Pairs.from_traces(tr, pairs) as h2:                   # a second handle over the same input
        rerun = h2.summary()
    for k in whole:
        assert np.array_equal(whole[k], again[k], equal_nan=True) and np.array_equal(whole[k], rerun[k], equal_nan=True), k
    for cap in (1, 3):
        with gpu.options(pairs_slab=cap):
            with Pairs.from_traces(tr, pairs) as h:
                got = h.summary()
                small = h.device_bytes()
        for k in whole:
            assert np.array_equal(whole[k], got[k], equal_nan=True), (cap, k)
        # the largest slab: cap pairs and, in this list, as many distinct members as cap pairs can have (2 cap; 1 + cap in the hub)
        assert small == (4 + 8 * 65 + 16) * (2 * cap) + 68 * cap + 8 * 40 * 65


def test_sampler_path_equals_host_traces_and_the_reference(gpu, orc):
    """a small generated problem, transcripts renumbered on the device, two chains, 64 iterations: the device's gather of a chain's
    trace against mmg_pairs_of_traces fed mmg_sampler_get_trace; and mean_a - mean_sum against the contrast a / (a, b)"""
    from mmseq_amd import Contrast, Pairs
    S = 64
    p, _ = orc.synth_problem(R=4000, T=150, avg_hits=4, seed=11, sort=False)
    n = p.n
    rng = np.random.default_rng(2)
    txo = (rng.permutation(n).astype(np.uint64) // np.uint64(4)) << np.uint64(32)
    prob = gpu.Problem.from_csr(p.row_ptr, p.col_idx, p.l, tx_order=txo)
    mu0, _ = prob.start_values()
    smp = gpu.Sampler(prob, mu0, seed=3, n_chains=2, gibbs_iter=S, trace_len=S)
    smp.run(S)
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, n, (300, 2)) if a != b] + [(0, n - 1), (n - 1, 0)] + [(7, m) for m in range(8, 40)]
    by_chain = []
    for c in (0, 1):
        tr = smp.trace(c)
        for cap in (-1, 5):
            with gpu.options(pairs_slab=cap):
                with Pairs.from_sampler(smp, pairs, chain=c) as a, Pairs.from_traces(tr, pairs) as b:
                    sa, sb = a.summary(), b.summary()
                    for k in sa:
                        assert np.array_equal(sa[k], sb[k], equal_nan=True), (c, cap, k)
                    if cap < 0:
                        distinct = len(set(m for pr in pairs for m in pr))
                        assert a.device_bytes() == (4 + 16 * S + 16) * distinct + 68 * len(pairs)
                        assert b.device_bytes() == (4 + 8 * S + 16) * distinct + 68 * len(pairs) + 8 * n * S
        _same_bits(sa, R.pairs_ref(tr, pairs, log=_dlog(gpu)), c)
        by_chain.append(sa)
    assert not np.array_equal(by_chain[0]["sab"], by_chain[1]["sab"])
    q = gpu.Summary(smp, chain=0)
    three = pairs[:3]
    with Contrast.from_sampler(smp, q, [([a], [a, b]) for a, b in three]) as h:
        share = h.summary()
    np.testing.assert_allclose(by_chain[0]["mean_a"][:3] - by_chain[0]["mean_sum"][:3], share["log_ratio"], rtol=0, atol=1e-9)
    q.close(); smp.close(); prob.close()


def test_columns_read_as_stated_on_the_devices_chain(gpu):
    from mmseq_amd import Pairs
    rp, ci, k, l = R.stat_problem()
    prob = gpu.Problem.from_csr(rp, ci, l, k=k, keep_rows=True)
    mu0, _ = prob.start_values()
    smp = gpu.Sampler(prob, mu0, seed=4321, gibbs_iter=16384, trace_len=1024)
    smp.run(16384)
    with Pairs.from_sampler(smp, R.STAT_PAIRS) as h:
        s = h.summary()
    print({k: s[k] for k in ("cor", "sd_a", "sd_b", "sd_sum", "p_gt")})
    R.stat_rule(s)
    smp.close(); prob.close()


def _live(lib):
    from mmseq_amd import _lib
    c = (C.c_int64 * 3)()
    _lib.check(lib.mmg_selftest_live(c))
    return list(c)


def test_the_memory_formula_and_the_errors(gpu):
    from mmseq_amd import Pairs, _lib
    from mmseq_amd._lib import MMGError
    lib = _lib.load()
    rng = np.random.default_rng(9)
    n, S = 12, 16
    tr = np.exp(rng.normal(0.0, 1.0, (n, S)))
    pairs = [(0, 1), (1, 2), (5, 0), (0, 1)]
    with Pairs.from_traces(tr, pairs) as h:
        # one slab: 4 distinct members, 4 pairs; list + centred rows + means and squares, slots + results, the uploaded traces
        assert h.device_bytes() == 4 * 4 + 8 * S * 4 + 16 * 4 + 8 * 4 + 60 * 4 + 8 * n * S
        good = h.summary()
    for bad, text in (([], "n_pairs must be at least 1"), ([(0, 1), (3, 3)], "pair 1: a == b (member 3)"), ([(0, 1), (2, 3), (4, n)], "pair 2: member 12 out of range"),
                      ([(n + 7, 0)], "pair 0: member 19 out of range")):
        with pytest.raises(MMGError) as e:
            Pairs.from_traces(tr, bad)
        assert e.value.code == 1 and text in str(e.value), bad
    hnd = C.c_void_p()
    a, b = np.array([0, 1], np.uint32), np.array([1, 2], np.uint32)
    pa, pb, pt = a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p), tr.ctypes.data_as(C.c_void_p)
    assert lib.mmg_pairs_of_traces(0, S, n, None, 2, pa, pb, C.byref(hnd)) == 1 and b"NULL" in lib.mmg_last_error()
    assert lib.mmg_pairs_of_traces(0, S, n, pt, 2, None, pb, C.byref(hnd)) == 1 and b"NULL" in lib.mmg_last_error()
    assert lib.mmg_pairs_of_traces(0, S, n, pt, 2, pa, None, C.byref(hnd)) == 1 and b"NULL" in lib.mmg_last_error()
    assert lib.mmg_pairs_of_traces(0, S, n, pt, 2, pa, pb, None) == 1 and b"NULL" in lib.mmg_last_error()
    assert lib.mmg_pairs_of_traces(0, 0, n, pt, 2, pa, pb, C.byref(hnd)) == 1
    assert lib.mmg_pairs_get(None, *[None] * 8) == 1 and lib.mmg_pairs_device_bytes(None, None) == 1
    # the sampler's side: a chain out of range, the pair checks, a trace that is not finished, no trace at all
    q = gpu.Problem.from_csr(np.array([0, 2], np.uint64), np.array([0, 1], np.uint32), np.ones(2))
    smp = gpu.Sampler(q, np.ones(2), gibbs_iter=8, trace_len=4)
    smp.run(4)
    smp.sync()
    for chain in (-1, 1):
        with pytest.raises(MMGError) as e:
            Pairs.from_sampler(smp, [(0, 1)], chain=chain)
        assert e.value.code == 1 and "chain index out of range" in str(e.value)
    with pytest.raises(MMGError) as e:
        Pairs.from_sampler(smp, [(0, 1), (0, 2)])
    assert e.value.code == 1 and "pair 1: member 2 out of range" in str(e.value)
    assert lib.mmg_pairs_create(smp._h, 0, 1, None, pb, C.byref(hnd)) == 1 and lib.mmg_pairs_create(None, 0, 1, pa, pb, C.byref(hnd)) == 1
    with pytest.raises(MMGError) as e:
        Pairs.from_sampler(smp, [(0, 1)])                      # 2 of 4 samples kept
    assert e.value.code == 4
    smp.run(4)
    with Pairs.from_sampler(smp, [(0, 1), (1, 0)]) as h:
        s = h.summary()
        t = smp.trace(0)
        np.testing.assert_allclose(s["mean_a"], np.log(t).mean(axis=1), rtol=1e-12, atol=1e-12)
        assert s["n_gt"][0] == (t[0] > t[1]).sum() and s["n_gt"].sum() == 4
    smp.close()
    bare = gpu.Sampler(q, np.ones(2), gibbs_iter=4, trace_len=4, keep_trace=False)
    bare.run(4)
    with pytest.raises(MMGError) as e:
        Pairs.from_sampler(bare, [(0, 1)])
    assert e.value.code == 4
    bare.close(); q.close()
    with Pairs.from_traces(tr, pairs) as h:                    # the device is as usable as before
        for k, v in h.summary().items():
            assert np.array_equal(v, good[k], equal_nan=True)


def test_failed_acquisitions_give_back_everything(gpu, orc):
    from mmseq_amd import Pairs, _lib
    from mmseq_amd._lib import MMGError
    lib = _lib.load()
    tr, pairs = _edge_case(65, 11)
    p, _ = orc.synth_problem(R=2000, T=60, avg_hits=3, seed=5, sort=False)
    prob = gpu.Problem.from_csr(p.row_ptr, p.col_idx, p.l)
    mu0, _ = prob.start_values()
    smp = gpu.Sampler(prob, mu0, seed=1, gibbs_iter=64, trace_len=64)
    smp.run(64)
    smp.sync()
    makers = {"from_traces": lambda: Pairs.from_traces(tr, pairs), "from_sampler": lambda: Pairs.from_sampler(smp, pairs)}
    with gpu.options(pairs_slab=16):                           # several slabs: the scratch is acquired once, whatever their number
        for name, make in makers.items():
            first = make()
            want = first.summary()
            first.close()
            gc.collect()                                       # handles of earlier tests that only a collection frees must not go mid-sweep
            base = _live(lib)
            v = 0
            try:
                while True:
                    _lib.check(lib.mmg_selftest_option(_lib.OPT_FAIL_ALLOC, v))
                    try:
                        h = make()
                    except MMGError as e:
                        assert e.code == 3 and str(e)
                        assert _live(lib) == base, (name, v)
                        v += 1
                        continue
                    break
            finally:
                lib.mmg_selftest_option(_lib.OPT_FAIL_ALLOC, -1)
            assert v >= 8, (name, v)                           # the stream and the seven buffers of the pass
            assert _live(lib) == base                          # nothing is held after create
            got = h.summary()
            for k in want:
                assert np.array_equal(got[k], want[k], equal_nan=True), (name, k)
            h.close()
            assert _live(lib) == base
    smp.close(); prob.close()


# ------------------------------------------------------------------------------------------ the CLI
def _pairs_file(path):
    lines = open(path).read().split("\n")
    assert lines[-1] == "" and lines[0].startswith("# ")
    hdr = lines[1].split("\t")
    assert hdr == ["feature_a", "feature_b", "shared_hits", "shared_sets", "cor", "sd_a", "sd_b", "sd_sum", "log_mu_sum", "p_a_gt_b"]
    return lines[0], [dict(zip(hdr, ln.split("\t"))) for ln in lines[2:-1]]


def _printed(x, y, digits=6):
    """two numbers printed with `digits` significant digits agree up to a unit of the last one"""
    return abs(x - y) <= 10.0 ** (np.floor(np.log10(max(abs(x), abs(y), 1e-300))) - (digits - 1)) * 1.0000001


def test_cli_writes_the_pairs_table(gpu, tmp_path):
    """mmseq -pairs: one row per pair of transcripts that share a hit set, in header order; every other file and stdout are the
    bytes of a run without the flag; the columns against the hit sets, the .mmseq table, the trace file and a -contrasts table."""
    data = dataset(n_reads=1500)
    g = H.ingest(data)
    hidx = {name: i for i, name in enumerate(data.names)}
    label = [hidx[name] for name in g["index_sid"]]
    ref, ref_skipped = restate(g["rows"], g["k"], 16, label)
    want_pairs = sorted(ref)
    assert len(want_pairs) == 160 and ref_skipped == [0, 0]
    three = [want_pairs[0], want_pairs[50], want_pairs[159]]
    lines = ["gt%d\t%s\t%s" % (i, data.names[a], data.names[b]) for i, (a, b) in enumerate(three)]
    lines += ["share%d\t%s\t%s,%s" % (i, data.names[a], data.names[a], data.names[b]) for i, (a, b) in enumerate(three)]
    dirs = {}
    for name, extra in (("plain", []), ("pairs", ["-pairs"]), ("both", ["-pairs", "-contrasts", "c.txt"]), ("max3", ["-pairs", "-pairs_maxset", "3"])):
        d = tmp_path / name
        d.mkdir()
        (d / "in.hits").write_bytes(H.write_hits_text(data))
        (d / "c.txt").write_text("\n".join(lines) + "\n")
        r = run(["-gibbs_iter", "1024", "-seed", "5"] + extra + ["in.hits", "out"], timeout=300, cwd=str(d))
        assert r.returncode == 0, r.stderr.decode()
        dirs[name] = (d, r)
    (plain_dir, plain), (d, flag) = dirs["plain"], dirs["pairs"]
    listed = b"  out.pairs\n\n"
    assert flag.stdout.count(listed) == 1 and flag.stdout.replace(listed, b"") == plain.stdout
    with_names, plain_names = sorted(os.listdir(d)), sorted(os.listdir(plain_dir))
    assert sorted(set(with_names) - set(plain_names)) == ["out.pairs"]
    for name in plain_names:
        opener = gzip.open if name.endswith(".gz") else open
        assert opener(d / name, "rb").read() == opener(plain_dir / name, "rb").read(), name

    top, rows = _pairs_file(d / "out.pairs")
    assert top == "# 160 pairs of transcripts that share a hit set of at most 16 transcripts (-pairs_maxset); 0 larger sets skipped with 0 hits"
    assert [(hidx[r["feature_a"]], hidx[r["feature_b"]]) for r in rows] == want_pairs
    assert [[int(r["shared_hits"]), int(r["shared_sets"])] for r in rows] == [ref[p] for p in want_pairs]
    _, _, table = _table(d / "out.mmseq")
    sd_of = {r["feature_id"]: float(r["sd"]) for r in table}
    names, samples = _trace_file(d / "out.trace_gibbs.gz")
    col = {name: i for i, name in enumerate(names)}
    tr = np.array([[float(v) for v in s] for s in samples]).T             # (observed transcripts, 1024), six significant digits each
    S = tr.shape[1]
    assert S == 1024
    text = R.summary_ref(tr, [(col[r["feature_a"]], col[r["feature_b"]]) for r in rows])
    # A value printed with six significant digits is off by at most 5e-6 of itself, its logarithm by delta = 5.01e-6.  The centred
    # series du of S samples then moves by a vector e with |e| <= delta sqrt(S) (centring is a projection), while |du| = sd_a sqrt(S - 1);
    # the unit vector du / |du| moves by at most 2 |e| / |du| = 2 r_a with r_a = delta sqrt(S / (S - 1)) / sd_a, and cor, the product
    # of two unit vectors, by at most 2 r_a + 2 r_b + 4 r_a r_b <= 4 r + 4 r^2 with r taken at the pair's smaller sd (itself lowered
    # by its own error delta sqrt(S / (S - 1))).  On top: the table's own six digits of cor, half a unit of |cor| <= 1: 5e-6.
    delta, root = 5.01e-6, np.sqrt(S / (S - 1.0))
    for i, r in enumerate(rows):
        for side in ("a", "b"):
            assert _printed(float(r["sd_" + side]), sd_of[r["feature_" + side]]), (i, side, r["sd_" + side], sd_of[r["feature_" + side]])
        rr = delta * root / (min(text["sd_a"][i], text["sd_b"][i]) - delta * root)
        bound = 4 * rr + 4 * rr * rr + 5e-6
        print(i, r["cor"], text["cor"][i], bound)
        assert abs(float(r["cor"]) - text["cor"][i]) <= bound, (i, r["cor"], text["cor"][i], bound)

    # with -contrasts in the same run: the same .pairs, p_gt as printed, and the share line a / (a, b)
    d2 = dirs["both"][0]
    assert open(d2 / "out.pairs").read() == open(d / "out.pairs").read()
    ctext = open(d2 / "out.contrasts.mmseq").read().split("\n")
    crow = {ln.split("\t")[0]: dict(zip(ctext[1].split("\t"), ln.split("\t"))) for ln in ctext[2:-1]}
    log_mu = {r["feature_id"]: float(r["log_mu"]) for r in table}
    by_pair = {(hidx[r["feature_a"]], hidx[r["feature_b"]]): r for r in rows}
    for i, pr in enumerate(three):
        r = by_pair[pr]
        assert r["p_a_gt_b"] == crow["gt%d" % i]["p_gt"]
        # mean_a - mean_sum is the share line's log_mu.  The three numbers reach this test through three tables of six significant
        # digits, so the comparison is held to half a unit of the sixth digit of each (the handles' own doubles are compared to
        # 1e-9 in test_sampler_path_equals_host_traces_and_the_reference)
        mean_a, mean_sum, share = log_mu[r["feature_a"]], float(r["log_mu_sum"]), float(crow["share%d" % i]["log_mu"])
        half = lambda x: 0.5 * 10.0 ** (np.floor(np.log10(abs(x))) - 5) if x else 0.0
        assert abs((mean_a - mean_sum) - share) <= (half(mean_a) + half(mean_sum) + half(share)) * 1.0000001 + 1e-9, (i, mean_a, mean_sum, share)

    top3, rows3 = _pairs_file(dirs["max3"][0] / "out.pairs")
    ref3, skipped3 = restate(g["rows"], g["k"], 3, label)
    assert len(rows3) == 136 and skipped3[0] == 93
    assert top3 == "# 136 pairs of transcripts that share a hit set of at most 3 transcripts (-pairs_maxset); 93 larger sets skipped with %d hits" % skipped3[1]
    assert [(hidx[r["feature_a"]], hidx[r["feature_b"]]) for r in rows3] == sorted(ref3)
    kept = {(r["feature_a"], r["feature_b"]): r for r in rows}
    for r in rows3:                                                            # the device columns do not depend on the pair list
        assert all(kept[(r["feature_a"], r["feature_b"])][k] == r[k] for k in ("cor", "sd_a", "sd_b", "sd_sum", "log_mu_sum", "p_a_gt_b"))
