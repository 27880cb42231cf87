"""mmg_fold_* on the device (mmseq_amd.Fold, the mmfold CLI) against tests/fold_ref.py: every output compared with ==, over the sizes
at which the kernel pads, sorts and searches differently, slab edges, ties, constant sides, wide magnitudes, invalid draws, the
samplers' resident traces, the error codes, the memory formula and the CLI's table end to end."""
import ctypes as C
import gc
import subprocess

import numpy as np
import pytest

import fold_ref as R
from test_mmfold_cli import MMFOLD, TRACELEN, INFIX, write_table, write_trace

pytestmark = pytest.mark.gpu

KEYS = R.DEVICE_COLUMNS + ("lfc", "sd", "p_gt")


def _draws(rng, F, S, sig=None):
    x = np.exp(rng.normal(-3.0, 2.0, F)[:, None] + rng.uniform(0.01, 1.5, F)[:, None] * rng.normal(0.0, 1.0, (F, S)))
    if sig is None:
        return x
    return np.array([float("%.*g" % (sig, v)) for v in x.ravel()]).reshape(x.shape)


def _same(got, ref, what=None):
    for k in KEYS:
        g, r = np.asarray(got[k]), np.asarray(ref[k])
        assert g.shape == r.shape and g.dtype == r.dtype, (what, k, g.shape, r.shape, g.dtype, r.dtype)
        assert np.array_equal(g, r, equal_nan=True), (what, k, np.argwhere(~((g == r) | (np.isnan(g) & np.isnan(r))))[:5])


def _fold(a, b, off=0.0, ranks=()):
    from mmseq_amd import Fold
    with Fold.of_traces(a, b, off, ranks) as h:
        return h.summary()


def _ranks(n):
    """the edges, the percentiles of the CLI's defaults, a duplicate, and one rank that is not there"""
    return [0, n - 1, n // 2, R.percentile_rank(2.5, n), R.percentile_rank(97.5, n), n // 2, n, R.percentile_rank(1, n)]


@pytest.mark.parametrize("Sa,Sb", [(1, 1), (2, 3), (3, 2), (64, 64), (100, 1024), (1024, 1024), (4096, 4096), (4096, 1)])
def test_every_output_is_the_references_at_every_size(gpu, Sa, Sb):
    """4096: 64 KiB of LDS, the cap; 100 and 3: padded sorts; (4096, 1) and (1, 1): a side of one draw.  Three significant digits:
    ties among the draws and between the sides"""
    rng = np.random.default_rng(Sa * 5 + Sb)
    F = 1 if Sa * Sb > (1 << 20) else 3
    a, b = _draws(rng, F, Sa, sig=3), _draws(rng, F, Sb, sig=3) * 1.5
    ranks = _ranks(Sa * Sb)
    off = 0.375
    got = _fold(a, b, off, ranks)
    ref = R.summary_ref(a, b, off, ranks)
    _same(got, ref, (Sa, Sb))
    assert np.isnan(got["quantiles"][:, 6]).all() and np.isfinite(got["quantiles"][:, :6]).all()
    assert np.array_equal(got["quantiles"][:, 2], got["quantiles"][:, 5])
    assert (got["status"] == 0).all()


@pytest.fixture(scope="module")
def thousand():
    """1003 features of 37 x 50 draws, two significant digits, with invalid features between valid ones; the reference once"""
    rng = np.random.default_rng(77)
    F, Sa, Sb = 1003, 37, 50
    a, b = _draws(rng, F, Sa, sig=2), _draws(rng, F, Sb, sig=2)
    a[3, 5] = 0.0; b[4, 49] = np.nan; a[255, 0] = -1.0; a[256, 36] = np.inf; b[256, 0] = 0.0; b[1002, 7] = -np.inf
    ranks = _ranks(Sa * Sb)
    return a, b, 0.25, ranks, R.summary_ref(a, b, 0.25, ranks)


@pytest.mark.parametrize("F", [1, 2, 257, 1003])
def test_feature_counts(gpu, thousand, F):
    a, b, off, ranks, ref = thousand
    got = _fold(a[:F], b[:F], off, ranks)
    _same(got, {k: ref[k][:F] for k in KEYS}, F)


@pytest.mark.parametrize("cap", [1, 2, 100])
def test_slab_edges_do_not_change_a_bit(gpu, thousand, cap):
    from mmseq_amd import Fold
    a, b, off, ranks, ref = thousand
    F = 257
    with gpu.options(fold_slab=cap):
        with Fold.of_traces(a[:F], b[:F], off, ranks) as h:
            got = h.summary()
            assert h.device_bytes() == 8 * cap * (37 + 50) + cap * (41 + 8 * len(ranks)) + 4 * len(ranks)
    _same(got, {k: ref[k][:F] for k in KEYS}, cap)


def test_invalid_features_get_their_bits_and_leave_their_neighbours_alone(gpu):
    rng = np.random.default_rng(5)
    Sa, Sb = 130, 70
    a, b = _draws(rng, 11, Sa), _draws(rng, 11, Sb)
    a[1, 129] = 0.0
    a[2, 0] = -2.5
    a[4, 64] = np.nan
    a[5, 3] = np.inf
    b[6, 69] = 0.0
    b[7, 0] = -1e-300
    b[8, 33] = np.nan
    b[9, 1] = np.inf
    a[9, 1] = -np.inf
    ranks = _ranks(Sa * Sb)
    got = _fold(a, b, -0.5, ranks)
    assert list(got["status"]) == [0, 1, 1, 0, 1, 1, 2, 2, 2, 3, 0]
    bad = got["status"] != 0
    for k in ("mean_a", "mean_b", "ss_a", "ss_b", "lfc", "sd", "p_gt"):
        assert np.isnan(got[k][bad]).all(), k
    assert np.isnan(got["quantiles"][bad]).all() and (got["n_gt"][bad] == 0).all() and (got["n_eq"][bad] == 0).all()
    _same(got, R.summary_ref(a, b, -0.5, ranks))
    alone = _fold(a[~bad], b[~bad], -0.5, ranks)               # the valid features without their neighbours: the same bits
    for k in KEYS:
        assert np.array_equal(got[k][~bad], alone[k], equal_nan=True), k


@pytest.mark.parametrize("sig", [2, 6])
def test_rounded_draws_tie_and_the_counts_stay_exact(gpu, sig):
    rng = np.random.default_rng(sig)
    Sa, Sb = 300, 257
    base = _draws(rng, 4, Sa + Sb, sig=sig)
    a, b = base[:, :Sa], base[:, Sa:]
    ranks = _ranks(Sa * Sb)
    got = _fold(a, b, 0.0, ranks)
    _same(got, R.summary_ref(a, b, 0.0, ranks), sig)
    if sig == 2:
        assert (got["n_eq"] > 0).all()


def test_constant_sides_exact_ties_by_the_offset_and_wide_magnitudes(gpu):
    rng = np.random.default_rng(8)
    Sa, Sb = 96, 65
    a, b = _draws(rng, 6, Sa, sig=3), _draws(rng, 6, Sb, sig=3)
    a[0] = 0.75                                                # a constant A
    b[1] = 3.0                                                 # a constant B
    a[2] = 2.0; b[2] = 2.0                                     # both constant and equal: every pair ties
    a[3] = rng.choice([1.0, 2.0, 4.0], Sa); b[3] = 1.0          # with off = log 2, y == log 2 == x wherever a == 2
    a[4] = 10.0 ** rng.uniform(-300, 300, Sa); b[4] = 10.0 ** rng.uniform(-300, 300, Sb)
    a[4, :2] = (1e-300, 1e300); b[4, :2] = (1e300, 1e-300)
    a[5] = b[5, rng.integers(0, Sb, Sa)]                        # A's draws are draws of B
    ranks = _ranks(Sa * Sb)
    for off in (float(R.dlog(np.array([2.0]))[0]), 0.0, -0.0):
        got = _fold(a, b, off, ranks)
        _same(got, R.summary_ref(a, b, off, ranks), off)
        if off == 0.0:
            assert got["n_eq"][2] == Sa * Sb and got["n_gt"][2] == 0 and (got["quantiles"][2, :6] == 0.0).all() and got["p_gt"][2] == 0.5
            assert got["n_eq"][5] >= Sa
        else:
            assert got["n_eq"][3] == Sb * int((a[3] == 2.0).sum()) and got["n_gt"][3] == Sb * int((a[3] == 4.0).sum())


def test_reruns_are_bit_identical(gpu):
    from mmseq_amd import Fold
    rng = np.random.default_rng(12)
    a, b = _draws(rng, 40, 500, sig=4), _draws(rng, 40, 333, sig=4)
    ranks = _ranks(500 * 333)
    with Fold.of_traces(a, b, 0.1, ranks) as h:
        first, again = h.summary(), h.summary()
    rerun = _fold(a, b, 0.1, ranks)
    for k in KEYS:
        assert np.array_equal(first[k], again[k], equal_nan=True) and np.array_equal(first[k], rerun[k], equal_nan=True), k
    none = _fold(a, b, 0.1)                                    # no ranks asked: the rest is what it was
    assert none["quantiles"].shape == (40, 0)
    for k in ("mean_a", "mean_b", "ss_a", "ss_b", "n_gt", "n_eq", "status"):
        assert np.array_equal(first[k], none[k]), k


def test_samplers_resident_traces_give_the_bits_of_the_downloaded_ones(gpu, orc):
    """two generated problems, one renumbered on the device, chains of 64 and 128 kept samples; features are a permutation on each side"""
    from mmseq_amd import Fold
    rng = np.random.default_rng(21)
    made = []
    for seed, S, chains, renumber in ((11, 64, 2, True), (12, 128, 1, False)):
        p, _ = orc.synth_problem(R=4000, T=200, avg_hits=4, seed=seed, sort=False)
        txo = ((rng.permutation(p.n).astype(np.uint64) // np.uint64(4)) << np.uint64(32)) if renumber else None
        prob = gpu.Problem.from_csr(p.row_ptr, p.col_idx, p.l, tx_order=txo)
        mu0, _ = prob.start_values()
        smp = gpu.Sampler(prob, mu0, seed=seed, n_chains=chains, gibbs_iter=S, trace_len=S)
        smp.run(S)
        made.append((prob, smp, p.n, S))
    (pa, sa, na, Sa), (pb, sb, nb, Sb) = made
    F = min(na, nb) + 50                                       # a permutation on each side, then members that occur twice
    ia = np.concatenate([rng.permutation(na)[:F - 50], rng.integers(0, na, 50)])
    ib = np.concatenate([rng.permutation(nb)[:F - 50], rng.integers(0, nb, 50)])
    ranks = _ranks(Sa * Sb)
    ta, tb = sa.trace(1), sb.trace(0)
    for cap in (-1, 7):
        with gpu.options(fold_slab=cap):
            with Fold.of_samplers(sa, sb, ia, ib, 0.2, ranks, chain_a=1) as h, Fold.of_traces(ta[ia], tb[ib], 0.2, ranks) as g:
                x, y = h.summary(), g.summary()
                c = F if cap < 0 else cap
                assert g.device_bytes() == 8 * c * (Sa + Sb) + c * (41 + 8 * len(ranks)) + 4 * len(ranks)
                assert h.device_bytes() == g.device_bytes() + 8 * c
        for k in KEYS:
            assert np.array_equal(x[k], y[k], equal_nan=True), (cap, k)
    _same(x, R.summary_ref(ta[ia], tb[ib], 0.2, ranks))
    with Fold.of_samplers(sa, sa, ia, ia, 0.0, [0, Sa * Sa - 1], chain_a=0, chain_b=0) as h:     # a chain against itself
        s = h.summary()
        assert (s["lfc"] == 0.0).all() and (s["p_gt"] == 0.5).all() and np.array_equal(s["quantiles"][:, 0], -s["quantiles"][:, 1])
    for prob, smp, _, _ in made:
        smp.close(); prob.close()


def _live(lib):
    from mmseq_amd import _lib
    c = (C.c_int64 * 3)()
    _lib.check(lib.mmg_selftest_live(c))
    return list(c)


def test_the_errors_leave_the_library_usable(gpu):
    from mmseq_amd import Fold, _lib
    from mmseq_amd._lib import MMGError
    lib = _lib.load()
    rng = np.random.default_rng(9)
    a, b = _draws(rng, 5, 16), _draws(rng, 5, 9)
    good = _fold(a, b, 0.0, [0, 143])
    gc.collect()
    base = _live(lib)
    hnd = C.c_void_p()
    pa, pb = a.ctypes.data_as(C.c_void_p), b.ctypes.data_as(C.c_void_p)
    rk = np.array([0, 1], np.uint32)
    pr = rk.ctypes.data_as(C.c_void_p)

    def of(F=5, Sa=16, a_=pa, Sb=9, b_=pb, off=0.0, nr=2, r=pr, out=C.byref(hnd)):
        rc = lib.mmg_fold_of_traces(0, F, Sa, a_, Sb, b_, off, nr, r, out)
        return rc, lib.mmg_last_error().decode()

    for kw, text in ((dict(F=0), "n_features"), (dict(Sa=0), "Sa"), (dict(Sa=4097), "Sa = 4097"), (dict(Sb=0), "Sb"), (dict(Sb=4097), "Sb = 4097"),
                     (dict(nr=65), "n_ranks = 65"), (dict(r=None), "ranks"), (dict(off=float("nan")), "off"), (dict(off=float("inf")), "off"),
                     (dict(a_=None), "NULL"), (dict(b_=None), "NULL"), (dict(out=None), "NULL")):
        rc, msg = of(**kw)
        assert rc == 1 and text in msg, (kw, rc, msg)
    rc, msg = of(nr=0, r=None)                                 # no ranks, no array: in order
    assert rc == 0
    lib.mmg_fold_destroy(hnd)
    assert lib.mmg_fold_of_traces(99, 5, 16, pa, 9, pb, 0.0, 2, pr, C.byref(hnd)) == 1 and b"device" in lib.mmg_last_error()
    assert lib.mmg_fold_get(None, *[None] * 8) == 1 and lib.mmg_fold_device_bytes(None, None) == 1
    lib.mmg_fold_destroy(None)
    assert _live(lib) == base
    # the samplers' side
    q = gpu.Problem.from_csr(np.array([0, 2], np.uint64), np.array([0, 1], np.uint32), np.ones(2))
    smp = gpu.Sampler(q, np.ones(2), gibbs_iter=8, trace_len=4)
    done = gpu.Sampler(q, np.ones(2), gibbs_iter=4, trace_len=4)
    done.run(4)
    smp.run(4)
    smp.sync()
    for kw, code, text in ((dict(chain_a=1), 1, "chain_a out of range"), (dict(chain_b=-1), 1, "chain_b out of range")):
        with pytest.raises(MMGError) as e:
            Fold.of_samplers(done, done, [0], [1], **kw)
        assert e.value.code == code and text in str(e.value)
    with pytest.raises(MMGError) as e:
        Fold.of_samplers(done, done, [0, 1], [1, 2])
    assert e.value.code == 1 and "feature 1: ib = 2 out of range (n = 2)" in str(e.value)
    with pytest.raises(MMGError) as e:
        Fold.of_samplers(done, done, [0], [1], ranks=list(range(65)))
    assert e.value.code == 1 and "n_ranks" in str(e.value)
    with pytest.raises(MMGError) as e:
        Fold.of_samplers(done, done, [], [])
    assert e.value.code == 1 and "n_features" in str(e.value)
    one = np.array([0], np.uint32).ctypes.data_as(C.c_void_p)
    assert lib.mmg_fold_create(None, 0, done._h, 0, 1, one, one, 0.0, 0, None, C.byref(hnd)) == 1
    assert lib.mmg_fold_create(done._h, 0, done._h, 0, 1, None, one, 0.0, 0, None, C.byref(hnd)) == 1
    assert lib.mmg_fold_create(done._h, 0, done._h, 0, 1, one, one, 0.0, 0, None, None) == 1
    for sa, sb, which in ((smp, done, "sa"), (done, smp, "sb")):                # 2 of 4 samples kept on one side
        with pytest.raises(MMGError) as e:
            Fold.of_samplers(sa, sb, [0], [1])
        assert e.value.code == 4 and which in str(e.value)
    bare = gpu.Sampler(q, np.ones(2), gibbs_iter=4, trace_len=4, keep_trace=False)
    bare.run(4)
    with pytest.raises(MMGError) as e:
        Fold.of_samplers(done, bare, [0], [1])
    assert e.value.code == 4 and "keep_trace" in str(e.value)
    smp.run(4)
    with Fold.of_samplers(smp, done, [0, 1], [1, 1], 0.0, [0, 15]) as h:
        s = h.summary()
        ta, tb = smp.trace(0), done.trace(0)
        _same(s, R.summary_ref(ta[[0, 1]], tb[[1, 1]], 0.0, [0, 15]))
    bare.close(); smp.close(); done.close(); q.close()
    after = _fold(a, b, 0.0, [0, 143])                         # the device is as usable as before
    for k in KEYS:
        assert np.array_equal(after[k], good[k], equal_nan=True), k


def test_failed_acquisitions_give_back_everything(gpu):
    from mmseq_amd import Fold, _lib
    from mmseq_amd._lib import MMGError
    lib = _lib.load()
    rng = np.random.default_rng(10)
    a, b = _draws(rng, 9, 70), _draws(rng, 9, 40)
    want = _fold(a, b, 0.0, [0, 5])
    gc.collect()
    base = _live(lib)
    v = 0
    try:
        with gpu.options(fold_slab=4):
            while True:
                _lib.check(lib.mmg_selftest_option(_lib.OPT_FAIL_ALLOC, v))
                try:
                    h = Fold.of_traces(a, b, 0.0, [0, 5])
                except MMGError as e:
                    assert e.code == 3 and str(e)
                    assert _live(lib) == base, v
                    v += 1
                    continue
                break
    finally:
        lib.mmg_selftest_option(_lib.OPT_FAIL_ALLOC, -1)
    assert v == 8                                              # the stream and the seven buffers of the pass
    assert _live(lib) == base                                  # nothing is held after create
    got = h.summary()
    h.close()
    for k in KEYS:
        assert np.array_equal(got[k], want[k], equal_nan=True), k


# ------------------------------------------------------------------------------------------ the CLI
@pytest.fixture(scope="module")
def cli_samples(tmp_path_factory):
    """two samples at the transcript and the gene level: 6 features; B's trace file lacks f4, f2 of A has a zero draw"""
    d = tmp_path_factory.mktemp("mmfold_gpu")
    rng = np.random.default_rng(31)
    ids = ["f%d" % i for i in range(6)]
    out = {}
    for level in ("transcript", "gene"):
        per = {}
        for name, lack in (("a", None), ("b", "f4")):
            base = str(d / name)
            log_mu = list(rng.normal(1.0, 1.0, 6))
            log_mu[5] = "NA" if name == "b" else log_mu[5]
            uh = [int(u) for u in rng.integers(0, 6, 6)]
            uh[0], uh[1] = 5, 4
            write_table(base + INFIX[level] + ".mmseq", ids, log_mu, uh)
            tids = [i for i in ids if i != lack]
            draws = np.exp(rng.normal(-2.0, 1.0, len(tids))[:, None] + 0.4 * rng.normal(0.0, 1.0, (len(tids), TRACELEN)))
            if name == "a":
                draws[2, 100] = 0.0
            tids = tids[::-1]                                  # the files' columns are in another order than the tables' rows
            read = write_trace(base + INFIX[level] + ".trace_gibbs.gz", tids, draws[::-1])
            per[name] = dict(base=base, log_mu=[np.nan if isinstance(v, str) else v for v in log_mu], uh=uh, draws=dict(zip(tids, read)))
        out[level] = per
    return ids, out


@pytest.mark.parametrize("level,flags", [("transcript", []), ("gene", ["-nonorm"]), ("transcript", ["-offset", "-0.3", "-percentiles", "0,50,100", "-gfold", "0.1"]),
                                         ("gene", ["-uhmin", "4"])])
def test_cli_table_is_the_restatements_byte_for_byte(gpu, cli_samples, level, flags):
    ids, per = cli_samples
    A, B = per[level]["a"], per[level]["b"]
    percentiles, c, uhmin = [2.5, 50.0, 97.5], 0.01, 1
    if "-percentiles" in flags:
        percentiles, c = [0.0, 50.0, 100.0], 0.1
    if "-uhmin" in flags:
        uhmin = 4
    if "-nonorm" in flags:
        off, n_off = 0.0, 0
    elif "-offset" in flags:
        off, n_off = -0.3, 0
    else:
        off, n_off = R.offset_rule(A["log_mu"], B["log_mu"], A["uh"], B["uh"], uhmin)
        assert n_off >= 2
    have = [i in A["draws"] and i in B["draws"] for i in ids]
    assert have == [True, True, True, True, False, True]
    a = np.array([A["draws"][i] for i, h in zip(ids, have) if h])
    b = np.array([B["draws"][i] for i, h in zip(ids, have) if h])
    n = TRACELEN * TRACELEN
    dev = R.fold_ref(a, b, off, R.cli_ranks(percentiles, c, n))
    assert list(dev["status"]) == [0, 0, 1, 0, 0]
    want = R.table(A["base"], B["base"], level, ids, have, dev, TRACELEN, TRACELEN, off, n_off, percentiles, c)
    r = subprocess.run([MMFOLD, "-level", level] + flags + [A["base"], B["base"]], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr
    assert r.stdout == want
