"""mmg_sampler_extend: a finished run of length L, extended, is bit for bit the first half of a run planned at 2 L.
Every comparison is ==; traces are compared as bit patterns, so the zeros behind the kept rows are +0.0 as in a new sampler.

Shapes: n = 1, 2, 63, 64, 65, 129 (odd n: rows are only 8-byte aligned; one transcript past a wave and past two), 1 and 3 chains,
trace_len 2, 8, 16, 64 (8 and 16: every row distinct, where a wrong order of the in-place move shows), thinning 1 and 3, and a problem
the library renumbers (tx_order)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SEED = 4711


def small_csr(n, seed):
    """m rows of 1 .. 4 distinct hits among n transcripts (ascending within a row), every transcript hit"""
    rng = np.random.default_rng(seed)
    rows = [[t] for t in range(n)]
    for _ in range(max(40, 12 * n)):
        k = int(rng.integers(1, min(n, 4) + 1))
        rows.append(sorted(int(t) for t in rng.choice(n, size=k, replace=False)))
    order = rng.permutation(len(rows))
    rows = [rows[i] for i in order]
    rp = np.zeros(len(rows) + 1, np.uint64)
    rp[1:] = np.cumsum([len(r) for r in rows])
    ci = np.array([t for r in rows for t in r], np.uint32)
    l = rng.uniform(200.0, 3000.0, n)
    return rp, ci, l


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def state(s, with_trace=False):
    d = {"iteration": s.iteration}
    for c in range(s.n_chains):
        d["rows%d" % c] = bits(s.trace_rows(c))
        sl, sl2, ns = s.moments(c)
        d["sl%d" % c], d["sl2%d" % c], d["ns%d" % c] = bits(sl), bits(sl2), ns
        d["mu%d" % c] = bits(s.mu(c))
        d["cnt%d" % c] = s.counts(c)
        if with_trace:
            d["trace%d" % c] = bits(s.trace(c))
    return d


def same(a, b, label):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (label, k)


def identity(gpu, prob, mu0, n_chains, S, ss, seed=SEED):
    """A planned at S ss and extended twice, against B planned at 2 S ss and D planned at 4 S ss"""
    L = S * ss
    label = "n=%d C=%d S=%d ss=%d" % (prob.info.n, n_chains, S, ss)
    mk = lambda length: gpu.Sampler(prob, mu0, seed=seed, n_chains=n_chains, gibbs_iter=length, trace_len=S)
    a, b, d = mk(L), mk(2 * L), mk(4 * L)
    a.run(L)
    full = state(a)
    a.extend()
    b.run(L)
    sa = state(a)
    same(sa, state(b), label + " after extend")
    assert sa["iteration"] == L and sa["ns0"] == S // 2
    for c in range(n_chains):                              # the kept rows are the even rows of the run of L; zeros (+0.0) behind them
        assert np.array_equal(sa["rows%d" % c][:S // 2], full["rows%d" % c][0::2]), label
        assert not sa["rows%d" % c][S // 2:].any(), label
    a.run(L)
    b.run(L)
    sa = state(a, True)
    same(sa, state(b, True), label + " at 2 L")
    assert sa["ns0"] == S
    a.extend()
    d.run(2 * L)
    same(state(a), state(d), label + " after the second extend")
    a.run(2 * L)
    d.run(2 * L)
    same(state(a, True), state(d, True), label + " at 4 L")
    for s in (a, b, d):
        s.close()
    return sa


@pytest.fixture(scope="module")
def problems(gpu):
    out = {}
    for n in (1, 2, 63, 64, 65, 129):
        rp, ci, l = small_csr(n, 100 + n)
        prob = gpu.Problem.from_csr(rp, ci, l)
        out[n] = (prob, prob.start_values()[0])
    return out


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 129])
def test_extended_run_equals_the_run_planned_at_twice_the_length(gpu, problems, n):
    prob, mu0 = problems[n]
    for n_chains in (1, 3):
        for S in (2, 8, 16, 64):
            for ss in (1, 3):
                identity(gpu, prob, mu0, n_chains, S, ss)


def test_renumbered_transcripts(gpu):
    n = 65
    rp, ci, l = small_csr(n, 7)
    txo = np.random.default_rng(7).permutation(n).astype(np.uint64)
    prob = gpu.Problem.from_csr(rp, ci, l, tx_order=txo)
    assert not np.array_equal(prob.tx_perm(), np.arange(n))   # device and caller numberings differ
    mu0, _ = prob.start_values()
    for S, ss in ((8, 1), (16, 3)):
        identity(gpu, prob, mu0, 3, S, ss)


def test_extended_run_equals_the_oracle_chain_at_the_doubled_length(gpu, orc):
    """the identity against the keyed specification, not only against the library's other path"""
    n, S, ss = 65, 16, 3
    L = S * ss
    rp, ci, l = small_csr(n, 21)
    prob = gpu.Problem.from_csr(rp, ci, l)
    srp, sci = prob.download()                               # the stored rows: what the oracle replays
    p = orc.Problem(srp, sci, l)
    mu0, _ = prob.start_values()
    a = gpu.Sampler(prob, mu0, seed=SEED, n_chains=2, gibbs_iter=L, trace_len=S)
    a.run(L)
    a.extend()
    a.run(L)
    for c in range(2):
        ref = orc.gibbs_keyed(p, mu0, seed=SEED, chain=c, n_iter=2 * L, trace_len=S)
        assert np.array_equal(bits(a.trace(c)), bits(ref["trace"]))
        sl, sl2, ns = a.moments(c)
        assert np.array_equal(bits(sl), bits(ref["sum_log"])) and np.array_equal(bits(sl2), bits(ref["sum_log2"])) and ns == S
        assert np.array_equal(bits(a.mu(c)), bits(ref["mu"])) and np.array_equal(a.counts(c), ref["cnt"])


def test_two_extended_runs_agree(gpu, problems):
    prob, mu0 = problems[129]
    runs = []
    for _ in range(2):
        s = gpu.Sampler(prob, mu0, seed=SEED, n_chains=3, gibbs_iter=48, trace_len=16)
        s.run(48)
        s.extend()
        s.run(48)
        runs.append(state(s, True))
    same(runs[0], runs[1], "rerun")


def _raises(code, word, fn):
    from mmseq_amd._lib import MMGError
    with pytest.raises(MMGError) as e:
        fn()
    assert e.value.code == code and word in str(e.value), str(e.value)


def test_states_and_arguments(gpu, problems):
    prob, mu0 = problems[64]
    s = gpu.Sampler(prob, mu0, seed=SEED, gibbs_iter=16, trace_len=8)
    s.run(15)
    _raises(4, "not complete", s.extend)                     # before the end
    s.sample()
    _raises(4, "between sample() and update()", s.extend)
    s.update()
    assert s.iteration == 16
    s.extend()
    assert s.gibbs_iter == 32
    _raises(4, "not complete", s.extend)                     # the extended run is at its half
    s = gpu.Sampler(prob, mu0, seed=SEED, gibbs_iter=16, trace_len=8, keep_trace=False)
    s.run(16)
    _raises(4, "keep_trace", s.extend)
    s = gpu.Sampler(prob, mu0, seed=SEED, gibbs_iter=14, trace_len=7)
    s.run(14)
    _raises(1, "trace_len must be even", s.extend)
    s = gpu.Sampler(prob, mu0, seed=SEED, gibbs_iter=(1 << 30) + 8, trace_len=8)
    _raises(1, "2^30", s.extend)
    assert s.gibbs_iter == (1 << 30) + 8


def test_summary_begun_before_an_extend_is_stale(gpu, problems):
    prob, mu0 = problems[65]
    s = gpu.Sampler(prob, mu0, seed=SEED, gibbs_iter=16, trace_len=16)
    s.run(16)
    s.sync()
    q = gpu.Summary(s, staged=True)
    q.advance(8)
    q.rows(gpu.SERIES_TRANSCRIPT, 0, 8)
    s.extend()
    _raises(4, "extended", lambda: q.advance(16))
    _raises(4, "extended", lambda: q.rows(gpu.SERIES_TRANSCRIPT, 0, 8))
    _raises(4, "extended", q.finish)
    q.close()
    s.run(16)
    s.sync()
    q = gpu.Summary(s, staged=True)                          # begun after the extend: works as on a plain sampler
    q.advance(16)
    q.finish()
    plain = gpu.Sampler(prob, mu0, seed=SEED, gibbs_iter=32, trace_len=16)
    plain.run(32)
    want = gpu.Summary(plain)
    for k in ("log_mean", "var", "tau"):
        assert np.array_equal(q.series(gpu.SERIES_TRANSCRIPT)[k], want.series(gpu.SERIES_TRANSCRIPT)[k], equal_nan=True)


def test_full_trace_handles_refuse_a_half_filled_trace(gpu, problems):
    from mmseq_amd import Fold, Pairs
    prob, mu0 = problems[65]
    s = gpu.Sampler(prob, mu0, seed=SEED, gibbs_iter=16, trace_len=16)
    s.run(16)
    ia = np.arange(4, dtype=np.uint32)
    pr = np.array([[0, 1], [2, 3]], np.uint32)
    Fold.of_samplers(s, s, ia, ia[::-1].copy()).close()
    Pairs.from_sampler(s, pr).close()
    s.extend()
    _raises(4, "the fold is taken after the last kept sample", lambda: Fold.of_samplers(s, s, ia, ia[::-1].copy()))
    _raises(4, "pairs are taken after the chain's last kept sample", lambda: Pairs.from_sampler(s, pr))
    s.run(16)
    Fold.of_samplers(s, s, ia, ia[::-1].copy()).close()
    Pairs.from_sampler(s, pr).close()


def test_failed_acquisitions_leave_the_sampler_as_it_was(gpu, problems):
    from mmseq_amd import _lib
    from mmseq_amd._lib import MMGError
    lib = _lib.load()
    prob, mu0 = problems[129]
    S, L = 16, 48

    def live():
        c = (C.c_int64 * 3)()
        _lib.check(lib.mmg_selftest_live(c))
        return list(c)

    a = gpu.Sampler(prob, mu0, seed=SEED, n_chains=3, gibbs_iter=L, trace_len=S)
    a.run(L)
    before = state(a, True)
    base = live()
    v = 0
    while True:
        _lib.check(lib.mmg_selftest_option(_lib.OPT_FAIL_ALLOC, v))
        try:
            a.extend()
        except MMGError as e:
            lib.mmg_selftest_option(_lib.OPT_FAIL_ALLOC, -1)
            assert e.code == 3 and str(e)
            assert live() == base, v
            assert a.gibbs_iter == L
            same(state(a, True), before, "after failed acquisition %d" % v)
            v += 1
            assert v < 16
            continue
        finally:
            lib.mmg_selftest_option(_lib.OPT_FAIL_ALLOC, -1)
        break
    assert v >= 1                                            # the scratch buffer at least
    assert live() == base
    b = gpu.Sampler(prob, mu0, seed=SEED, n_chains=3, gibbs_iter=2 * L, trace_len=S)
    b.run(L)
    same(state(a), state(b), "extend after the failures")
    a.run(L)
    b.run(L)
    same(state(a, True), state(b, True), "at 2 L after the failures")
