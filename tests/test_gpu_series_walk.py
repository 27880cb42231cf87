"""The workspace instantiations of the four per-series kernels (k_series_summary<0, .>, k_convergence<0>, k_pooled_summary<0, .>,
k_contrast_summary<0>: series too long for LDS) when a workgroup walks SEVERAL series, `for (ser = blockIdx.x; ser < count; ser +=
gridDim.x)`.  In production 1024 workgroups stride over every transcript; on test inputs MMG_OPT_SERIES_GROUPS caps the workgroups, so
that 7 series are walked by 1, 2 and 3 of them (7; 4 and 3; 3, 2 and 2 series in a row), and the production geometry is taken once with
the option unset: 1027 series, of which workgroups 0 to 2 take a second one.

Every test first asserts with mmg_selftest_series_launch that the launch had the grid it is about (a launch site that forgot the option
would leave the rest vacuous), then that every output under the option is the unset run's bit for bit, then the series_groups = 2
result against the reference of the entry's own test (convergence_ref with _check, pooled_ref, contrast_ref, numpy's sort with the
oracle's Sokal, AS 241 on the device's logarithm) with that test's own helpers and tolerances.

The series are ordered so that what one leaves behind would show in the next (with two workgroups the even indices share one): a long
Geyer walk before a constant series before a short walk, series 60 orders of magnitude apart side by side, Sokal's early return (a
length that is no power of two) before the next series, an all-NaN proportion series between finite ones."""
import numpy as np
import pytest

import contrast_ref as CR
import convergence_ref as VR
import pooled_ref as PR
from key_space_checks import probit_as241
from test_gpu_contrast import _check_summary, _dlog
from test_gpu_convergence import KINDS, _ar1, _check, _mixed
from test_gpu_pooled import COLS, _positive, _same
from test_gpu_summary import check_log_series, check_proportions

pytestmark = pytest.mark.gpu

GROUPS = (1, 2, 3)
WS_GROUPS = 1024                    # SERIES_WS_GROUPS, CONV_WS_GROUPS, POOL_WS_GROUPS, CONTRAST_WS_GROUPS
LOG_COLS = ("log_mean", "var", "tau", "rc", "percentiles")
PROP_COLS = ("mean", "probit_mean", "probit_sd", "percentiles")


def _launch_is(gpu, kernel, v, count):
    """the last workspace launch of `kernel`: min(v, count) workgroups (v None: the library's own 1024) over `count` series"""
    assert gpu.selftest_series_launch(kernel) == (min(v or WS_GROUPS, count), count), (kernel, v)


def _walks(gpu, run):
    """{v: run(v)} for the option unset (None) and series_groups = 1, 2, 3; run asserts its launches itself.  (Under the option the
    library fills the result columns with 0xFF bytes before the launch: a series that no workgroup reached reads NaN / -1 here, whatever
    an earlier call left in the memory the allocator hands out.)"""
    out = {None: run(None)}
    for v in GROUPS:
        with gpu.options(series_groups=v):
            out[v] = run(v)
    return out


def _same_bits(walks, keys):
    for v in GROUPS:
        _same(walks[v], walks[None], keys, "series_groups %d against the option unset" % v)


def _scales(count):
    """neighbouring series 60 orders of magnitude apart"""
    return np.where(np.arange(count) % 2 == 0, 1e-30, 1e30)


# ------------------------------------------------------------------------------------------ the hook itself
def test_the_option_is_an_upper_bound_and_restores(gpu):
    """more groups than series or than the library's 1024 change nothing; leaving the context restores the library's choice"""
    rng = np.random.default_rng(1)
    x = rng.normal(size=(3, 4096, 5))
    want = gpu.convergence_of_traces(x)
    _launch_is(gpu, "convergence", None, 5)
    for v in (5, 6, 4000):
        with gpu.options(series_groups=v):
            got = gpu.convergence_of_traces(x)
        _launch_is(gpu, "convergence", v, 5)
        _same(got, want, KINDS)
    with gpu.options(series_groups=0):                            # v >= 1 caps; 0 is no cap
        gpu.convergence_of_traces(x)
    _launch_is(gpu, "convergence", None, 5)
    gpu.convergence_of_traces(x[:, :64])                          # in LDS: not a workspace launch, the record stays
    _launch_is(gpu, "convergence", None, 5)
    from mmseq_amd import _lib
    assert _lib.load().mmg_selftest_series_launch(4, None, None) == 1 and _lib.load().mmg_selftest_series_launch(0, None, None) == 1


# ------------------------------------------------------------------------------------------ convergence
def _conv_series(rng, C_, S):
    """7 series: 0 AR(1) at 0.9 (a long Geyer walk: many lags into the scratch on the keys), 2 constant (three NaNs, the `continue`),
    4 iid (a short walk, which must not read stale lags), 6 heavy integer ties; 1 a shifted chain, 3 AR(1) at 0.5, 5 a second constant
    (with two workgroups the second one ends on it, with three the third)"""
    x = rng.normal(size=(C_, S, 7))
    x[:, :, 0] = _ar1(rng, C_, S, 1, 0.9)[:, :, 0]
    x[C_ - 1, :, 1] += 3.0
    x[:, :, 2] = 1.25
    x[:, :, 3] = _ar1(rng, C_, S, 1, 0.5)[:, :, 0]
    x[:, :, 5] = -7.0
    x[:, :, 6] = rng.integers(0, 4, size=(C_, S))
    return x


@pytest.mark.parametrize("C_,S", [(3, 4096), (2, 4099)])
def test_convergence_walks(gpu, C_, S):
    """(2, 4099): an odd S, the split drops the middle draw"""
    x = _conv_series(np.random.default_rng(C_ * 10000 + S), C_, S)

    def run(v):
        got = gpu.convergence_of_traces(x)
        _launch_is(gpu, "convergence", v, 7)
        return got

    walks = _walks(gpu, run)
    _same_bits(walks, KINDS)
    got = walks[2]
    _check(got, VR.diagnostics_of_traces(x), "C=%d S=%d, two workgroups" % (C_, S))
    for k in KINDS:
        assert np.isnan(got[k][[2, 5]]).all() and np.isfinite(got[k][[0, 1, 3, 4, 6]]).all(), k
    assert got["ess_bulk"][0] < 0.5 * got["ess_bulk"][4]          # the long walk and the short one are what they are meant to be


# ------------------------------------------------------------------------------------------ pooled, traces from the host
def _pooled_series(rng, C_, S):
    """the 7 series of the convergence test made positive, neighbours 60 orders of magnitude apart, a NaN in series 1 and a +inf in
    series 3 (NaNs and the padding sort last: the order statistics at N - 1 and N)"""
    x = np.exp(_conv_series(rng, C_, S)) * _scales(7)
    x[C_ - 1, S // 2, 1] = np.nan
    x[0, S - 1, 3] = np.inf
    return x


@pytest.mark.parametrize("C_,S", [(3, 4096), (2, 16384)])
def test_pooled_of_traces_walks(gpu, C_, S):
    """(3, 4096): N = 12288 is no power of two, padding above the real keys; (2, 16384): the chains' columns, 14 series of 16384, take
    k_series_summary<0, true> through launch_chain_columns on the series workspace"""
    x = _pooled_series(np.random.default_rng(C_ * 10000 + S), C_, S)
    N = C_ * S
    pidx = [0, N - 1, -1, N, N // 2, N // 3]

    def run(v):
        got = gpu.pooled_of_traces(x, pidx)
        _launch_is(gpu, "pooled", v, 7)
        if S > 8192:
            _launch_is(gpu, "series", v, 7 * C_)
        return got

    walks = _walks(gpu, run)
    _same_bits(walks, COLS)
    got = walks[2]
    _same(got, PR.pooled_of_traces(x, pidx, log=_dlog(gpu)), COLS, "C=%d S=%d, two workgroups" % (C_, S))
    assert np.isnan(got["percentiles"][:, 2:4]).all() and (got["rc"] == 0).all()
    assert np.isnan(got["percentiles"][1, 1]) and np.isinf(got["percentiles"][3, 1]) and np.isfinite(got["percentiles"][[0, 2, 4, 5, 6], 1]).all()


# ------------------------------------------------------------------------------------------ from a sampler
VID = np.array([901, 902, 903, 904], np.uint64)
VSCALE = np.array([0.5, 2.0, 0.1, 1.0])


def _tiny(gpu, orc, T, n_chains, S, seed):
    """a sampler of T transcripts that has run, and a description: 4 isoforms without hits (T .. T + 3; the last launch of a kind is
    theirs, and 4 series tell 1, 2 and 3 workgroups from the library's choice), transcript 2 outside every gene between finite
    neighbours, transcript 3 a gene of its own (probit mean +inf, sd NaN) directly before the multi-isoform gene of 4 .., one identical set"""
    p, _ = orc.synth_problem(R=400, T=T, avg_hits=3, seed=seed, sort=False)
    assert p.n == T
    prob = gpu.Problem.from_csr(p.row_ptr, p.col_idx, p.l)
    mu0, _ = prob.start_values()
    s = gpu.Sampler(prob, mu0, seed=9, n_chains=n_chains, gibbs_iter=S, trace_len=S)
    s.run(S)
    genes = [[0, 1, T - 1, T], [3], list(range(4, T - 1)) + [T + 1, T + 2, T + 3]]
    desc = dict(virtual_id=VID, virtual_scale=VSCALE, identical=[[5, 6]], genes=genes)
    return prob, s, desc


def _groups_of(full, gs):
    """full [..., member, S] -> the sums over the member lists gs, members added in the given order"""
    out = np.zeros(full.shape[:-2] + (len(gs), full.shape[-1]))
    for g, ms in enumerate(gs):
        for m in ms:
            out[..., g, :] += full[..., m, :]
    return out


def _proportions_of(full, t_gene, genes):
    gene_of = np.full(full.shape[-2], -1)
    for g, ms in enumerate(genes):
        gene_of[ms] = g
    with np.errstate(invalid="ignore", divide="ignore"):
        prop = np.where((gene_of >= 0)[:, None], full / t_gene[..., gene_of, :], np.nan)
    return prop, np.array([g >= 0 and len(genes[g]) > 1 for g in gene_of]), gene_of < 0


@pytest.mark.parametrize("S", [16384, 12000])
def test_summary_walks(gpu, orc, S):
    """gpu.Summary at trace_len 16384 and 12000 (no power of two: Sokal returns 201 early, then the next series; percentile positions
    0, S - 1 and S): k_series_summary<0, true> over the 9 transcripts, the 4 isoforms without hits, the identical set and the 3 genes,
    k_series_summary<0, false> over the proportions"""
    T = 9
    prob, s, desc = _tiny(gpu, orc, T, 1, S, 12)
    pidx = [0, S // 2, S - 1, S]

    def run(v):
        q = gpu.Summary(s, percentile_index=pidx, **desc)
        _launch_is(gpu, "series", v, len(VID))                   # the last launch: the proportions of the isoforms without hits
        out = {}
        for kind in range(4):
            out.update({"%s %d" % (k, kind): a for k, a in q.series(kind).items()})
        for kind in range(2):
            out.update({"prop %s %d" % (k, kind): a for k, a in q.proportions(kind).items()})
        q.close()
        return out

    walks = _walks(gpu, run)
    _same_bits(walks, sorted(walks[None]))
    got = walks[2]
    trace = s.trace(0)
    V = np.stack([orc.simu_gamma_trace(9, int(VID[v]), 0.1, VSCALE[v], S) for v in range(len(VID))])
    full = np.concatenate([trace, V])
    t_gene, t_ident = _groups_of(full, desc["genes"]), _groups_of(full, desc["identical"])
    for kind, tr in enumerate((trace, V, t_ident, t_gene)):
        r = {k: got["%s %d" % (k, kind)] for k in LOG_COLS}
        check_log_series(r, tr, pidx, orc, range(tr.shape[0]))
        assert np.isnan(r["percentiles"][:, 3]).all() and np.isfinite(r["percentiles"][:, :3]).all()
    prop, multi, outside = _proportions_of(full, t_gene, desc["genes"])
    assert outside[2] and not outside[[1, 3]].any() and not multi[3] and multi[4]
    for kind, sl in enumerate((slice(0, T), slice(T, None))):
        r = {k: got["prop %s %d" % (k, kind)] for k in PROP_COLS}
        check_proportions(gpu, r, prop[sl], multi[sl], pidx)
        out = outside[sl]
        assert np.isnan(r["mean"][out]).all() and np.isnan(r["percentiles"][out]).all() and np.isfinite(r["mean"][~out]).all()
    s.close(); prob.close()


def test_pooled_summary_walks(gpu, orc):
    """gpu.PooledSummary, 3 chains of 4096 samples (C S = 12288; the chains' columns stay in LDS): k_pooled_summary<0, true> over the
    four kinds and k_pooled_summary<0, false>, whose cm / cv / ct scratch a workgroup rewrites for every series it walks"""
    T, C_, S = 12, 3, 4096
    prob, s, desc = _tiny(gpu, orc, T, C_, S, 13)
    N = C_ * S
    pidx = [0, N - 1, -1, N, N // 2]
    bytes_of = {}

    def run(v):
        ps = gpu.PooledSummary(s, percentile_index=pidx, **desc)
        _launch_is(gpu, "pooled", v, len(VID))                   # the last launch: the proportions of the isoforms without hits
        bytes_of[v] = ps.device_bytes()
        out = {}
        for kind in range(4):
            out.update({"%s %d" % (k, kind): a for k, a in ps.series(kind).items()})
        for kind in range(2):
            out.update({"prop %s %d" % (k, kind): a for k, a in ps.proportions(kind).items()})
        ps.close()
        return out

    walks = _walks(gpu, run)
    _same_bits(walks, sorted(walks[None]))
    assert len(set(bytes_of.values())) == 1                      # include/mmgibbs.h: the workspaces keep their size under the option
    got = walks[2]
    full = np.stack([np.concatenate([s.trace(c), np.stack([orc.simu_gamma_trace_keyed(9, c, orc.TAG_SIMU, int(VID[v]), 0.1, VSCALE[v], S)
                                                           for v in range(len(VID))])]) for c in range(C_)])        # [C, T + nv, S]
    t_gene = _groups_of(full, desc["genes"])
    for kind, tr in enumerate((full[:, :T], full[:, T:], _groups_of(full, desc["identical"]), t_gene)):
        r = {k: got["%s %d" % (k, kind)] for k in COLS}
        _same(r, PR.pooled_of_traces(tr.transpose(0, 2, 1), pidx, log=_dlog(gpu)), COLS, "kind %d" % kind)
    prop, multi, outside = _proportions_of(full, t_gene, desc["genes"])
    assert outside[2] and not outside[[1, 3]].any() and not multi[3] and multi[4]
    for kind, sl in enumerate((slice(0, T), slice(T, None))):
        r = {k: got["prop %s %d" % (k, kind)] for k in PROP_COLS}
        pr, mu, out = prop[:, sl].transpose(0, 2, 1), multi[sl], outside[sl]
        _same(r, PR.pooled_proportions(pr, mu, pidx), ("mean", "percentiles"), "proportions, kind %d" % kind)
        exact = PR.pooled_proportions(pr, mu, pidx, probit=lambda p: probit_as241(p, _dlog(gpu)))
        assert np.array_equal(r["probit_mean"][mu], exact["probit_mean"][mu]) and np.array_equal(r["probit_sd"][mu], exact["probit_sd"][mu])
        assert np.isinf(r["probit_mean"][~mu]).all() and (r["probit_mean"][~mu] > 0).all() and np.isnan(r["probit_sd"][~mu]).all()
        assert np.isnan(r["mean"][out]).all() and np.isnan(r["percentiles"][out]).all() and np.isfinite(r["mean"][~out]).all()
    s.close(); prob.close()


# ------------------------------------------------------------------------------------------ mmcollapse's output stage
def test_collapse_summarize_walks(gpu, orc):
    """collapse.summarize at S = 16384: 7 output series, neighbours 60 orders of magnitude apart"""
    from mmseq_amd.collapse import summarize
    S = 16384
    rng = np.random.default_rng(5)
    trace = rng.gamma(2.0, 1.0, (S, 9)) * _scales(9)
    trace[:, 2] = np.exp(_ar1(rng, 1, S, 1, 0.9)[0, :, 0]) * 1e-30
    groups = [[0], [1], [2], [3], [4], [5], [6, 8]]

    def run(v):
        lm, var, tau, rc = summarize(trace, groups)
        _launch_is(gpu, "series", v, 7)
        return dict(log_mean=lm, var=var, tau=tau, rc=rc)

    walks = _walks(gpu, run)
    _same_bits(walks, ("log_mean", "var", "tau", "rc"))
    tr = _groups_of(np.ascontiguousarray(trace.T), groups)
    check_log_series(dict(walks[2], percentiles=np.empty((7, 0))), tr, [], orc, range(7))
    assert walks[2]["tau"][2] > 4 * walks[2]["tau"][4]            # the correlated series between independent ones


# ------------------------------------------------------------------------------------------ contrasts
@pytest.mark.parametrize("S", [16384, 12000])
def test_contrast_walks(gpu, orc, S):
    """Contrast.from_traces: 7 contrasts; numerators 60 orders of magnitude apart from one contrast to the next; contrast 2 is a
    series of zeros (Sokal divides by 0: NaNs left in the transform buffers for contrast 4); 12000: rc 201"""
    from mmseq_amd import Contrast
    rng = np.random.default_rng(S)
    tr = np.exp(rng.normal(0.0, 3.0, (9, S)))
    tr[[0, 4, 6]] *= 1e30
    tr[[2, 5, 7]] *= 1e-30
    cs = [([0], [1]), ([2, 5], [1]), ([8], [8]), ([4], [3]), ([5], [0, 5]), ([6], [1]), ([7, 2], [3])]
    pidx = [0, S // 2, S - 1, S]

    def run(v):
        with Contrast.from_traces(tr, cs, pidx) as h:
            _launch_is(gpu, "contrast", v, 7)
            return h.summary()

    walks = _walks(gpu, run)
    _same_bits(walks, sorted(walks[None]))
    got = walks[2]
    ref = CR.contrast_ref(tr, cs, pidx, log=_dlog(gpu))
    assert not ref["R"][2].any() and np.abs(np.diff(ref["R"].mean(axis=1)[[0, 1, 3, 4, 5, 6]])).min() > 130.0      # (60 ln 10 = 138)
    _check_summary(got, ref, S, pidx, orc)
    assert np.isnan(got["percentiles"][:, 3]).all() and np.isfinite(got["percentiles"][:, :3]).all() and np.isfinite(got["log_ratio"]).all()


# ------------------------------------------------------------------------------------------ the production geometry, option unset
PROD = 1027                                                       # series: workgroups 0, 1 and 2 of 1024 take a second one
CHECKED = [0, 1, 1023, 1024, 1025, 1026]


def _rows(got, idx, keys):
    return {k: got[k][idx] for k in keys}


def test_convergence_at_the_production_geometry(gpu):
    """(C, S) = (2, 4098): PP = 16384, one slab, 1024 workgroups"""
    x = _mixed(np.random.default_rng(41), 2, 4098, PROD)
    got = gpu.convergence_of_traces(x)
    _launch_is(gpu, "convergence", None, PROD)
    assert gpu.selftest_series_launch("convergence")[0] == WS_GROUPS
    _check(_rows(got, CHECKED, KINDS), VR.diagnostics_of_traces(x[:, :, CHECKED]), "series %s of %d" % (CHECKED, PROD))
    once = gpu.convergence_of_traces(x[:, :, 3:])                 # 1024 series: no workgroup takes a second
    _launch_is(gpu, "convergence", None, PROD - 3)
    _same(_rows(got, slice(3, None), KINDS), once, KINDS, "1027 series against 1024")


def test_pooled_at_the_production_geometry(gpu):
    """(C, S) = (2, 4098): PP = 16384, one slab, 1024 workgroups"""
    x = _positive(np.random.default_rng(42), 2, 4098, PROD)
    N = 2 * 4098
    pidx = [0, N - 1, N, N // 2]
    got = gpu.pooled_of_traces(x, pidx)
    _launch_is(gpu, "pooled", None, PROD)
    assert gpu.selftest_series_launch("pooled")[0] == WS_GROUPS
    _same(_rows(got, CHECKED, COLS), PR.pooled_of_traces(x[:, :, CHECKED], pidx, log=_dlog(gpu)), COLS, "series %s of %d" % (CHECKED, PROD))
    once = gpu.pooled_of_traces(x[:, :, 3:], pidx)
    _launch_is(gpu, "pooled", None, PROD - 3)
    _same(_rows(got, slice(3, None), COLS), once, COLS, "1027 series against 1024")


def test_contrasts_at_the_production_geometry(gpu, orc):
    """1027 single-member contrasts over 48 series of S = 16384 (the slab holds 2048): one launch of 1024 workgroups"""
    from mmseq_amd import Contrast
    S, n = 16384, 48
    rng = np.random.default_rng(43)
    tr = np.exp(rng.normal(0.0, 3.0, (n, S)))
    cs = [([i % n], [(i % n + 1 + i // n) % n]) for i in range(PROD)]
    pidx = [0, S // 2, S - 1, S]
    with Contrast.from_traces(tr, cs, pidx) as h:
        _launch_is(gpu, "contrast", None, PROD)
        got = h.summary()
    assert gpu.selftest_series_launch("contrast")[0] == WS_GROUPS
    ref = CR.contrast_ref(tr, [cs[i] for i in CHECKED], pidx, log=_dlog(gpu))
    _check_summary(_rows(got, CHECKED, sorted(got)), ref, S, pidx, orc)
    with Contrast.from_traces(tr, cs[3:], pidx) as h:
        _launch_is(gpu, "contrast", None, PROD - 3)
        once = h.summary()
    _same(_rows(got, slice(3, None), sorted(got)), once, sorted(got), "1027 contrasts against 1024")
