// post.hip -- device TU + host side of the mmg_summary_* entry points: the posterior summary of the resident Gibbs trace
// (src/mmseq.cpp:927-1008, :1110-1227, :1235-1363; src/sokal.cc:33-87).  Kernels in post_kernels.h.
#include "post_kernels.h"
#include "conv_kernels.h"
#include "contrast_kernels.h"
#include "pool_kernels.h"
#include "mmg_host.h"
#include "mmg_launch.h"

#include <atomic>
#include <cmath>
#include <memory>
#include <mutex>
#include <vector>

using namespace mmg;

struct SeriesBuf {            // results of one kind of series, on the device
    uint32_t count = 0;
    DevBuf<double> log_mean, var, tau, pct;
    DevBuf<int32_t> rc;
};
struct PropBuf {
    uint32_t count = 0;
    DevBuf<double> mean, probit_mean, probit_sd, pct;
};

// Members are destroyed in reverse declaration order: the destructor waits for `st`, then the buffers go, and the stream last.
struct mmg_summary {
    DevStream st;                  // the summary's own stream: its kernels neither wait for nor delay the chain
    int device = 0;
    uint32_t n = 0, nv = 0, ni = 0, ng = 0, np = 0, S = 0;
    // sample-major derived traces the writers stream row by row
    DevBuf<double> d_ident;      // [S][ni]
    DevBuf<double> d_gene;       // [S][ng]
    DevBuf<double> d_prop;       // [S][n], caller's numbering
    SeriesBuf ser[4];            // MMG_SERIES_TRANSCRIPT, _VIRTUAL, _IDENTICAL, _GENE
    PropBuf prop[2];             // MMG_SERIES_TRANSCRIPT, _VIRTUAL
    // the summary is built in steps (mmg_summary_begin / _advance / _finish): what the steps share
    const mmg_problem *p = nullptr;
    const double *trace = nullptr; // the chain's resident trace [S][n], device numbering
    // what keys the simulated traces (the device's copy goes at _finish; mmg_contrast_create draws the ones it needs again)
    uint64_t seed = 0;
    double alpha = 0.0;
    std::vector<uint64_t> h_vid;
    std::vector<double> h_vscale;
    uint32_t done = 0;             // samples whose derived rows exist
    // the sampler's count of mmg_sampler_extend calls and its value at _begin: an extend in between replaced the samples the rows
    // were derived from
    std::shared_ptr<const std::atomic<uint64_t>> extensions;
    uint64_t extensions_at_begin = 0;
    bool finished = false;
    std::vector<DevBuf<uint8_t>> scratch; // device buffers that live until _finish (the pointers below point into them)
    uint64_t *d_iptr = nullptr, *d_gptr = nullptr;
    uint32_t *d_imem = nullptr, *d_gmem = nullptr, *d_gene_t = nullptr, *d_gene_v = nullptr;
    uint8_t *d_multi_t = nullptr, *d_multi_v = nullptr;
    int32_t *d_pind = nullptr;
    double *d_V = nullptr, *d_propV = nullptr, *d_tw = nullptr;
    // mmg_summary_get_rows: a stream and pinned buffers of its own (the writers of a caller fetch rows while the chain runs)
    DevStream rows_st;
    std::mutex rows_mu;
    PinnedStage rows_stage;
    ~mmg_summary() { if (st) (void)hipStreamSynchronize(st.get()); }
};

// a device buffer of `bytes` (at least 8) kept in `list`; *ptr points into it
static hipError_t scratch_alloc(std::vector<DevBuf<uint8_t>> &list, void **ptr, size_t bytes)
{
    DevBuf<uint8_t> b;
    HIPE_TRY(b.alloc(bytes ? bytes : 8));
    *ptr = b.get();
    list.push_back(std::move(b));
    return hipSuccess;
}

static inline unsigned blocks_of(uint64_t n) { return (unsigned)((n + 255) / 256); }

static int check_not_extended(const mmg_summary *q)
{
    if (q->extensions && q->extensions->load() != q->extensions_at_begin)
        return fail(MMG_ERR_STATE, "the sampler was extended after mmg_summary_begin: the samples this summary was begun on no longer exist");
    return MMG_OK;
}

// The per-series summary kernel sorts and transforms in LDS up to 8192 samples (128 KB of the 160 KB a workgroup may hold); longer
// traces take the same steps in a global workspace, SERIES_WS_GROUPS workgroups striding over the series.
static constexpr uint32_t SERIES_WS_GROUPS = 1024;
static size_t series_workspace_bytes(uint32_t S)
{
    if (S <= 8192) return 0;
    return (size_t)SERIES_WS_GROUPS * 3 * next_pow2<size_t>(S) * 8;
}

// What the workspace instantiations were last launched with, by kernel (mmg_selftest_series_launch): grid << 32 | series.  Written on the
// host by the launchers below, nothing of it is on the device.
static std::atomic<uint64_t> g_series_launch[4] = {{0}, {0}, {0}, {0}};
static inline unsigned walked(int kernel, uint32_t count, uint32_t groups)
{
    const uint32_t grid = count < groups ? count : groups;
    g_series_launch[kernel].store((uint64_t)grid << 32 | count, std::memory_order_relaxed);
    return grid;
}
// Under MMG_OPT_SERIES_GROUPS the result columns of such a launch start as 0xFF bytes (NaN, return code -1): a series that no workgroup
// reached shows as that, not as what the allocator left in a fresh buffer -- which may be an earlier call's correct numbers.
template <typename T> static void unreached(T *col, size_t count, hipStream_t st)
{
    if (col && count && opt(MMG_OPT_SERIES_GROUPS) > 0) (void)hipMemsetAsync(col, 0xFF, count * sizeof(T), st);
}
extern "C" int mmg_selftest_series_launch(int kernel, uint32_t *grid, uint32_t *count)
{
    if (kernel < 0 || kernel > 3) return fail(MMG_ERR_ARG, "kernel: 0 series summary, 1 convergence, 2 pooled summary, 3 contrast summary");
    if (!grid || !count) return fail(MMG_ERR_ARG, "NULL argument");
    const uint64_t v = g_series_launch[kernel].load(std::memory_order_relaxed);
    *grid = (uint32_t)(v >> 32); *count = (uint32_t)v;
    return MMG_OK;
}

template <bool LOG_MODE>
static int launch_series(uint32_t count, uint32_t S, const double *X, uint32_t np, const int32_t *pind, const uint8_t *multi, const double *tw,
                         SeriesOut o, uint64_t *ws, hipStream_t st)
{
    if (count == 0) return MMG_OK;
#define SERIES_IN_LDS(SMAX) hipLaunchKernelGGL((k_series_summary<SMAX, LOG_MODE>), dim3(count), dim3(256), 0, st, count, S, X, np, pind, multi, tw, o, (uint64_t *)nullptr)
    if (S <= 1024) SERIES_IN_LDS(1024);
    else if (S <= 2048) SERIES_IN_LDS(2048);
    else if (S <= 4096) SERIES_IN_LDS(4096);
    else if (S <= 8192) SERIES_IN_LDS(8192);
    else {
        if (!ws) return fail(MMG_ERR_STATE, "no workspace for the summary of a long trace");
        uint32_t groups = SERIES_WS_GROUPS;   // (the workspace holds that many slices whatever the option says)
        const int og = opt(MMG_OPT_SERIES_GROUPS);
        if (og > 0 && (uint32_t)og < groups) groups = (uint32_t)og;
        for (double *col : {o.log_mean, o.var, o.tau, o.mean, o.probit_mean, o.probit_sd}) unreached(col, count, st);
        unreached(o.rc, count, st);
        unreached(o.pct, (size_t)count * np, st);
        hipLaunchKernelGGL((k_series_summary<0, LOG_MODE>), dim3(walked(0, count, groups)), dim3(256), 0, st, count, S, X, np, pind, multi, tw, o, ws);
    }
#undef SERIES_IN_LDS
    HIP_TRY(hipGetLastError());
    return MMG_OK;
}

// twiddle factors of host/numerics.hpp:fft_pow2, computed with the host's cos / sin: tw[half + j] = exp(-2 pi i j / (2 half))
static std::vector<double> twiddles(uint32_t S)
{
    std::vector<double> tw(2 * (size_t)(S ? S : 1), 0.0);
    for (uint32_t len = 2; len <= S; len <<= 1) {
        const double ang = -2.0 * M_PI / (double)len;
        const uint32_t half = len / 2;
        for (uint32_t j = 0; j < half; ++j) { tw[2 * (half + j)] = std::cos(ang * (double)j); tw[2 * (half + j) + 1] = std::sin(ang * (double)j); }
    }
    return tw;
}

// Step 1: the description is checked and uploaded, the buffers exist, the simulated traces of isoforms without hits (which do not
// depend on the chain, :971-978) are drawn.  The chain may still be running: nothing of its trace is read here.
extern "C" int mmg_summary_begin(mmg_sampler *smp, const mmg_summary_desc *d, mmg_summary **out)
{
    if (!smp || !d || !out) return fail(MMG_ERR_ARG, "NULL argument");
    SamplerView v;
    int rc = sampler_view(smp, &v);
    if (rc) return rc;
    if (!v.d_trace) return fail(MMG_ERR_STATE, "sampler was created with keep_trace == 0");
    if (d->chain < 0 || d->chain >= v.cfg.n_chains) return fail(MMG_ERR_ARG, "chain index out of range");
    const mmg_problem *p = v.p;
    const uint32_t n = p->n, S = (uint32_t)v.cfg.trace_len, nv = d->n_virtual, ni = d->n_identical, ng = d->n_genes, np = d->n_percentiles;
    if ((nv && (!d->virtual_id || !d->virtual_scale)) || (ni && (!d->identical_ptr || !d->identical_member)) ||
        (ng && (!d->gene_ptr || !d->gene_member)) || (np && !d->percentile_index))
        return fail(MMG_ERR_ARG, "summary description: missing array");
    // groups: member indices in range; gene of every transcript (a transcript in no gene gets NaN proportions)
    std::vector<uint32_t> gene_of_t(n, 0xffffffffu), gene_of_v(nv ? nv : 1, 0xffffffffu);
    std::vector<uint8_t> multi_t(n, 0), multi_v(nv ? nv : 1, 0);
    for (uint32_t g = 0; g < ng; ++g) {
        if (d->gene_ptr[g + 1] < d->gene_ptr[g]) return fail(MMG_ERR_ARG, "gene_ptr must be non-decreasing");
        const bool multi = d->gene_ptr[g + 1] - d->gene_ptr[g] > 1; // :1243 a gene with more than one transcript
        for (uint64_t j = d->gene_ptr[g]; j < d->gene_ptr[g + 1]; ++j) {
            const uint32_t m = d->gene_member[j];
            if (m >= n + nv) return fail(MMG_ERR_ARG, "gene member out of range");
            if (m < n) { gene_of_t[m] = g; multi_t[m] = multi; } else { gene_of_v[m - n] = g; multi_v[m - n] = multi; }
        }
    }
    for (uint32_t g = 0; g < ni; ++g) {
        if (d->identical_ptr[g + 1] < d->identical_ptr[g]) return fail(MMG_ERR_ARG, "identical_ptr must be non-decreasing");
        for (uint64_t j = d->identical_ptr[g]; j < d->identical_ptr[g + 1]; ++j)
            if (d->identical_member[j] >= n + nv) return fail(MMG_ERR_ARG, "identical-set member out of range");
    }
    HIP_TRY(hipSetDevice(p->device));
    std::unique_ptr<mmg_summary> q(new mmg_summary());
    q->device = p->device; q->n = n; q->nv = nv; q->ni = ni; q->ng = ng; q->np = np; q->S = S;
    q->p = p;
    q->trace = v.d_trace + (size_t)d->chain * S * n;
    q->seed = v.cfg.seed; q->alpha = v.cfg.alpha;
    q->extensions = v.extensions;
    q->extensions_at_begin = v.extensions ? v.extensions->load() : 0;
    if (nv) { q->h_vid.assign(d->virtual_id, d->virtual_id + nv); q->h_vscale.assign(d->virtual_scale, d->virtual_scale + nv); }
    HIP_TRY(q->st.create(hipStreamNonBlocking));
    hipStream_t st = q->st.get();
    auto dalloc = [&](void **ptr, size_t bytes) { return scratch_alloc(q->scratch, ptr, bytes); };
    auto upload = [&](void **dst, const void *src, size_t bytes) {
        hipError_t e = dalloc(dst, bytes);
        if (e == hipSuccess && bytes) e = hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, st);
        return e;
    };
    uint64_t *d_vid = nullptr;
    double *d_vscale = nullptr;
    HIP_TRY(upload((void **)&d_vid, d->virtual_id, (size_t)nv * 8));
    HIP_TRY(upload((void **)&d_vscale, d->virtual_scale, (size_t)nv * 8));
    HIP_TRY(upload((void **)&q->d_iptr, d->identical_ptr, ((size_t)ni + 1) * 8 * (ni ? 1 : 0)));
    HIP_TRY(upload((void **)&q->d_imem, d->identical_member, ni ? (size_t)d->identical_ptr[ni] * 4 : 0));
    HIP_TRY(upload((void **)&q->d_gptr, d->gene_ptr, ((size_t)ng + 1) * 8 * (ng ? 1 : 0)));
    HIP_TRY(upload((void **)&q->d_gmem, d->gene_member, ng ? (size_t)d->gene_ptr[ng] * 4 : 0));
    HIP_TRY(upload((void **)&q->d_gene_t, gene_of_t.data(), (size_t)n * 4));
    HIP_TRY(upload((void **)&q->d_gene_v, gene_of_v.data(), (size_t)nv * 4));
    HIP_TRY(upload((void **)&q->d_multi_t, multi_t.data(), (size_t)n));
    HIP_TRY(upload((void **)&q->d_multi_v, multi_v.data(), (size_t)nv));
    HIP_TRY(upload((void **)&q->d_pind, d->percentile_index, (size_t)np * 4));
    const std::vector<double> tw = twiddles(S);
    HIP_TRY(upload((void **)&q->d_tw, tw.data(), tw.size() * 8));
    HIP_TRY(dalloc((void **)&q->d_V, (size_t)S * nv * 8));
    HIP_TRY(dalloc((void **)&q->d_propV, (size_t)S * nv * 8));
    if (nv) hipLaunchKernelGGL(k_virtual_traces, dim3(blocks_of((uint64_t)nv * S)), dim3(256), 0, st, v.cfg.seed, 0u, (uint32_t)TAG_SIMU, v.cfg.alpha, nv, S, d_vid, d_vscale, q->d_V);
    HIP_TRY(hipGetLastError());
    HIP_TRY(q->d_ident.alloc((size_t)S * (ni ? ni : 1)));
    HIP_TRY(q->d_gene.alloc((size_t)S * (ng ? ng : 1)));
    HIP_TRY(q->d_prop.alloc((size_t)S * n));
    HIP_TRY(hipStreamSynchronize(st));   // (the host vectors of this call were sources of asynchronous copies)
    *out = q.release();
    return MMG_OK;
}

// Step 2: the derived sample rows -- sums over identical sets and genes (:927-1008), proportions (:1014-1031) -- of the samples
// [done, samples_done).  The caller vouches that the chain has finished those samples (it synchronised after iteration
// samples_done * gibbs_ss - 1 or later); iterations enqueued behind them neither are waited for nor delayed.
extern "C" int mmg_summary_advance(mmg_summary *q, int samples_done)
{
    if (!q) return fail(MMG_ERR_ARG, "NULL summary");
    if (int rc = check_not_extended(q)) return rc;
    if (q->finished) return fail(MMG_ERR_STATE, "the summary is finished");
    if (samples_done < (int)q->done || samples_done > (int)q->S) return fail(MMG_ERR_ARG, "samples_done out of range");
    if ((uint32_t)samples_done == q->done) return MMG_OK;
    HIP_TRY(hipSetDevice(q->device));
    const uint32_t s0 = q->done, c = (uint32_t)samples_done - s0, n = q->n, nv = q->nv, ni = q->ni, ng = q->ng;
    hipStream_t st = q->st.get();
    const double *tr = q->trace + (size_t)s0 * n, *V = q->d_V + (size_t)s0 * nv;
    const uint32_t *ioe = q->p->d_int_of_ext.get();
    if (ni) hipLaunchKernelGGL(k_group_sums, dim3(blocks_of((uint64_t)ni * c)), dim3(256), 0, st, ni, c, n, nv, q->d_iptr, q->d_imem, ioe, tr, V, q->d_ident.get() + (size_t)s0 * ni);
    if (ng) hipLaunchKernelGGL(k_group_sums, dim3(blocks_of((uint64_t)ng * c)), dim3(256), 0, st, ng, c, n, nv, q->d_gptr, q->d_gmem, ioe, tr, V, q->d_gene.get() + (size_t)s0 * ng);
    hipLaunchKernelGGL(k_proportions, dim3(blocks_of((uint64_t)n * c)), dim3(256), 0, st, n, c, n, tr, ioe, q->d_gene_t, ng, q->d_gene.get() + (size_t)s0 * ng, q->d_prop.get() + (size_t)s0 * n);
    if (nv) hipLaunchKernelGGL(k_proportions, dim3(blocks_of((uint64_t)nv * c)), dim3(256), 0, st, nv, c, nv, V, (const uint32_t *)nullptr, q->d_gene_v, ng, q->d_gene.get() + (size_t)s0 * ng, q->d_propV + (size_t)s0 * nv);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    q->done = (uint32_t)samples_done;
    return MMG_OK;
}

// Step 3, once every sample is in: per series the percentiles (:1110-1192), the mean of the logged trace (:1195-1227), Sokal's
// variance and autocorrelation time (:1307-1363), the proportion summaries (:1235-1305).
extern "C" int mmg_summary_finish(mmg_summary *q)
{
    if (!q) return fail(MMG_ERR_ARG, "NULL summary");
    if (int rc = check_not_extended(q)) return rc;
    if (q->finished) return MMG_OK;
    if (q->done != q->S) return fail(MMG_ERR_STATE, "mmg_summary_finish before every sample was handed to mmg_summary_advance");
    HIP_TRY(hipSetDevice(q->device));
    const uint32_t n = q->n, nv = q->nv, ni = q->ni, ng = q->ng, np = q->np, S = q->S;
    hipStream_t st = q->st.get();
    // transpose to series-major, one workgroup per series
    size_t maxcnt = n;
    for (size_t c : {(size_t)nv, (size_t)ni, (size_t)ng}) if (c > maxcnt) maxcnt = c;
    double *d_T = nullptr;
    HIP_TRY(scratch_alloc(q->scratch, (void **)&d_T, maxcnt * S * 8));
    uint64_t *d_ws = nullptr;
    if (series_workspace_bytes(S)) HIP_TRY(scratch_alloc(q->scratch, (void **)&d_ws, series_workspace_bytes(S)));
    const uint32_t counts[4] = {n, nv, ni, ng};
    const double *srcs[4] = {q->trace, q->d_V, q->d_ident.get(), q->d_gene.get()};
    for (int k = 0; k < 4; ++k) {
        SeriesBuf &b = q->ser[k];
        b.count = counts[k];
        const size_t c = counts[k] ? counts[k] : 1;
        HIP_TRY(b.log_mean.alloc(c));
        HIP_TRY(b.var.alloc(c));
        HIP_TRY(b.tau.alloc(c));
        HIP_TRY(b.rc.alloc(c));
        HIP_TRY(b.pct.alloc(c * (np ? np : 1)));
        if (!counts[k]) continue;
        launch_transpose(srcs[k], d_T, counts[k], S, k == MMG_SERIES_TRANSCRIPT ? q->p->d_int_of_ext.get() : nullptr, st);
        SeriesOut o{b.log_mean.get(), b.var.get(), b.tau.get(), b.rc.get(), b.pct.get(), nullptr, nullptr, nullptr};
        int rc = launch_series<true>(counts[k], S, d_T, np, q->d_pind, nullptr, q->d_tw, o, d_ws, st);
        if (rc) return rc;
    }
    const double *psrc[2] = {q->d_prop.get(), q->d_propV};
    const uint8_t *pmulti[2] = {q->d_multi_t, q->d_multi_v};
    for (int k = 0; k < 2; ++k) {
        PropBuf &b = q->prop[k];
        b.count = counts[k];
        const size_t c = counts[k] ? counts[k] : 1;
        HIP_TRY(b.mean.alloc(c));
        HIP_TRY(b.probit_mean.alloc(c));
        HIP_TRY(b.probit_sd.alloc(c));
        HIP_TRY(b.pct.alloc(c * (np ? np : 1)));
        if (!counts[k]) continue;
        launch_transpose(psrc[k], d_T, counts[k], S, nullptr, st); // d_prop is in the caller's numbering already
        SeriesOut o{nullptr, nullptr, nullptr, nullptr, b.pct.get(), b.mean.get(), b.probit_mean.get(), b.probit_sd.get()};
        int rc = launch_series<false>(counts[k], S, d_T, np, q->d_pind, pmulti[k], q->d_tw, o, d_ws, st);
        if (rc) return rc;
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    q->scratch.clear();   // the group tables, the virtual traces: the results no longer need them
    q->d_V = q->d_propV = nullptr;
    q->finished = true;
    return MMG_OK;
}

// The three steps at once, after the chain has run.
extern "C" int mmg_summary_create(mmg_sampler *smp, const mmg_summary_desc *d, mmg_summary **out)
{
    if (!out) return fail(MMG_ERR_ARG, "NULL argument");
    mmg_summary *q = nullptr;
    int rc = mmg_summary_begin(smp, d, &q);
    if (rc) return rc;
    rc = mmg_sampler_sync(smp);                      // every sample is final
    if (rc == MMG_OK) rc = mmg_summary_advance(q, (int)q->S);
    if (rc == MMG_OK) rc = mmg_summary_finish(q);
    if (rc) { delete q; return rc; }
    *out = q;
    return MMG_OK;
}

static int check_kind(const mmg_summary *q, int kind, int max_kind)
{
    if (!q) return fail(MMG_ERR_ARG, "NULL summary");
    if (kind < 0 || kind > max_kind) return fail(MMG_ERR_ARG, "series kind out of range");
    return MMG_OK;
}

extern "C" int mmg_summary_get(mmg_summary *q, int kind, double *log_mean, double *var, double *tau, int32_t *sokal_rc, double *percentiles)
{
    int rc = check_kind(q, kind, MMG_SERIES_GENE);
    if (rc) return rc;
    if (!q->finished) return fail(MMG_ERR_STATE, "summary columns exist after mmg_summary_finish");
    HIP_TRY(hipSetDevice(q->device));
    const SeriesBuf &b = q->ser[kind];
    const size_t c = b.count;
    if (!c) return MMG_OK;
    if (log_mean) HIP_TRY(hipMemcpy(log_mean, b.log_mean.get(), c * 8, hipMemcpyDeviceToHost));
    if (var) HIP_TRY(hipMemcpy(var, b.var.get(), c * 8, hipMemcpyDeviceToHost));
    if (tau) HIP_TRY(hipMemcpy(tau, b.tau.get(), c * 8, hipMemcpyDeviceToHost));
    if (sokal_rc) HIP_TRY(hipMemcpy(sokal_rc, b.rc.get(), c * 4, hipMemcpyDeviceToHost));
    if (percentiles && q->np) HIP_TRY(hipMemcpy(percentiles, b.pct.get(), c * q->np * 8, hipMemcpyDeviceToHost));
    return MMG_OK;
}

extern "C" int mmg_summary_get_proportions(mmg_summary *q, int kind, double *mean_prop, double *mean_probit, double *sd_probit, double *percentiles)
{
    int rc = check_kind(q, kind, MMG_SERIES_VIRTUAL);
    if (rc) return rc;
    if (!q->finished) return fail(MMG_ERR_STATE, "summary columns exist after mmg_summary_finish");
    HIP_TRY(hipSetDevice(q->device));
    const PropBuf &b = q->prop[kind];
    const size_t c = b.count;
    if (!c) return MMG_OK;
    if (mean_prop) HIP_TRY(hipMemcpy(mean_prop, b.mean.get(), c * 8, hipMemcpyDeviceToHost));
    if (mean_probit) HIP_TRY(hipMemcpy(mean_probit, b.probit_mean.get(), c * 8, hipMemcpyDeviceToHost));
    if (sd_probit) HIP_TRY(hipMemcpy(sd_probit, b.probit_sd.get(), c * 8, hipMemcpyDeviceToHost));
    if (percentiles && q->np) HIP_TRY(hipMemcpy(percentiles, b.pct.get(), c * q->np * 8, hipMemcpyDeviceToHost));
    return MMG_OK;
}

extern "C" int mmg_summary_get_rows(mmg_summary *q, int kind, int first_sample, int n_samples, double *out)
{
    if (!q || !out) return fail(MMG_ERR_ARG, "NULL argument");
    if (int rc = check_not_extended(q)) return rc;
    const double *src = nullptr;
    size_t width = 0;
    switch (kind) {
    case MMG_SERIES_TRANSCRIPT: src = q->d_prop.get(); width = q->n; break;   // proportions of gene expression, caller's numbering
    case MMG_SERIES_IDENTICAL: src = q->d_ident.get(); width = q->ni; break;
    case MMG_SERIES_GENE: src = q->d_gene.get(); width = q->ng; break;
    default: return fail(MMG_ERR_ARG, "rows exist for the proportion, identical-set and gene traces");
    }
    if (first_sample < 0 || n_samples < 0 || (int64_t)first_sample + n_samples > (int64_t)q->S) return fail(MMG_ERR_ARG, "bad sample range");
    if ((uint32_t)(first_sample + n_samples) > q->done) return fail(MMG_ERR_STATE, "rows of samples that were not yet handed to mmg_summary_advance");
    HIP_TRY(hipSetDevice(q->device));
    if (width && n_samples) {
        std::lock_guard<std::mutex> lock(q->rows_mu);
        if (!q->rows_st) HIP_TRY(q->rows_st.create(hipStreamNonBlocking));
        HIP_TRY(q->rows_stage.copy_out(out, src + (size_t)first_sample * width, (size_t)n_samples * width * 8, q->rows_st.get()));
    }
    return MMG_OK;
}

extern "C" void mmg_summary_destroy(mmg_summary *q) { delete q; }

// what contrast.hip sees of a summary (mmg_host.h)
int mmg::summary_view(mmg_summary *q, SummaryView *v)
{
    if (!q || !v) return fail(MMG_ERR_ARG, "NULL summary");
    v->p = q->p; v->device = q->device; v->n = q->n; v->nv = q->nv; v->S = q->S; v->trace = q->trace; v->finished = q->finished;
    v->seed = q->seed; v->alpha = q->alpha; v->vid = q->h_vid.data(); v->vscale = q->h_vscale.data();
    return MMG_OK;
}

std::vector<double> mmg::series_twiddles(uint32_t S) { return twiddles(S); }

// mmcollapse's output stage (src/mmcollapse.cpp:827-1107) on traces from the host, independent of any sampler: simulated traces of the
// features without one, sums over the output series (:443-481), then per series the mean of the logged trace and Sokal's var / tau
// (:923-943) -- k_virtual_traces, k_group_sums and k_series_summary, the kernels of the summary above.
extern "C" int mmg_collapse_summarize(int device, uint32_t trace_len, uint32_t n_cols, const double *trace, uint32_t n_virtual,
                                      const uint64_t *virtual_id, const double *virtual_scale, double alpha, uint64_t seed, uint32_t stream,
                                      uint32_t n_series, const uint64_t *series_ptr, const uint32_t *series_member, double *log_mean,
                                      double *var, double *tau, int32_t *sokal_rc)
{
    if ((n_cols && !trace) || (n_virtual && (!virtual_id || !virtual_scale)) || !series_ptr || (n_series && (!series_member || !log_mean || !var || !tau || !sokal_rc)))
        return fail(MMG_ERR_ARG, "NULL argument");
    if (trace_len == 0) return fail(MMG_ERR_ARG, "trace_len must be positive");
    if (stream > 0x00FFFFFFu) return fail(MMG_ERR_ARG, "stream must fit 24 bits");
    const uint64_t nm = series_ptr[n_series];
    for (uint32_t g = 0; g < n_series; ++g)
        if (series_ptr[g + 1] < series_ptr[g]) return fail(MMG_ERR_ARG, "series_ptr must be non-decreasing");
    if (series_ptr[0] != 0) return fail(MMG_ERR_ARG, "series_ptr[0] must be 0");
    for (uint64_t j = 0; j < nm; ++j)
        if (series_member[j] >= (uint64_t)n_cols + n_virtual) return fail(MMG_ERR_ARG, "series member out of range");
    int rc = require_device(device);
    if (rc) return rc;
    if (n_series == 0) return MMG_OK;
    const uint32_t S = trace_len, n = n_cols, nv = n_virtual, ng = n_series;
    std::vector<DevBuf<uint8_t>> bufs;
    auto dalloc = [&](void **p, size_t bytes) { return scratch_alloc(bufs, p, bytes); };
    auto upload = [&](void **p, const void *src, size_t bytes) {
        hipError_t e = dalloc(p, bytes);
        if (e == hipSuccess && bytes) e = hipMemcpy(*p, src, bytes, hipMemcpyHostToDevice);
        return e;
    };
    double *d_tr = nullptr, *d_vs = nullptr, *d_V = nullptr, *d_G = nullptr, *d_T = nullptr, *d_tw = nullptr;
    uint64_t *d_vid = nullptr, *d_ptr = nullptr, *d_ws = nullptr;
    uint32_t *d_mem = nullptr;
    double *d_lm = nullptr, *d_var = nullptr, *d_tau = nullptr;
    int32_t *d_rc = nullptr;
    HIP_TRY(upload((void **)&d_tr, trace, (size_t)S * n * 8));
    HIP_TRY(upload((void **)&d_vid, virtual_id, (size_t)nv * 8));
    HIP_TRY(upload((void **)&d_vs, virtual_scale, (size_t)nv * 8));
    HIP_TRY(upload((void **)&d_ptr, series_ptr, ((size_t)ng + 1) * 8));
    HIP_TRY(upload((void **)&d_mem, series_member, (size_t)nm * 4));
    const std::vector<double> tw = twiddles(S);
    HIP_TRY(upload((void **)&d_tw, tw.data(), tw.size() * 8));
    HIP_TRY(dalloc((void **)&d_V, (size_t)S * nv * 8));
    HIP_TRY(dalloc((void **)&d_G, (size_t)S * ng * 8));
    HIP_TRY(dalloc((void **)&d_T, (size_t)S * ng * 8));
    HIP_TRY(dalloc((void **)&d_lm, (size_t)ng * 8));
    HIP_TRY(dalloc((void **)&d_var, (size_t)ng * 8));
    HIP_TRY(dalloc((void **)&d_tau, (size_t)ng * 8));
    HIP_TRY(dalloc((void **)&d_rc, (size_t)ng * 4));
    if (series_workspace_bytes(S)) HIP_TRY(dalloc((void **)&d_ws, series_workspace_bytes(S)));
    hipStream_t st = nullptr;   // the null stream: the uploads above were synchronous
    if (nv) hipLaunchKernelGGL(k_virtual_traces, dim3(blocks_of((uint64_t)nv * S)), dim3(256), 0, st, seed, stream, (uint32_t)TAG_COLLAPSE_SIMU, alpha, nv, S,
                               (const uint64_t *)d_vid, (const double *)d_vs, d_V);
    hipLaunchKernelGGL(k_group_sums, dim3(blocks_of((uint64_t)ng * S)), dim3(256), 0, st, ng, S, n, nv, (const uint64_t *)d_ptr, (const uint32_t *)d_mem,
                       (const uint32_t *)nullptr, (const double *)d_tr, (const double *)d_V, d_G);
    HIP_TRY(hipGetLastError());
    launch_transpose(d_G, d_T, ng, S, nullptr, st);
    SeriesOut o{d_lm, d_var, d_tau, d_rc, nullptr, nullptr, nullptr, nullptr};
    rc = launch_series<true>(ng, S, d_T, 0, nullptr, nullptr, d_tw, o, d_ws, st);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(log_mean, d_lm, (size_t)ng * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(var, d_var, (size_t)ng * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(tau, d_tau, (size_t)ng * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(sokal_rc, d_rc, (size_t)ng * 4, hipMemcpyDeviceToHost));
    return MMG_OK;
}

// launchers of convergence.hip (mmg_launch.h)
void mmg::launch_virtual_traces(uint64_t seed, uint32_t chain, uint32_t tag, double alpha, uint32_t nv, uint32_t S, const uint64_t *id, const double *scale,
                                double *V, hipStream_t st)
{
    if (nv && S) hipLaunchKernelGGL(k_virtual_traces, dim3(blocks_of((uint64_t)nv * S)), dim3(256), 0, st, seed, chain, tag, alpha, nv, S, id, scale, V);
}

void mmg::launch_group_sums(uint32_t ng, uint32_t S, uint32_t n, uint32_t nv, const uint64_t *ptr, const uint32_t *member, const uint32_t *int_of_ext,
                            const double *trace, const double *V, double *G, hipStream_t st)
{
    if (ng && S) hipLaunchKernelGGL(k_group_sums, dim3(blocks_of((uint64_t)ng * S)), dim3(256), 0, st, ng, S, n, nv, ptr, member, int_of_ext, trace, V, G);
}

void mmg::launch_conv_slab(const double *in, uint64_t ld, uint32_t t0, uint32_t cnt, uint32_t S, uint32_t C, uint32_t c, const uint32_t *col, double *out,
                           hipStream_t st)
{
    if (cnt && S) hipLaunchKernelGGL(k_conv_slab, dim3((cnt + 31) / 32, (S + 31) / 32), dim3(256), 0, st, in, ld, t0, cnt, S, C, c, col, out);
}

void mmg::launch_convergence(uint32_t cnt, uint32_t C, uint32_t S, const double *X, double inv_log10_p, double *rhat, double *ess_bulk, double *ess_tail,
                             uint64_t *ws, uint32_t ws_groups, hipStream_t st)
{
    if (!cnt) return;
    const uint64_t cs = (uint64_t)C * S;
#define CONV_IN_LDS(SMAX) hipLaunchKernelGGL((k_convergence<SMAX>), dim3(cnt), dim3(256), 0, st, cnt, C, S, X, inv_log10_p, rhat, ess_bulk, ess_tail, (uint64_t *)nullptr)
    if (cs <= 1024) CONV_IN_LDS(1024);
    else if (cs <= 2048) CONV_IN_LDS(2048);
    else if (cs <= 4096) CONV_IN_LDS(4096);
    else if (cs <= 8192) CONV_IN_LDS(8192);
    else {
        for (double *col : {rhat, ess_bulk, ess_tail}) unreached(col, cnt, st);
        hipLaunchKernelGGL((k_convergence<0>), dim3(walked(1, cnt, ws_groups)), dim3(256), 0, st, cnt, C, S, X, inv_log10_p, rhat, ess_bulk, ess_tail, ws);
    }
#undef CONV_IN_LDS
}

// launchers of contrast.hip (mmg_launch.h)
void mmg::launch_contrast_gather(uint32_t nm, uint32_t S, uint32_t n, const uint32_t *col, const uint32_t *int_of_ext, const double *trace, uint64_t seed,
                                 double alpha, const uint64_t *vid, const double *vscale, double *M, hipStream_t st)
{
    if (nm && S) hipLaunchKernelGGL(k_contrast_gather, dim3((nm + 31) / 32, (S + 31) / 32), dim3(256), 0, st, nm, S, n, col, int_of_ext, trace, seed, alpha, vid, vscale, M);
}

void mmg::launch_contrast_series(uint32_t c0, uint32_t cnt, uint32_t S, const uint64_t *num_ptr, const uint32_t *num_slot, const uint64_t *den_ptr,
                                 const uint32_t *den_slot, const double *M, double *R, uint32_t *gt, hipStream_t st)
{
    constexpr unsigned per = CTR_BLOCK / CTR_LANES;
    if (cnt && S) hipLaunchKernelGGL(k_contrast_series, dim3((cnt + per - 1) / per), dim3(CTR_BLOCK), 0, st, c0, cnt, S, num_ptr, num_slot, den_ptr, den_slot, M, R, gt);
}

void mmg::launch_contrast_summary(uint32_t cnt, uint32_t S, const double *R, uint32_t np, const int32_t *pind, const double *tw, double *log_ratio,
                                  double *var, double *tau, int32_t *rc, double *pct, uint64_t *ws, uint32_t ws_groups, hipStream_t st)
{
    if (!cnt) return;
    ContrastOut o{log_ratio, var, tau, rc, pct};
#define CONTRAST_IN_LDS(SMAX) hipLaunchKernelGGL((k_contrast_summary<SMAX>), dim3(cnt), dim3(256), 0, st, cnt, S, R, np, pind, tw, o, (uint64_t *)nullptr)
    if (S <= 1024) CONTRAST_IN_LDS(1024);
    else if (S <= 2048) CONTRAST_IN_LDS(2048);
    else if (S <= 4096) CONTRAST_IN_LDS(4096);
    else if (S <= 8192) CONTRAST_IN_LDS(8192);
    else {
        for (double *col : {log_ratio, var, tau}) unreached(col, cnt, st);
        unreached(rc, cnt, st);
        unreached(pct, (size_t)cnt * np, st);
        hipLaunchKernelGGL((k_contrast_summary<0>), dim3(walked(3, cnt, ws_groups)), dim3(256), 0, st, cnt, S, R, np, pind, tw, o, ws);
    }
#undef CONTRAST_IN_LDS
}

// launchers of pooled.hip (mmg_launch.h)
void mmg::launch_proportions(uint32_t cnt, uint32_t S, uint32_t stride, const double *X, const uint32_t *col_of, const uint32_t *gene_of, uint32_t ng,
                             const double *G, double *P, hipStream_t st)
{
    if (cnt && S) hipLaunchKernelGGL(k_proportions, dim3(blocks_of((uint64_t)cnt * S)), dim3(256), 0, st, cnt, S, stride, X, col_of, gene_of, ng, G, P);
}

int mmg::launch_chain_columns(uint32_t count, uint32_t S, const double *X, const double *tw, double *log_mean, double *var, double *tau, int32_t *rc,
                              uint64_t *ws, hipStream_t st)
{
    SeriesOut o{log_mean, var, tau, rc, nullptr, nullptr, nullptr, nullptr};
    return launch_series<true>(count, S, X, 0, nullptr, nullptr, tw, o, ws, st);
}

size_t mmg::chain_columns_workspace_bytes(uint32_t S) { return series_workspace_bytes(S); }

void mmg::launch_pooled_summary(bool log_mode, uint32_t cnt, uint32_t C, uint32_t S, const double *X, uint32_t np, const int32_t *pind, double *cm,
                                double *cv, double *ct, const int32_t *crc, const uint8_t *multi, double *a, double *b, double *c, double *mcse2,
                                int32_t *rc, double *pct, uint64_t *ws, uint32_t ws_groups, hipStream_t st)
{
    if (!cnt) return;
    PoolOut o{a, b, c, mcse2, rc, pct};
    const uint64_t cs = (uint64_t)C * S;
#define POOLED_IN_LDS(PMAX)                                                                                                                                      \
    do {                                                                                                                                                         \
        if (log_mode) hipLaunchKernelGGL((k_pooled_summary<PMAX, true>), dim3(cnt), dim3(256), 0, st, cnt, C, S, X, np, pind, cm, cv, ct, crc, multi, o, (uint64_t *)nullptr); \
        else hipLaunchKernelGGL((k_pooled_summary<PMAX, false>), dim3(cnt), dim3(256), 0, st, cnt, C, S, X, np, pind, cm, cv, ct, crc, multi, o, (uint64_t *)nullptr);       \
    } while (0)
    if (cs <= 1024) POOLED_IN_LDS(1024);
    else if (cs <= 2048) POOLED_IN_LDS(2048);
    else if (cs <= 4096) POOLED_IN_LDS(4096);
    else if (cs <= 8192) POOLED_IN_LDS(8192);
    else {
        for (double *col : {a, b, c, mcse2}) unreached(col, cnt, st);
        unreached(rc, cnt, st);
        unreached(pct, (size_t)cnt * np, st);
        if (log_mode) hipLaunchKernelGGL((k_pooled_summary<0, true>), dim3(walked(2, cnt, ws_groups)), dim3(256), 0, st, cnt, C, S, X, np, pind, cm, cv, ct, crc, multi, o, ws);
        else hipLaunchKernelGGL((k_pooled_summary<0, false>), dim3(walked(2, cnt, ws_groups)), dim3(256), 0, st, cnt, C, S, X, np, pind, cm, cv, ct, crc, multi, o, ws);
    }
#undef POOLED_IN_LDS
}
