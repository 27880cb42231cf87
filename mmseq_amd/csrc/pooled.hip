// pooled.hip -- host side of the mmg_pooled_* entry points: the posterior summary of a series over the draws of ALL chains of a sampler
// (or of traces from the host).  Kernels in pool_kernels.h, launched from post.hip (mmg_launch.h).
//
// The series are built as convergence.hip builds them: chain by chain with the summary's kernels (post_kernels.h, unchanged), the
// simulated traces of chain c keyed (seed, chain c, TAG_SIMU, id, sample), into series-major slabs [series][chain][sample] in the
// caller's numbering.  A slab is count * C series of length S to k_series_summary<., true>: the per-chain columns are the summary's own
// bits.  k_pooled_summary then sorts the C S pooled draws and combines the chains.  The proportions of a slab of
// transcripts need, per chain, the sums of the genes those transcripts belong to: the slab's genes are numbered locally (first
// appearance), k_group_sums and k_proportions run on that local table, and the slab kernel transposes the result.
// Every device buffer exists from the start of the call to its end: mmg_pooled_device_bytes is their sum.
#include "mmg_host.h"
#include "mmg_launch.h"
#include "mmg_series.h"   // next_pow2
#include "mmg_math.h"   // (TAG_SIMU)

#include <memory>
#include <vector>

using namespace mmg;

static constexpr size_t POOL_SLAB_BYTES = 256u << 20;
static constexpr size_t POOL_WS_BYTES = 256u << 20;
static constexpr uint32_t POOL_WS_GROUPS = 1024;

// The results, on the host: the stream and the device buffers live only as long as the create call.
struct mmg_pooled {
    uint32_t C = 0, S = 0, np = 0;
    uint64_t bytes = 0;   // device memory held during the create call
    struct Series {
        uint32_t count = 0;
        std::vector<double> log_mean, var, tau, mcse2, pct;   // [count], pct [count][np]
        std::vector<int32_t> rc;
        std::vector<double> c_mean, c_var, c_tau;             // [count][C]: the chains' own columns
        std::vector<int32_t> c_rc;
    } ser[4];             // MMG_SERIES_TRANSCRIPT, _VIRTUAL, _IDENTICAL, _GENE
    struct Prop {
        uint32_t count = 0;
        std::vector<double> mean, probit_mean, probit_sd, pct;
    } prop[2];            // MMG_SERIES_TRANSCRIPT, _VIRTUAL
};

namespace {

// The scratch of one pooled run.  `bytes` adds up what was allocated.
struct PoolWork {
    uint32_t C = 0, S = 0, np = 0, cap = 0, ws_groups = 0;
    uint64_t bytes = 0;
    DevBuf<double> slab, stage_g, stage_p, cm, cv, ct, out, pct, tw;
    DevBuf<int32_t> crc, orc, pind;
    DevBuf<uint64_t> ws, ws_series, lptr;
    DevBuf<uint32_t> lmem, lgene;
    DevBuf<uint8_t> lmulti;

    template <typename T> hipError_t get(DevBuf<T> &b, size_t count)
    {
        HIPE_TRY(b.alloc(count));
        bytes += (uint64_t)count * sizeof(T);
        return hipSuccess;
    }
    static uint32_t slab_cap(uint32_t C, uint32_t S, uint32_t max_count)
    {
        const size_t per = (size_t)C * S * 8;
        size_t cap = POOL_SLAB_BYTES / per;
        if (cap < 1) cap = 1;
        if (cap > max_count) cap = max_count ? max_count : 1;
        const int o = opt(MMG_OPT_POOL_SLAB);
        if (o > 0 && (size_t)o < cap) cap = (size_t)o;
        return (uint32_t)cap;
    }
    uint64_t pooled_pow2() const
    {
        return next_pow2((uint64_t)C * S);
    }
    // need_groups: the sums of a slab of groups are staged; max_local > 0: proportions, whose slabs list at most max_local gene members
    hipError_t alloc(uint32_t c_, uint32_t s_, uint32_t max_count, uint32_t np_, const int32_t *h_pind, const std::vector<double> &h_tw, bool need_groups,
                     bool need_props, size_t max_local, hipStream_t st)
    {
        C = c_; S = s_; np = np_;
        cap = slab_cap(C, S, max_count);
        HIPE_TRY(get(slab, (size_t)cap * C * S));
        if (need_groups || need_props) HIPE_TRY(get(stage_g, (size_t)cap * S));
        if (need_props) {
            HIPE_TRY(get(stage_p, (size_t)cap * S));
            HIPE_TRY(get(lptr, (size_t)cap + 1));
            HIPE_TRY(get(lmem, max_local ? max_local : 1));
            HIPE_TRY(get(lgene, cap));
            HIPE_TRY(get(lmulti, cap));
        }
        HIPE_TRY(get(cm, (size_t)cap * C));
        HIPE_TRY(get(cv, (size_t)cap * C));
        HIPE_TRY(get(ct, (size_t)cap * C));
        HIPE_TRY(get(crc, (size_t)cap * C));
        HIPE_TRY(get(out, (size_t)4 * cap));
        HIPE_TRY(get(orc, cap));
        HIPE_TRY(get(pct, (size_t)cap * (np ? np : 1)));
        HIPE_TRY(get(pind, np ? np : 1));
        if (np) HIPE_TRY(hipMemcpyAsync(pind.get(), h_pind, (size_t)np * 4, hipMemcpyHostToDevice, st));
        HIPE_TRY(get(tw, h_tw.size()));
        HIPE_TRY(hipMemcpyAsync(tw.get(), h_tw.data(), h_tw.size() * 8, hipMemcpyHostToDevice, st));
        if (chain_columns_workspace_bytes(S)) HIPE_TRY(get(ws_series, chain_columns_workspace_bytes(S) / 8));
        if ((uint64_t)C * S > 8192) {
            const uint64_t pp = pooled_pow2();
            uint64_t g = POOL_WS_BYTES / (8 * pp);
            if (g < 1) g = 1;
            if (g > POOL_WS_GROUPS) g = POOL_WS_GROUPS;
            if (g > cap) g = cap;
            HIPE_TRY(get(ws, (size_t)pp * g));
            const int og = opt(MMG_OPT_SERIES_GROUPS);   // (fewer workgroups in the workspace of the size above)
            if (og > 0 && (uint64_t)og < g) g = (uint64_t)og;
            ws_groups = (uint32_t)g;
        }
        return hipSuccess;
    }
    void fill(const double *in, uint64_t ld, uint32_t t0, uint32_t cnt, uint32_t c, const uint32_t *col, hipStream_t st)
    {
        launch_conv_slab(in, ld, t0, cnt, S, C, c, col, slab.get(), st);
    }
    int fetch(double *dst, const double *src, size_t count, hipStream_t st)
    {
        if (dst && count) HIP_TRY(hipMemcpyAsync(dst, src, count * 8, hipMemcpyDeviceToHost, st));
        return MMG_OK;
    }
    // the log columns of the cnt series in `slab`: per chain (c_* [cnt][C], may be null) and pooled ([cnt]; any may be null)
    int run_log(uint32_t cnt, hipStream_t st, double *c_mean, double *c_var, double *c_tau, int32_t *c_rc, double *log_mean, double *var, double *tau,
                double *mcse2, int32_t *rc, double *pct_o)
    {
        int r = launch_chain_columns(cnt * C, S, slab.get(), tw.get(), cm.get(), cv.get(), ct.get(), crc.get(), ws_series.get(), st);
        if (r) return r;
        double *a = out.get(), *b = a + cap, *c = b + cap, *m2 = c + cap;
        launch_pooled_summary(true, cnt, C, S, slab.get(), np, pind.get(), cm.get(), cv.get(), ct.get(), crc.get(), nullptr, a, b, c, m2, orc.get(),
                              pct.get(), ws.get(), ws_groups, st);
        HIP_TRY(hipGetLastError());
        const size_t cc = (size_t)cnt * C;
        if ((r = fetch(c_mean, cm.get(), cc, st)) || (r = fetch(c_var, cv.get(), cc, st)) || (r = fetch(c_tau, ct.get(), cc, st))) return r;
        if (c_rc) HIP_TRY(hipMemcpyAsync(c_rc, crc.get(), cc * 4, hipMemcpyDeviceToHost, st));
        if ((r = fetch(log_mean, a, cnt, st)) || (r = fetch(var, b, cnt, st)) || (r = fetch(tau, c, cnt, st)) || (r = fetch(mcse2, m2, cnt, st))) return r;
        if (rc) HIP_TRY(hipMemcpyAsync(rc, orc.get(), (size_t)cnt * 4, hipMemcpyDeviceToHost, st));
        if (np && (r = fetch(pct_o, pct.get(), (size_t)cnt * np, st))) return r;
        HIP_TRY(hipStreamSynchronize(st));
        return MMG_OK;
    }
    // the proportion columns of the cnt series in `slab` (lmulti holds their flags)
    int run_prop(uint32_t cnt, hipStream_t st, double *mean, double *probit_mean, double *probit_sd, double *pct_o)
    {
        double *a = out.get(), *b = a + cap, *c = b + cap;
        launch_pooled_summary(false, cnt, C, S, slab.get(), np, pind.get(), cm.get(), cv.get(), ct.get(), nullptr, lmulti.get(), a, b, c, nullptr, nullptr,
                              pct.get(), ws.get(), ws_groups, st);
        HIP_TRY(hipGetLastError());
        int r;
        if ((r = fetch(mean, a, cnt, st)) || (r = fetch(probit_mean, b, cnt, st)) || (r = fetch(probit_sd, c, cnt, st))) return r;
        if (np && (r = fetch(pct_o, pct.get(), (size_t)cnt * np, st))) return r;
        HIP_TRY(hipStreamSynchronize(st));
        return MMG_OK;
    }
};

// the genes of the items [t0, t0 + cnt), numbered by first appearance: their member lists, and per item its local gene (or 0xffffffff)
struct LocalGenes {
    std::vector<uint64_t> ptr;
    std::vector<uint32_t> mem, gene;
    void build(const uint32_t *gene_of, uint32_t t0, uint32_t cnt, const uint64_t *gptr, const uint32_t *gmem, std::vector<uint32_t> &local_of,
               bool members)
    {
        ptr.assign(1, 0); mem.clear(); gene.assign(cnt, 0xffffffffu);
        std::vector<uint32_t> seen;
        for (uint32_t i = 0; i < cnt; ++i) {
            const uint32_t g = gene_of[t0 + i];
            if (g == 0xffffffffu) continue;
            if (local_of[g] == 0xffffffffu) {
                local_of[g] = (uint32_t)ptr.size() - 1;
                seen.push_back(g);
                if (members) mem.insert(mem.end(), gmem + gptr[g], gmem + gptr[g + 1]);
                ptr.push_back(ptr.back() + (gptr[g + 1] - gptr[g]));
            }
            gene[i] = local_of[g];
        }
        for (uint32_t g : seen) local_of[g] = 0xffffffffu;
    }
};

int check_groups(uint32_t ng, const uint64_t *ptr, const uint32_t *mem, uint64_t limit, const char *what)
{
    if (!ng) return MMG_OK;
    if (ptr[0] != 0) return fail(MMG_ERR_ARG, std::string(what) + "_ptr[0] must be 0");
    for (uint32_t g = 0; g < ng; ++g) {
        if (ptr[g + 1] < ptr[g]) return fail(MMG_ERR_ARG, std::string(what) + "_ptr must be non-decreasing");
        for (uint64_t j = ptr[g]; j < ptr[g + 1]; ++j)
            if (mem[j] >= limit) return fail(MMG_ERR_ARG, std::string(what) + " member out of range");
    }
    return MMG_OK;
}

} // namespace

extern "C" int mmg_pooled_create(mmg_sampler *smp, const mmg_summary_desc *d, mmg_pooled **out)
{
    if (!smp || !out) return fail(MMG_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (!d) return fail(MMG_ERR_ARG, "NULL summary description");
    SamplerView v;
    int rc = sampler_view(smp, &v);
    if (rc) return rc;
    if (!v.d_trace) return fail(MMG_ERR_ARG, "the pooled summary needs the chains' traces: the sampler was created with keep_trace == 0");
    const mmg_problem *p = v.p;
    const uint32_t n = p->n, C = (uint32_t)v.cfg.n_chains, S = (uint32_t)v.cfg.trace_len, nv = d->n_virtual, ni = d->n_identical, ng = d->n_genes,
                   np = d->n_percentiles;
    if (C < 1 || S < 1) return fail(MMG_ERR_ARG, "the pooled summary needs at least one chain and one kept sample");
    if ((uint64_t)C * S > (1ull << 30)) return fail(MMG_ERR_ARG, "n_chains * trace_len must not exceed 2^30");
    if ((nv && (!d->virtual_id || !d->virtual_scale)) || (ni && (!d->identical_ptr || !d->identical_member)) || (ng && (!d->gene_ptr || !d->gene_member)) ||
        (np && !d->percentile_index))
        return fail(MMG_ERR_ARG, "summary description: missing array");
    rc = check_groups(ni, d->identical_ptr, d->identical_member, (uint64_t)n + nv, "identical");
    if (!rc) rc = check_groups(ng, d->gene_ptr, d->gene_member, (uint64_t)n + nv, "gene");
    if (rc) return rc;
    // the gene of every transcript and isoform without hits (the last gene that lists it, as mmg_summary_begin), and whether it has company
    std::vector<uint32_t> gene_of[2] = {std::vector<uint32_t>(n, 0xffffffffu), std::vector<uint32_t>(nv, 0xffffffffu)};
    std::vector<uint8_t> multi[2] = {std::vector<uint8_t>(n, 0), std::vector<uint8_t>(nv, 0)};
    for (uint32_t g = 0; g < ng; ++g) {
        const bool mm = d->gene_ptr[g + 1] - d->gene_ptr[g] > 1;
        for (uint64_t j = d->gene_ptr[g]; j < d->gene_ptr[g + 1]; ++j) {
            const uint32_t m = d->gene_member[j];
            if (m < n) { gene_of[0][m] = g; multi[0][m] = mm; } else { gene_of[1][m - n] = g; multi[1][m - n] = mm; }
        }
    }
    const uint32_t counts[4] = {n, nv, ni, ng};
    uint32_t maxcnt = 0;
    for (int k = 0; k < 4; ++k) if (counts[k] > maxcnt) maxcnt = counts[k];
    // the largest local member list of a slab of transcripts or of isoforms without hits
    const uint32_t cap = PoolWork::slab_cap(C, S, maxcnt);
    std::vector<uint32_t> local_of(ng, 0xffffffffu);
    LocalGenes lg;
    size_t max_local = 0;
    for (int k = 0; k < 2; ++k)
        for (uint32_t t0 = 0; t0 < counts[k]; t0 += cap) {
            lg.build(gene_of[k].data(), t0, counts[k] - t0 < cap ? counts[k] - t0 : cap, d->gene_ptr, d->gene_member, local_of, false);
            if (lg.ptr.back() > max_local) max_local = (size_t)lg.ptr.back();
        }
    const std::vector<double> h_tw = series_twiddles(S);
    rc = mmg_sampler_sync(smp);   // every sample of every chain is final; nothing of the sampler is touched below
    if (rc) return rc;
    HIP_TRY(hipSetDevice(p->device));
    std::unique_ptr<mmg_pooled> h(new mmg_pooled());
    h->C = C; h->S = S; h->np = np;
    for (int k = 0; k < 4; ++k) {
        mmg_pooled::Series &s = h->ser[k];
        const size_t c = counts[k];
        s.count = counts[k];
        s.log_mean.resize(c); s.var.resize(c); s.tau.resize(c); s.mcse2.resize(c); s.rc.resize(c); s.pct.resize(c * np);
        s.c_mean.resize(c * C); s.c_var.resize(c * C); s.c_tau.resize(c * C); s.c_rc.resize(c * C);
    }
    for (int k = 0; k < 2; ++k) {
        mmg_pooled::Prop &q = h->prop[k];
        const size_t c = counts[k];
        q.count = counts[k];
        q.mean.resize(c); q.probit_mean.resize(c); q.probit_sd.resize(c); q.pct.resize(c * np);
    }
    // (the host vectors above outlive everything below: the stream goes after the buffers, and hipFree waits for the device)
    DevStream sth;
    HIP_TRY(sth.create(hipStreamNonBlocking));
    hipStream_t st = sth.get();
    PoolWork w;
    DevBuf<uint64_t> d_vid, d_iptr, d_gptr;
    DevBuf<double> d_vscale, d_V;
    DevBuf<uint32_t> d_imem, d_gmem;
    auto upload = [&](auto &buf, const auto *src, size_t count) -> hipError_t {
        HIPE_TRY(w.get(buf, count ? count : 1));
        if (count) HIPE_TRY(hipMemcpyAsync(buf.get(), src, count * sizeof(*src), hipMemcpyHostToDevice, st));
        return hipSuccess;
    };
    HIP_TRY(upload(d_vid, d->virtual_id, nv));
    HIP_TRY(upload(d_vscale, d->virtual_scale, nv));
    HIP_TRY(upload(d_iptr, d->identical_ptr, ni ? (size_t)ni + 1 : 0));
    HIP_TRY(upload(d_imem, d->identical_member, ni ? (size_t)d->identical_ptr[ni] : 0));
    HIP_TRY(upload(d_gptr, d->gene_ptr, ng ? (size_t)ng + 1 : 0));
    HIP_TRY(upload(d_gmem, d->gene_member, ng ? (size_t)d->gene_ptr[ng] : 0));
    HIP_TRY(w.get(d_V, (size_t)C * S * (nv ? nv : 1)));
    for (uint32_t c = 0; c < C && nv; ++c)
        launch_virtual_traces(v.cfg.seed, c, (uint32_t)TAG_SIMU, v.cfg.alpha, nv, S, d_vid.get(), d_vscale.get(), d_V.get() + (size_t)c * S * nv, st);
    HIP_TRY(hipGetLastError());
    HIP_TRY(w.alloc(C, S, maxcnt, np, d->percentile_index, h_tw, ni || ng, true, max_local, st));
    h->bytes = w.bytes;
    const uint32_t *ioe = p->d_int_of_ext.get();
    auto trace_of = [&](uint32_t c) { return v.d_trace + (size_t)c * S * n; };
    auto V_of = [&](uint32_t c) { return (const double *)d_V.get() + (size_t)c * S * nv; };
    // ---- the log columns of every kind
    const uint64_t *gptrs[4] = {nullptr, nullptr, d_iptr.get(), d_gptr.get()};
    const uint32_t *gmems[4] = {nullptr, nullptr, d_imem.get(), d_gmem.get()};
    for (int k = 0; k < 4; ++k) {
        mmg_pooled::Series &s = h->ser[k];
        for (uint32_t t0 = 0; t0 < counts[k]; t0 += w.cap) {
            const uint32_t cnt = counts[k] - t0 < w.cap ? counts[k] - t0 : w.cap;
            for (uint32_t c = 0; c < C; ++c) {
                if (k == MMG_SERIES_TRANSCRIPT) w.fill(trace_of(c), n, t0, cnt, c, ioe, st);
                else if (k == MMG_SERIES_VIRTUAL) w.fill(V_of(c), nv, t0, cnt, c, nullptr, st);
                else {
                    launch_group_sums(cnt, S, n, nv, gptrs[k] + t0, gmems[k], ioe, trace_of(c), V_of(c), w.stage_g.get(), st);
                    w.fill(w.stage_g.get(), cnt, 0, cnt, c, nullptr, st);
                }
            }
            HIP_TRY(hipGetLastError());
            rc = w.run_log(cnt, st, s.c_mean.data() + (size_t)t0 * C, s.c_var.data() + (size_t)t0 * C, s.c_tau.data() + (size_t)t0 * C,
                           s.c_rc.data() + (size_t)t0 * C, s.log_mean.data() + t0, s.var.data() + t0, s.tau.data() + t0, s.mcse2.data() + t0,
                           s.rc.data() + t0, s.pct.data() + (size_t)t0 * np);
            if (rc) return rc;
        }
    }
    // ---- the proportions of the transcripts and of the isoforms without hits
    for (int k = 0; k < 2; ++k) {
        mmg_pooled::Prop &q = h->prop[k];
        for (uint32_t t0 = 0; t0 < counts[k]; t0 += w.cap) {
            const uint32_t cnt = counts[k] - t0 < w.cap ? counts[k] - t0 : w.cap;
            lg.build(gene_of[k].data(), t0, cnt, d->gene_ptr, d->gene_member, local_of, true);
            const uint32_t ngl = (uint32_t)lg.ptr.size() - 1;
            HIP_TRY(hipMemcpyAsync(w.lptr.get(), lg.ptr.data(), lg.ptr.size() * 8, hipMemcpyHostToDevice, st));
            if (!lg.mem.empty()) HIP_TRY(hipMemcpyAsync(w.lmem.get(), lg.mem.data(), lg.mem.size() * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(w.lgene.get(), lg.gene.data(), (size_t)cnt * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(w.lmulti.get(), multi[k].data() + t0, cnt, hipMemcpyHostToDevice, st));
            for (uint32_t c = 0; c < C; ++c) {
                launch_group_sums(ngl, S, n, nv, w.lptr.get(), w.lmem.get(), ioe, trace_of(c), V_of(c), w.stage_g.get(), st);
                if (k == MMG_SERIES_TRANSCRIPT)   // (without a renumbering the columns are the caller's: the slab starts at column t0)
                    launch_proportions(cnt, S, n, ioe ? trace_of(c) : trace_of(c) + t0, ioe ? ioe + t0 : nullptr, w.lgene.get(), ngl, w.stage_g.get(),
                                       w.stage_p.get(), st);
                else launch_proportions(cnt, S, nv, V_of(c) + t0, nullptr, w.lgene.get(), ngl, w.stage_g.get(), w.stage_p.get(), st);
                w.fill(w.stage_p.get(), cnt, 0, cnt, c, nullptr, st);
            }
            HIP_TRY(hipGetLastError());
            rc = w.run_prop(cnt, st, q.mean.data() + t0, q.probit_mean.data() + t0, q.probit_sd.data() + t0, q.pct.data() + (size_t)t0 * np);
            if (rc) return rc;   // (run_prop synchronised: lg may be rebuilt)
        }
    }
    *out = h.release();
    return MMG_OK;
}

static int pooled_kind(const mmg_pooled *h, int kind, int max_kind)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL pooled handle");
    if (kind < MMG_SERIES_TRANSCRIPT || kind > max_kind) return fail(MMG_ERR_ARG, "series kind out of range");
    return MMG_OK;
}
template <typename T> static void copy_out(T *dst, const std::vector<T> &src)
{
    if (dst && !src.empty()) std::memcpy(dst, src.data(), src.size() * sizeof(T));
}

extern "C" int mmg_pooled_get(mmg_pooled *h, int kind, double *log_mean, double *var, double *tau, double *mcse2, int32_t *rc, double *percentiles)
{
    int r = pooled_kind(h, kind, MMG_SERIES_GENE);
    if (r) return r;
    const mmg_pooled::Series &s = h->ser[kind];
    copy_out(log_mean, s.log_mean); copy_out(var, s.var); copy_out(tau, s.tau); copy_out(mcse2, s.mcse2); copy_out(rc, s.rc); copy_out(percentiles, s.pct);
    return MMG_OK;
}

extern "C" int mmg_pooled_get_chain(mmg_pooled *h, int kind, int chain, double *log_mean, double *var, double *tau, int32_t *rc)
{
    int r = pooled_kind(h, kind, MMG_SERIES_GENE);
    if (r) return r;
    if (chain < 0 || (uint32_t)chain >= h->C) return fail(MMG_ERR_ARG, "chain index out of range");
    const mmg_pooled::Series &s = h->ser[kind];
    for (size_t i = 0; i < s.count; ++i) {
        const size_t j = i * h->C + (uint32_t)chain;
        if (log_mean) log_mean[i] = s.c_mean[j];
        if (var) var[i] = s.c_var[j];
        if (tau) tau[i] = s.c_tau[j];
        if (rc) rc[i] = s.c_rc[j];
    }
    return MMG_OK;
}

extern "C" int mmg_pooled_get_proportions(mmg_pooled *h, int kind, double *mean_prop, double *mean_probit, double *sd_probit, double *percentiles)
{
    int r = pooled_kind(h, kind, MMG_SERIES_VIRTUAL);
    if (r) return r;
    const mmg_pooled::Prop &q = h->prop[kind];
    copy_out(mean_prop, q.mean); copy_out(mean_probit, q.probit_mean); copy_out(sd_probit, q.probit_sd); copy_out(percentiles, q.pct);
    return MMG_OK;
}

extern "C" int mmg_pooled_device_bytes(mmg_pooled *h, uint64_t *bytes)
{
    if (!h || !bytes) return fail(MMG_ERR_ARG, "NULL argument");
    *bytes = h->bytes;
    return MMG_OK;
}

extern "C" void mmg_pooled_destroy(mmg_pooled *h) { delete h; }

extern "C" int mmg_pooled_of_traces(int device, uint32_t n_chains, uint32_t S, uint32_t count, const double *traces, uint32_t np, const int32_t *pind,
                                    double *log_mean, double *var, double *tau, double *mcse2, int32_t *rc_o, double *percentiles)
{
    if (n_chains < 1) return fail(MMG_ERR_ARG, "n_chains must be positive");
    if (S < 1) return fail(MMG_ERR_ARG, "S must be positive");
    if ((count && !traces) || (np && !pind)) return fail(MMG_ERR_ARG, "NULL argument");
    if ((uint64_t)n_chains * S > (1ull << 30)) return fail(MMG_ERR_ARG, "n_chains * S must not exceed 2^30");
    int rc = require_device(device);
    if (rc) return rc;
    if (count == 0) return MMG_OK;
    const std::vector<double> h_tw = series_twiddles(S);
    DevStream sth;
    HIP_TRY(sth.create(hipStreamNonBlocking));
    hipStream_t st = sth.get();
    PoolWork w;
    DevBuf<double> d_tr;
    const size_t total = (size_t)n_chains * S * count;
    HIP_TRY(w.get(d_tr, total));
    HIP_TRY(hipMemcpyAsync(d_tr.get(), traces, total * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(w.alloc(n_chains, S, count, np, pind, h_tw, false, false, 0, st));
    for (uint32_t t0 = 0; t0 < count; t0 += w.cap) {
        const uint32_t cnt = count - t0 < w.cap ? count - t0 : w.cap;
        for (uint32_t c = 0; c < n_chains; ++c) w.fill(d_tr.get() + (size_t)c * S * count, count, t0, cnt, c, nullptr, st);
        HIP_TRY(hipGetLastError());
        rc = w.run_log(cnt, st, nullptr, nullptr, nullptr, nullptr, log_mean ? log_mean + t0 : nullptr, var ? var + t0 : nullptr, tau ? tau + t0 : nullptr,
                       mcse2 ? mcse2 + t0 : nullptr, rc_o ? rc_o + t0 : nullptr, percentiles ? percentiles + (size_t)t0 * np : nullptr);
        if (rc) { (void)hipStreamSynchronize(st); return rc; }
    }
    return MMG_OK;
}
