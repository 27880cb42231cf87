// convergence.hip -- host side of the mmg_convergence_* entry points: per series the rank-normalized split R-hat and the bulk
// and tail effective sample sizes across the chains of a sampler (or of traces from the host).  Kernels in conv_kernels.h, launched from post.hip (mmg_launch.h).
//
// The series of every kind are built chain by chain with the summary's kernels (post_kernels.h, unchanged): the transcripts straight
// from the sampler's resident trace, the isoforms without hits from k_virtual_traces keyed (seed, chain c, TAG_SIMU, id, sample), the
// identical sets and genes from k_group_sums over chain c's trace and simulated traces.  They reach the diagnostic kernel series-major,
// [series][chain][sample] in the caller's numbering, a slab of series at a time, so scratch memory is bounded:
//   slab      <= CONV_SLAB_BYTES (or one series, if a single series is larger), and S / C of that again for the group sums of a slab;
//   workspace <= max(CONV_WS_BYTES, 16 PP) when C S > 8192 (PP = the pooled draws rounded up to a power of two);
//   the simulated traces of every chain, C S n_virtual doubles (the group sums of any slab may read any of them).
#include "mmg_host.h"
#include "mmg_launch.h"
#include "mmg_series.h"   // next_pow2
#include "mmg_math.h"   // (TAG_SIMU)

#include <cmath>
#include <memory>
#include <vector>

using namespace mmg;

static constexpr size_t CONV_SLAB_BYTES = 256u << 20;
static constexpr size_t CONV_WS_BYTES = 256u << 20;
static constexpr uint32_t CONV_WS_GROUPS = 1024;

// The results, on the host: the stream and the device buffers live only as long as the create call.
struct mmg_convergence {
    int device = 0;
    uint32_t C = 0, S = 0;
    std::vector<double> rhat[4], ess_bulk[4], ess_tail[4];   // MMG_SERIES_TRANSCRIPT, _VIRTUAL, _IDENTICAL, _GENE
};

namespace {

// The scratch of one diagnostic run: a slab of series-major series, the group sums of a slab, the slab's results, the workspace.
struct ConvWork {
    uint32_t C = 0, S = 0, cap = 0, ws_groups = 0;
    DevBuf<double> slab, stage, out;
    DevBuf<uint64_t> ws;

    hipError_t alloc(uint32_t c_, uint32_t s_, uint32_t max_count, bool need_stage)
    {
        C = c_; S = s_;
        const size_t per = (size_t)C * S * 8;
        size_t cap_ = CONV_SLAB_BYTES / per;
        if (cap_ < 1) cap_ = 1;
        if (cap_ > max_count) cap_ = max_count ? max_count : 1;
        const int o = opt(MMG_OPT_CONV_SLAB);
        if (o > 0 && (size_t)o < cap_) cap_ = (size_t)o;
        cap = (uint32_t)cap_;
        HIPE_TRY(slab.alloc((size_t)cap * C * S));
        if (need_stage) HIPE_TRY(stage.alloc((size_t)cap * S));
        HIPE_TRY(out.alloc((size_t)3 * cap));
        if ((uint64_t)C * S > 8192) {
            const uint64_t pp = pooled_pow2();
            uint64_t g = CONV_WS_BYTES / (16 * pp);
            if (g < 1) g = 1;
            if (g > CONV_WS_GROUPS) g = CONV_WS_GROUPS;
            if (g > cap) g = cap;
            HIPE_TRY(ws.alloc((size_t)2 * pp * g));
            const int og = opt(MMG_OPT_SERIES_GROUPS);   // (fewer workgroups in the workspace of the size above)
            if (og > 0 && (uint64_t)og < g) g = (uint64_t)og;
            ws_groups = (uint32_t)g;
        }
        return hipSuccess;
    }
    uint64_t pooled_pow2() const
    {
        return next_pow2((uint64_t)2 * C * (S / 2));
    }
    // the diagnostic of the cnt series in `slab`; results into host rhat[t0 + i], ...
    int run(uint32_t cnt, hipStream_t st, double *rhat, double *essb, double *esst)
    {
        const double inv_log10_p = 1.0 / std::log10((double)((uint64_t)2 * C * (S / 2)));
        double *r = out.get(), *eb = r + cap, *et = eb + cap;
        launch_convergence(cnt, C, S, slab.get(), inv_log10_p, r, eb, et, ws.get(), ws_groups, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(rhat, r, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(essb, eb, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(esst, et, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return MMG_OK;
    }
    void fill(const double *in, uint64_t ld, uint32_t t0, uint32_t cnt, uint32_t c, const uint32_t *col, hipStream_t st)
    {
        launch_conv_slab(in, ld, t0, cnt, S, C, c, col, slab.get(), st);
    }
};

// count series in slabs: fill_chain(c, t0, cnt) puts chain c of the series [t0, t0 + cnt) into w.slab
template <typename Fill>
int conv_series(ConvWork &w, uint32_t count, hipStream_t st, Fill fill_chain, double *rhat, double *essb, double *esst)
{
    for (uint32_t t0 = 0; t0 < count; t0 += w.cap) {
        const uint32_t cnt = count - t0 < w.cap ? count - t0 : w.cap;
        for (uint32_t c = 0; c < w.C; ++c) fill_chain(c, t0, cnt);
        HIP_TRY(hipGetLastError());
        int rc = w.run(cnt, st, rhat + t0, essb + t0, esst + t0);
        if (rc) return rc;
    }
    return MMG_OK;
}

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

extern "C" int mmg_convergence_create(mmg_sampler *smp, const mmg_summary_desc *d, mmg_convergence **out)
{
    if (!smp || !d || !out) return fail(MMG_ERR_ARG, "NULL argument");
    *out = nullptr;
    SamplerView v;
    int rc = sampler_view(smp, &v);
    if (rc) return rc;
    if (!v.d_trace) return fail(MMG_ERR_STATE, "convergence diagnostics need the chains' traces: the sampler was created with keep_trace == 0");
    const mmg_problem *p = v.p;
    const uint32_t n = p->n, C = (uint32_t)v.cfg.n_chains, S = (uint32_t)v.cfg.trace_len, nv = d->n_virtual, ni = d->n_identical, ng = d->n_genes;
    if (S < 4) return fail(MMG_ERR_ARG, "convergence diagnostics need trace_len >= 4 (two halves of at least two draws per chain)");
    if ((uint64_t)C * S > (1ull << 30)) return fail(MMG_ERR_ARG, "n_chains * trace_len must not exceed 2^30");
    if ((nv && (!d->virtual_id || !d->virtual_scale)) || (ni && (!d->identical_ptr || !d->identical_member)) || (ng && (!d->gene_ptr || !d->gene_member)))
        return fail(MMG_ERR_ARG, "convergence description: missing array");
    rc = check_groups(ni, d->identical_ptr, d->identical_member, (uint64_t)n + nv, "identical");
    if (!rc) rc = check_groups(ng, d->gene_ptr, d->gene_member, (uint64_t)n + nv, "gene");
    if (rc) return rc;
    rc = mmg_sampler_sync(smp);   // every sample of every chain is final; nothing of the sampler is touched below
    if (rc) return rc;
    HIP_TRY(hipSetDevice(p->device));
    std::unique_ptr<mmg_convergence> h(new mmg_convergence());
    h->device = p->device; h->C = C; h->S = S;
    // (declared first, destroyed last: every buffer below is freed before its stream goes, and hipFree waits for the device)
    DevStream sth;
    HIP_TRY(sth.create(hipStreamNonBlocking));
    hipStream_t st = sth.get();
    const uint32_t counts[4] = {n, nv, ni, ng};
    uint32_t maxcnt = 0;
    for (int k = 0; k < 4; ++k) {
        h->rhat[k].resize(counts[k]); h->ess_bulk[k].resize(counts[k]); h->ess_tail[k].resize(counts[k]);
        if (counts[k] > maxcnt) maxcnt = counts[k];
    }
    // the descriptors and the simulated traces of every chain, V[c][s][v]
    DevBuf<uint64_t> d_vid, d_iptr, d_gptr;
    DevBuf<double> d_vscale, d_V;
    DevBuf<uint32_t> d_imem, d_gmem;
    auto upload = [&](auto &buf, const auto *src, size_t count) -> hipError_t {
        HIPE_TRY(buf.alloc(count ? count : 1));
        if (count) HIPE_TRY(hipMemcpyAsync(buf.get(), src, count * sizeof(*src), hipMemcpyHostToDevice, st));
        return hipSuccess;
    };
    HIP_TRY(upload(d_vid, d->virtual_id, nv));
    HIP_TRY(upload(d_vscale, d->virtual_scale, nv));
    HIP_TRY(upload(d_iptr, d->identical_ptr, ni ? (size_t)ni + 1 : 0));
    HIP_TRY(upload(d_imem, d->identical_member, ni ? (size_t)d->identical_ptr[ni] : 0));
    HIP_TRY(upload(d_gptr, d->gene_ptr, ng ? (size_t)ng + 1 : 0));
    HIP_TRY(upload(d_gmem, d->gene_member, ng ? (size_t)d->gene_ptr[ng] : 0));
    HIP_TRY(d_V.alloc((size_t)C * S * (nv ? nv : 1)));
    for (uint32_t c = 0; c < C && nv; ++c)
        launch_virtual_traces(v.cfg.seed, c, (uint32_t)TAG_SIMU, v.cfg.alpha, nv, S, d_vid.get(), d_vscale.get(), d_V.get() + (size_t)c * S * nv, st);
    HIP_TRY(hipGetLastError());
    ConvWork w;
    HIP_TRY(w.alloc(C, S, maxcnt, ni || ng));
    const uint32_t *ioe = p->d_int_of_ext.get();
    auto trace_of = [&](uint32_t c) { return v.d_trace + (size_t)c * S * n; };
    auto V_of = [&](uint32_t c) { return (const double *)d_V.get() + (size_t)c * S * nv; };
    rc = conv_series(w, n, st, [&](uint32_t c, uint32_t t0, uint32_t cnt) { w.fill(trace_of(c), n, t0, cnt, c, ioe, st); },
                     h->rhat[0].data(), h->ess_bulk[0].data(), h->ess_tail[0].data());
    if (!rc) rc = conv_series(w, nv, st, [&](uint32_t c, uint32_t t0, uint32_t cnt) { w.fill(V_of(c), nv, t0, cnt, c, nullptr, st); },
                              h->rhat[1].data(), h->ess_bulk[1].data(), h->ess_tail[1].data());
    const uint64_t *gptrs[2] = {d_iptr.get(), d_gptr.get()};
    const uint32_t *gmems[2] = {d_imem.get(), d_gmem.get()};
    for (int k = 2; k < 4 && !rc; ++k) {
        const uint64_t *ptr = gptrs[k - 2];
        const uint32_t *mem = gmems[k - 2];
        rc = conv_series(w, counts[k], st, [&](uint32_t c, uint32_t t0, uint32_t cnt) {
                launch_group_sums(cnt, S, n, nv, ptr + t0, mem, ioe, trace_of(c), V_of(c), w.stage.get(), st);
                w.fill(w.stage.get(), cnt, 0, cnt, c, nullptr, st);
            }, h->rhat[k].data(), h->ess_bulk[k].data(), h->ess_tail[k].data());
    }
    if (rc) return rc;
    *out = h.release();
    return MMG_OK;
}

extern "C" int mmg_convergence_get(mmg_convergence *h, int kind, double *rhat, double *ess_bulk, double *ess_tail)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL convergence handle");
    if (kind < MMG_SERIES_TRANSCRIPT || kind > MMG_SERIES_GENE) return fail(MMG_ERR_ARG, "series kind out of range");
    const size_t c = h->rhat[kind].size();
    if (rhat && c) std::memcpy(rhat, h->rhat[kind].data(), c * 8);
    if (ess_bulk && c) std::memcpy(ess_bulk, h->ess_bulk[kind].data(), c * 8);
    if (ess_tail && c) std::memcpy(ess_tail, h->ess_tail[kind].data(), c * 8);
    return MMG_OK;
}

extern "C" void mmg_convergence_destroy(mmg_convergence *h) { delete h; }

extern "C" int mmg_convergence_of_traces(int device, uint32_t n_chains, uint32_t S, uint32_t count, const double *traces, double *rhat,
                                         double *ess_bulk, double *ess_tail)
{
    if ((count && (!traces || !rhat || !ess_bulk || !ess_tail))) return fail(MMG_ERR_ARG, "NULL argument");
    if (n_chains < 1) return fail(MMG_ERR_ARG, "n_chains must be positive");
    if (S < 4) return fail(MMG_ERR_ARG, "convergence diagnostics need S >= 4 samples per chain (two halves of at least two draws)");
    if ((uint64_t)n_chains * S > (1ull << 30)) return fail(MMG_ERR_ARG, "n_chains * S must not exceed 2^30");
    int rc = require_device(device);
    if (rc) return rc;
    if (count == 0) return MMG_OK;
    DevStream sth;
    HIP_TRY(sth.create(hipStreamNonBlocking));
    hipStream_t st = sth.get();
    DevBuf<double> d_tr;
    const size_t total = (size_t)n_chains * S * count;
    HIP_TRY(d_tr.alloc(total));
    HIP_TRY(hipMemcpyAsync(d_tr.get(), traces, total * 8, hipMemcpyHostToDevice, st));
    ConvWork w;
    HIP_TRY(w.alloc(n_chains, S, count, false));
    rc = conv_series(w, count, st, [&](uint32_t c, uint32_t t0, uint32_t cnt) { w.fill(d_tr.get() + (size_t)c * S * count, count, t0, cnt, c, nullptr, st); },
                     rhat, ess_bulk, ess_tail);
    if (rc) { (void)hipStreamSynchronize(st); return rc; }
    HIP_TRY(hipStreamSynchronize(st));
    return MMG_OK;
}
