// contrast.hip -- host side of the mmg_contrast_* entry points: posterior log-ratios between sets of transcripts of one sample from
// the kept samples of a chain.  Kernels in contrast_kernels.h, launched from post.hip (mmg_launch.h), as those of convergence.hip are:
// post_kernels.h, which they build on, defines its plain kernels outright and so belongs to one translation unit.  Specification in
// tests/contrast_ref.py and DESIGN.md section 13.
//
// The contrasts are cut into slabs of at most CONTRAST_SLAB_BYTES of series (at least one contrast), as mmg_convergence_create cuts
// its series.  Per slab: the distinct members of its contrasts are gathered out of the chain's sample-major trace (isoforms without
// hits: drawn) into a series-major matrix, a wave per contrast walks its two lists over that matrix, and the summary kernel takes
// the slab's series one workgroup each.  From host traces the uploaded matrix is series-major already and nothing is gathered.
// MemberSource (mmg_host.h), where those members come from, is defined here; iso.hip and pairs.hip use it as well.
#include "mmg_host.h"
#include "mmg_launch.h"
#include "mmg_series.h"   // next_pow2

#include <algorithm>
#include <memory>
#include <vector>

using namespace mmg;

static constexpr size_t CONTRAST_SLAB_BYTES = 256u << 20;
static constexpr uint32_t CONTRAST_WS_GROUPS = 1024;

// Members are destroyed in reverse declaration order: the destructor waits for `st`, then the buffers go, and the stream last.
struct mmg_contrast {
    DevStream st;
    uint32_t C = 0, np = 0, cap = 0;
    uint64_t n_num = 0, n_den = 0;
    // the descriptor on the device: the lists as slots of the slab's matrix (from host traces: the members themselves)
    DevBuf<uint64_t> d_num_ptr, d_den_ptr;
    DevBuf<uint32_t> d_num_slot, d_den_slot;
    // from a sampler: the distinct members of slab k are d_cols[slab_col[k] .. slab_col[k + 1]), ascending
    DevBuf<uint32_t> d_cols;
    std::vector<uint64_t> slab_col;
    uint64_t max_cols = 0;
    MemberSource src;
    // the results
    std::vector<double> log_ratio, var, tau, p_gt, pct;
    std::vector<int32_t> rc;
    ~mmg_contrast() { if (st) (void)hipStreamSynchronize(st.get()); }
};

namespace {

size_t workspace_elems(uint32_t S, uint32_t groups)
{
    if (S <= 8192) return 0;
    return (size_t)groups * 3 * next_pow2<size_t>(S);
}

// the lists of a description: pointers, offsets, empty sides, member range, duplicates within a side -- before any device work
int check_desc(const mmg_contrast_desc *d, uint64_t limit)
{
    if (!d->num_ptr || !d->num_member || !d->den_ptr || !d->den_member || (d->n_percentiles && !d->percentile_index))
        return fail(MMG_ERR_ARG, "contrast description: NULL array");
    if (d->n_contrasts == 0) return fail(MMG_ERR_ARG, "n_contrasts must be at least 1");
    if (d->n_contrasts >= 0x7fffffffu) return fail(MMG_ERR_ARG, "too many contrasts");
    std::vector<uint32_t> seen(limit, 0xffffffffu);   // the last list (2 c + side) a member was seen in
    const uint64_t *ptrs[2] = {d->num_ptr, d->den_ptr};
    const uint32_t *mems[2] = {d->num_member, d->den_member};
    const char *side[2] = {"numerator", "denominator"};
    for (int k = 0; k < 2; ++k) {
        if (ptrs[k][0] != 0) return fail(MMG_ERR_ARG, std::string(side[k]) + " offsets must start at 0");
        for (uint32_t c = 0; c < d->n_contrasts; ++c) {
            const std::string where = " of contrast " + std::to_string(c);
            if (ptrs[k][c + 1] < ptrs[k][c]) return fail(MMG_ERR_ARG, std::string(side[k]) + " offsets must not decrease");
            if (ptrs[k][c + 1] == ptrs[k][c]) return fail(MMG_ERR_ARG, std::string("empty ") + side[k] + where);
            const uint32_t list = 2 * c + (uint32_t)k;   // (n_contrasts < 2^31: 0xffffffff is no list)
            for (uint64_t j = ptrs[k][c]; j < ptrs[k][c + 1]; ++j) {
                const uint32_t m = mems[k][j];
                if (m >= limit) return fail(MMG_ERR_ARG, std::string(side[k]) + " member out of range" + where);
                if (seen[m] == list) return fail(MMG_ERR_ARG, std::string("member ") + std::to_string(m) + " twice in the " + side[k] + where);
                seen[m] = list;
            }
        }
    }
    return MMG_OK;
}

uint32_t slab_cap(uint32_t C, uint32_t S)
{
    size_t cap = CONTRAST_SLAB_BYTES / ((size_t)(S ? S : 1) * 8);
    if (cap < 1) cap = 1;
    if (cap > C) cap = C;
    const int o = opt(MMG_OPT_CONTRAST_SLAB);
    if (o > 0 && (size_t)o < cap) cap = (size_t)o;
    return (uint32_t)cap;
}

// the series of the contrasts [c0, c0 + cnt) of slab k (all inside it) into R[cnt][S]; gt: their counts of N_s > D_s, or null
void launch_rows(const mmg_contrast *h, uint32_t k, uint32_t c0, uint32_t cnt, double *M, double *R, uint32_t *gt, hipStream_t st)
{
    const uint32_t *cols = nullptr;   // from host traces the members are the uploaded rows: no columns
    uint32_t nm = 0;
    if (!h->src.from_traces) { cols = h->d_cols.get() + h->slab_col[k]; nm = (uint32_t)(h->slab_col[k + 1] - h->slab_col[k]); }
    const double *X = h->src.rows(cols, nm, M, st);
    launch_contrast_series(c0, cnt, h->src.S, h->d_num_ptr.get(), h->d_num_slot.get(), h->d_den_ptr.get(), h->d_den_slot.get(), X, R, gt, st);
}

// The lists become slots, the descriptor goes to the device, every slab is summarised: what both create calls share.  h->src is set;
// the current device is its device.
int build(mmg_contrast *h, const mmg_contrast_desc *d)
{
    const bool from_traces = h->src.from_traces;
    const uint32_t C = d->n_contrasts, S = h->src.S, np = d->n_percentiles;
    h->C = C; h->np = np; h->cap = slab_cap(C, S);
    h->n_num = d->num_ptr[C]; h->n_den = d->den_ptr[C];
    const uint32_t cap = h->cap, n_slabs = (C + cap - 1) / cap;
    std::vector<uint32_t> num_slot(d->num_member, d->num_member + h->n_num), den_slot(d->den_member, d->den_member + h->n_den), cols;
    if (!from_traces) {
        h->slab_col.assign(1, 0);
        // a fixed number of contrasts per slab: the distinct members of their two sides
        SlabColumns sc((size_t)h->src.n + h->src.nv);
        for (uint32_t k = 0; k < n_slabs; ++k) {
            const uint32_t c0 = k * cap, c1 = std::min<uint64_t>((uint64_t)c0 + cap, C);
            for (uint64_t j = d->num_ptr[c0]; j < d->num_ptr[c1]; ++j) sc.add(d->num_member[j]);
            for (uint64_t j = d->den_ptr[c0]; j < d->den_ptr[c1]; ++j) sc.add(d->den_member[j]);
            h->max_cols = std::max<uint64_t>(h->max_cols, sc.count());
            sc.close([&](auto slot) {
                for (uint64_t j = d->num_ptr[c0]; j < d->num_ptr[c1]; ++j) num_slot[j] = slot(d->num_member[j]);
                for (uint64_t j = d->den_ptr[c0]; j < d->den_ptr[c1]; ++j) den_slot[j] = slot(d->den_member[j]);
            });
            h->slab_col.push_back(sc.cols.size());
        }
        cols = std::move(sc.cols);
    }
    HIP_TRY(h->st.create(hipStreamNonBlocking));
    hipStream_t st = h->st.get();
    HIP_TRY(upload(h->d_num_ptr, d->num_ptr, (size_t)C + 1, st));
    HIP_TRY(upload(h->d_den_ptr, d->den_ptr, (size_t)C + 1, st));
    HIP_TRY(upload(h->d_num_slot, num_slot.data(), num_slot.size(), st));
    HIP_TRY(upload(h->d_den_slot, den_slot.data(), den_slot.size(), st));
    if (!from_traces) HIP_TRY(upload(h->d_cols, cols.data(), cols.size(), st));
    // the scratch of creation: a slab of series, the gathered members, the tables, a slab's results, the workspace
    DevBuf<double> d_R, d_M, d_tw, d_res;
    DevBuf<int32_t> d_pind, d_rc;
    DevBuf<uint32_t> d_gt;
    DevBuf<uint64_t> d_ws;
    const std::vector<double> tw = series_twiddles(S);
    HIP_TRY(upload(d_tw, tw.data(), tw.size(), st));
    HIP_TRY(upload(d_pind, d->percentile_index, (size_t)np, st));
    HIP_TRY(d_R.alloc((size_t)cap * S));
    if (!from_traces) HIP_TRY(d_M.alloc((size_t)h->max_cols * S));
    HIP_TRY(d_res.alloc((size_t)cap * (3 + (np ? np : 0)) + 1));
    HIP_TRY(d_rc.alloc(cap));
    HIP_TRY(d_gt.alloc(cap));
    uint32_t ws_groups = cap < CONTRAST_WS_GROUPS ? cap : CONTRAST_WS_GROUPS;
    if (workspace_elems(S, ws_groups)) HIP_TRY(d_ws.alloc(workspace_elems(S, ws_groups)));
    const int og = opt(MMG_OPT_SERIES_GROUPS);   // (fewer workgroups in the workspace of the size above)
    if (og > 0 && (uint32_t)og < ws_groups) ws_groups = (uint32_t)og;
    h->log_ratio.resize(C); h->var.resize(C); h->tau.resize(C); h->p_gt.resize(C); h->rc.resize(C); h->pct.resize((size_t)C * np);
    std::vector<uint32_t> gt(cap);
    struct { double *log_ratio, *var, *tau; int32_t *rc; double *pct; } o{d_res.get(), d_res.get() + cap, d_res.get() + 2 * (size_t)cap, d_rc.get(),
                                                                            d_res.get() + 3 * (size_t)cap};
    for (uint32_t k = 0; k < n_slabs; ++k) {
        const uint32_t c0 = k * cap, cnt = C - c0 < cap ? C - c0 : cap;
        launch_rows(h, k, c0, cnt, d_M.get(), d_R.get(), d_gt.get(), st);
        launch_contrast_summary(cnt, S, d_R.get(), np, d_pind.get(), d_tw.get(), o.log_ratio, o.var, o.tau, o.rc, o.pct, d_ws.get(), ws_groups, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h->log_ratio.data() + c0, o.log_ratio, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h->var.data() + c0, o.var, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h->tau.data() + c0, o.tau, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h->rc.data() + c0, o.rc, (size_t)cnt * 4, hipMemcpyDeviceToHost, st));
        if (np) HIP_TRY(hipMemcpyAsync(h->pct.data() + (size_t)c0 * np, o.pct, (size_t)cnt * np * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(gt.data(), d_gt.get(), (size_t)cnt * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (uint32_t i = 0; i < cnt; ++i) h->p_gt[c0 + i] = (double)gt[i] / (double)S;
    }
    return MMG_OK;
}

} // namespace

int MemberSource::view_summary(mmg_sampler *s, mmg_summary *q, const char *not_finished)
{
    SamplerView v;
    int rc = sampler_view(s, &v);
    if (rc) return rc;
    SummaryView sv;
    rc = summary_view(q, &sv);
    if (rc) return rc;
    if (sv.p != v.p || !v.d_trace) return fail(MMG_ERR_ARG, "the summary is not one of this sampler");
    if (!sv.finished) return fail(MMG_ERR_STATE, not_finished);
    device = sv.device; S = sv.S; n = sv.n; nv = sv.nv;
    trace = sv.trace; int_of_ext = sv.p->d_int_of_ext.get(); seed = sv.seed; alpha = sv.alpha;
    h_vid_ = sv.vid; h_vscale_ = sv.vscale;
    return MMG_OK;
}

int MemberSource::acquire(mmg_sampler *s)
{
    int rc = mmg_sampler_sync(s);   // every sample is final; nothing of the sampler is touched below
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    if (nv) {
        HIP_TRY(d_vid.alloc(nv));
        HIP_TRY(d_vscale.alloc(nv));
        HIP_TRY(hipMemcpy(d_vid.get(), h_vid_, (size_t)nv * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_vscale.get(), h_vscale_, (size_t)nv * 8, hipMemcpyHostToDevice));
    }
    return MMG_OK;
}

void MemberSource::from_chain(const SamplerView &v, int chain)
{
    device = v.p->device; S = (uint32_t)v.cfg.trace_len; n = v.p->n;
    trace = v.d_trace + (uint64_t)chain * (uint64_t)v.cfg.trace_len * v.p->n;
    int_of_ext = v.p->d_int_of_ext.get();
}

int MemberSource::from_host(int device_, uint32_t S_, uint32_t n_series, const double *traces)
{
    device = device_; S = S_; n = n_series; from_traces = true;
    HIP_TRY(d_traces.alloc((size_t)n * S));
    HIP_TRY(hipMemcpy(d_traces.get(), traces, (size_t)n * S * 8, hipMemcpyHostToDevice));
    return MMG_OK;
}

const double *MemberSource::rows(const uint32_t *d_cols, uint32_t nm, double *M, hipStream_t st) const
{
    if (from_traces) return d_traces.get();
    launch_contrast_gather(nm, S, n, d_cols, int_of_ext, trace, seed, alpha, d_vid.get(), d_vscale.get(), M, st);
    return M;
}

extern "C" int mmg_contrast_create(mmg_sampler *s, mmg_summary *q, const mmg_contrast_desc *d, mmg_contrast **out)
{
    if (!s || !q || !d || !out) return fail(MMG_ERR_ARG, "NULL argument");
    *out = nullptr;
    std::unique_ptr<mmg_contrast> h(new mmg_contrast());
    int rc = h->src.view_summary(s, q, "contrasts are taken after mmg_summary_finish");
    if (rc) return rc;
    rc = check_desc(d, (uint64_t)h->src.n + h->src.nv);
    if (rc) return rc;
    rc = h->src.acquire(s);
    if (rc) return rc;
    rc = build(h.get(), d);
    if (rc) return rc;
    *out = h.release();
    return MMG_OK;
}

extern "C" int mmg_contrast_of_traces(int device, uint32_t S, uint32_t n_series, const double *traces, const mmg_contrast_desc *d, mmg_contrast **out)
{
    if (!traces || !d || !out) return fail(MMG_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (S < 1 || n_series < 1) return fail(MMG_ERR_ARG, "S and n_series must be at least 1");
    int rc = check_desc(d, n_series);
    if (rc) return rc;
    rc = require_device(device);
    if (rc) return rc;
    std::unique_ptr<mmg_contrast> h(new mmg_contrast());
    rc = h->src.from_host(device, S, n_series, traces);
    if (rc) return rc;
    rc = build(h.get(), d);
    if (rc) return rc;
    *out = h.release();
    return MMG_OK;
}

extern "C" int mmg_contrast_get(mmg_contrast *h, double *log_ratio, double *var, double *tau, int32_t *sokal_rc, double *p_gt, double *percentiles)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL contrast handle");
    const size_t c = h->C;
    if (log_ratio) std::memcpy(log_ratio, h->log_ratio.data(), c * 8);
    if (var) std::memcpy(var, h->var.data(), c * 8);
    if (tau) std::memcpy(tau, h->tau.data(), c * 8);
    if (sokal_rc) std::memcpy(sokal_rc, h->rc.data(), c * 4);
    if (p_gt) std::memcpy(p_gt, h->p_gt.data(), c * 8);
    if (percentiles && h->np) std::memcpy(percentiles, h->pct.data(), c * h->np * 8);
    return MMG_OK;
}

extern "C" int mmg_contrast_get_rows(mmg_contrast *h, uint32_t first, uint32_t count, double *R)
{
    if (!h || (count && !R)) return fail(MMG_ERR_ARG, "NULL argument");
    if (first > h->C || count > h->C - first) return fail(MMG_ERR_ARG, "contrast range out of bounds");
    if (!count) return MMG_OK;
    const uint32_t S = h->src.S;
    HIP_TRY(hipSetDevice(h->src.device));
    hipStream_t st = h->st.get();
    DevBuf<double> d_R, d_M;
    HIP_TRY(d_R.alloc((size_t)std::min(h->cap, count) * S));
    if (!h->src.from_traces) HIP_TRY(d_M.alloc((size_t)h->max_cols * S));
    for (uint32_t c = first; c < first + count;) {   // the piece of [first, first + count) in each slab it touches
        const uint32_t k = c / h->cap, end = std::min<uint64_t>((uint64_t)(k + 1) * h->cap, (uint64_t)first + count), cnt = end - c;
        launch_rows(h, k, c, cnt, d_M.get(), d_R.get(), nullptr, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(R + (size_t)(c - first) * S, d_R.get(), (size_t)cnt * S * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        c = end;
    }
    return MMG_OK;
}

extern "C" int mmg_contrast_device_bytes(mmg_contrast *h, uint64_t *bytes)
{
    if (!h || !bytes) return fail(MMG_ERR_ARG, "NULL argument");
    uint64_t b = 16 * ((uint64_t)h->C + 1) + 4 * (h->n_num + h->n_den);
    if (h->src.from_traces) b += 8 * (uint64_t)h->src.n * h->src.S;
    else b += 4 * h->slab_col.back() + 16 * (uint64_t)h->src.nv;
    *bytes = b;
    return MMG_OK;
}

extern "C" void mmg_contrast_destroy(mmg_contrast *h) { delete h; }
