// contrast.hip -- host side of the mmg_contrast_* entry points: posterior log-ratios between sets of transcripts of one sample from
// the kept samples of a chain.  Kernels in contrast_kernels.h, launched from post.hip (mmg_launch.h), as those of convergence.hip are:
// post_kernels.h, which they build on, defines its plain kernels outright and so belongs to one translation unit.  Specification in
// tests/contrast_ref.py and DESIGN.md section 13.
//
// The contrasts are cut into slabs of at most CONTRAST_SLAB_BYTES of series (at least one contrast), as mmg_convergence_create cuts
// its series.  Per slab: the distinct members of its contrasts are gathered out of the chain's sample-major trace (isoforms without
// hits: drawn) into a series-major matrix, a wave per contrast walks its two lists over that matrix, and the summary kernel takes
// the slab's series one workgroup each.  From host traces the uploaded matrix is series-major already and nothing is gathered.
#include "mmg_host.h"
#include "mmg_launch.h"

#include <algorithm>
#include <memory>
#include <vector>

using namespace mmg;

static constexpr size_t CONTRAST_SLAB_BYTES = 256u << 20;
static constexpr uint32_t CONTRAST_WS_GROUPS = 1024;

// Members are destroyed in reverse declaration order: the destructor waits for `st`, then the buffers go, and the stream last.
struct mmg_contrast {
    DevStream st;
    int device = 0;
    uint32_t C = 0, S = 0, n = 0, nv = 0, np = 0, cap = 0;
    bool from_traces = false;
    uint64_t n_num = 0, n_den = 0;
    // the descriptor on the device: the lists as slots of the slab's matrix (from host traces: the members themselves)
    DevBuf<uint64_t> d_num_ptr, d_den_ptr;
    DevBuf<uint32_t> d_num_slot, d_den_slot;
    // from a sampler: the distinct members of slab k are d_cols[slab_col[k] .. slab_col[k + 1]), ascending
    DevBuf<uint32_t> d_cols;
    std::vector<uint64_t> slab_col;
    uint64_t max_cols = 0;
    DevBuf<uint64_t> d_vid;
    DevBuf<double> d_vscale;
    const double *trace = nullptr;        // the summary's chain [S][n], device numbering (the sampler's)
    const uint32_t *int_of_ext = nullptr; // the problem's
    uint64_t seed = 0;
    double alpha = 0.0;
    // from host traces: [n_series][S]
    DevBuf<double> d_traces;
    // the results
    std::vector<double> log_ratio, var, tau, p_gt, pct;
    std::vector<int32_t> rc;
    ~mmg_contrast() { if (st) (void)hipStreamSynchronize(st.get()); }
};

namespace {

size_t workspace_elems(uint32_t S, uint32_t groups)
{
    if (S <= 8192) return 0;
    size_t sp = 1;
    while (sp < S) sp <<= 1;
    return (size_t)groups * 3 * sp;
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

template <typename T>
hipError_t upload(DevBuf<T> &buf, const T *src, size_t count, hipStream_t st)
{
    HIPE_TRY(buf.alloc(count ? count : 1));
    if (count) HIPE_TRY(hipMemcpyAsync(buf.get(), src, count * sizeof(T), hipMemcpyHostToDevice, st));
    return hipSuccess;
}

// the series of the contrasts [c0, c0 + cnt) of slab k (all inside it) into R[cnt][S]; gt: their counts of N_s > D_s, or null
void launch_rows(const mmg_contrast *h, uint32_t k, uint32_t c0, uint32_t cnt, double *M, double *R, uint32_t *gt, hipStream_t st)
{
    const double *src = h->d_traces.get();
    if (!h->from_traces) {
        launch_contrast_gather((uint32_t)(h->slab_col[k + 1] - h->slab_col[k]), h->S, h->n, h->d_cols.get() + h->slab_col[k], h->int_of_ext, h->trace, h->seed,
                               h->alpha, h->d_vid.get(), h->d_vscale.get(), M, st);
        src = M;
    }
    launch_contrast_series(c0, cnt, h->S, h->d_num_ptr.get(), h->d_num_slot.get(), h->d_den_ptr.get(), h->d_den_slot.get(), src, R, gt, st);
}

// The lists become slots, the descriptor goes to the device, every slab is summarised: what both create calls share.  h->device, S, n,
// nv, from_traces and the source pointers are set; the current device is h->device.
int build(mmg_contrast *h, const mmg_contrast_desc *d)
{
    const uint32_t C = d->n_contrasts, S = h->S, np = d->n_percentiles;
    h->C = C; h->np = np; h->cap = slab_cap(C, S);
    h->n_num = d->num_ptr[C]; h->n_den = d->den_ptr[C];
    const uint32_t cap = h->cap, n_slabs = (C + cap - 1) / cap;
    std::vector<uint32_t> num_slot(d->num_member, d->num_member + h->n_num), den_slot(d->den_member, d->den_member + h->n_den), cols;
    if (!h->from_traces) {
        // per slab: its distinct members, ascending (neighbours in the caller's numbering are mostly neighbours on the device); slot = rank
        std::vector<uint32_t> slot_of((size_t)h->n + h->nv, 0xffffffffu);
        h->slab_col.assign(1, 0);
        for (uint32_t k = 0; k < n_slabs; ++k) {
            const uint32_t c0 = k * cap, c1 = std::min<uint64_t>((uint64_t)c0 + cap, C);
            const size_t base = cols.size();
            auto collect = [&](const uint64_t *ptr, const uint32_t *mem) {
                for (uint64_t j = ptr[c0]; j < ptr[c1]; ++j)
                    if (slot_of[mem[j]] == 0xffffffffu) { slot_of[mem[j]] = 0; cols.push_back(mem[j]); }
            };
            collect(d->num_ptr, d->num_member);
            collect(d->den_ptr, d->den_member);
            std::sort(cols.begin() + (ptrdiff_t)base, cols.end());
            for (size_t i = base; i < cols.size(); ++i) slot_of[cols[i]] = (uint32_t)(i - base);
            for (uint64_t j = d->num_ptr[c0]; j < d->num_ptr[c1]; ++j) num_slot[j] = slot_of[d->num_member[j]];
            for (uint64_t j = d->den_ptr[c0]; j < d->den_ptr[c1]; ++j) den_slot[j] = slot_of[d->den_member[j]];
            for (size_t i = base; i < cols.size(); ++i) slot_of[cols[i]] = 0xffffffffu;
            h->slab_col.push_back(cols.size());
            h->max_cols = std::max<uint64_t>(h->max_cols, cols.size() - base);
        }
    }
    HIP_TRY(h->st.create(hipStreamNonBlocking));
    hipStream_t st = h->st.get();
    HIP_TRY(upload(h->d_num_ptr, d->num_ptr, (size_t)C + 1, st));
    HIP_TRY(upload(h->d_den_ptr, d->den_ptr, (size_t)C + 1, st));
    HIP_TRY(upload(h->d_num_slot, num_slot.data(), num_slot.size(), st));
    HIP_TRY(upload(h->d_den_slot, den_slot.data(), den_slot.size(), st));
    if (!h->from_traces) HIP_TRY(upload(h->d_cols, cols.data(), cols.size(), st));
    // the scratch of creation: a slab of series, the gathered members, the tables, a slab's results, the workspace
    DevBuf<double> d_R, d_M, d_tw, d_res;
    DevBuf<int32_t> d_pind, d_rc;
    DevBuf<uint32_t> d_gt;
    DevBuf<uint64_t> d_ws;
    const std::vector<double> tw = series_twiddles(S);
    HIP_TRY(upload(d_tw, tw.data(), tw.size(), st));
    HIP_TRY(upload(d_pind, d->percentile_index, (size_t)np, st));
    HIP_TRY(d_R.alloc((size_t)cap * S));
    if (!h->from_traces) HIP_TRY(d_M.alloc((size_t)h->max_cols * S));
    HIP_TRY(d_res.alloc((size_t)cap * (3 + (np ? np : 0)) + 1));
    HIP_TRY(d_rc.alloc(cap));
    HIP_TRY(d_gt.alloc(cap));
    const uint32_t ws_groups = cap < CONTRAST_WS_GROUPS ? cap : CONTRAST_WS_GROUPS;
    if (workspace_elems(S, ws_groups)) HIP_TRY(d_ws.alloc(workspace_elems(S, ws_groups)));
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

extern "C" int mmg_contrast_create(mmg_sampler *s, mmg_summary *q, const mmg_contrast_desc *d, mmg_contrast **out)
{
    if (!s || !q || !d || !out) return fail(MMG_ERR_ARG, "NULL argument");
    *out = nullptr;
    SamplerView v;
    int rc = sampler_view(s, &v);
    if (rc) return rc;
    SummaryView sv;
    rc = summary_view(q, &sv);
    if (rc) return rc;
    if (sv.p != v.p || !v.d_trace) return fail(MMG_ERR_ARG, "the summary is not one of this sampler");
    if (!sv.finished) return fail(MMG_ERR_STATE, "contrasts are taken after mmg_summary_finish");
    rc = check_desc(d, (uint64_t)sv.n + sv.nv);
    if (rc) return rc;
    rc = mmg_sampler_sync(s);   // every sample is final; nothing of the sampler is touched below
    if (rc) return rc;
    HIP_TRY(hipSetDevice(sv.device));
    std::unique_ptr<mmg_contrast> h(new mmg_contrast());
    h->device = sv.device; h->S = sv.S; h->n = sv.n; h->nv = sv.nv;
    h->trace = sv.trace; h->int_of_ext = sv.p->d_int_of_ext.get(); h->seed = sv.seed; h->alpha = sv.alpha;
    if (sv.nv) {
        HIP_TRY(h->d_vid.alloc(sv.nv));
        HIP_TRY(h->d_vscale.alloc(sv.nv));
        HIP_TRY(hipMemcpy(h->d_vid.get(), sv.vid, (size_t)sv.nv * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(h->d_vscale.get(), sv.vscale, (size_t)sv.nv * 8, hipMemcpyHostToDevice));
    }
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
    h->device = device; h->S = S; h->n = n_series; h->from_traces = true;
    HIP_TRY(h->d_traces.alloc((size_t)n_series * S));
    HIP_TRY(hipMemcpy(h->d_traces.get(), traces, (size_t)n_series * S * 8, hipMemcpyHostToDevice));
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
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = h->st.get();
    DevBuf<double> d_R, d_M;
    HIP_TRY(d_R.alloc((size_t)std::min(h->cap, count) * h->S));
    if (!h->from_traces) HIP_TRY(d_M.alloc((size_t)h->max_cols * h->S));
    for (uint32_t c = first; c < first + count;) {   // the piece of [first, first + count) in each slab it touches
        const uint32_t k = c / h->cap, end = std::min<uint64_t>((uint64_t)(k + 1) * h->cap, (uint64_t)first + count), cnt = end - c;
        launch_rows(h, k, c, cnt, d_M.get(), d_R.get(), nullptr, st);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(R + (size_t)(c - first) * h->S, d_R.get(), (size_t)cnt * h->S * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        c = end;
    }
    return MMG_OK;
}

extern "C" int mmg_contrast_device_bytes(mmg_contrast *h, uint64_t *bytes)
{
    if (!h || !bytes) return fail(MMG_ERR_ARG, "NULL argument");
    uint64_t b = 16 * ((uint64_t)h->C + 1) + 4 * (h->n_num + h->n_den);
    if (h->from_traces) b += 8 * (uint64_t)h->n * h->S;
    else b += 4 * h->slab_col.back() + 16 * (uint64_t)h->nv;
    *bytes = b;
    return MMG_OK;
}

extern "C" void mmg_contrast_destroy(mmg_contrast *h) { delete h; }
