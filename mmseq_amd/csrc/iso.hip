// iso.hip -- device TU + host side of the mmg_isoform_* entry points: posterior isoform usage within groups of transcripts of one
// sample, from the joint draws of a group's members in the kept samples of a chain.  Kernels in iso_kernels.h; specification in
// tests/isoforms_ref.py and DESIGN.md section 18.
//
// The groups are cut into slabs of consecutive groups: a slab ends in front of the group that would bring its distinct members over
// ISO_SLAB_BYTES of gathered series (from a sampler) or its groups over the group cap (ISO_SLAB_BYTES of H and P rows, MMG_OPT_ISO_SLAB);
// a slab holds at least one group.  Per slab: the distinct members are gathered out of the chain's sample-major trace (isoforms
// without hits: drawn) into a series-major matrix (k_contrast_gather, unchanged), a wave per group walks its list over that matrix,
// and a workgroup per group summarises the two series.  From host traces the uploaded matrix is series-major already and nothing is
// gathered.  A group's numbers depend on its own members alone, so the results do not depend on the cut.
#include "iso_kernels.h"
#include "mmg_host.h"
#include "mmg_launch.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

using namespace mmg;

static constexpr uint64_t ISO_SLAB_BYTES = 256ull << 20;

namespace {
struct IsoSlab {
    uint32_t g0 = 0, ng = 0;   // the groups [g0, g0 + ng)
    uint64_t c0 = 0, nm = 0;   // from a sampler: its distinct members cols[c0 .. c0 + nm), ascending
};
} // namespace

// Members are destroyed in reverse declaration order: the destructor waits for `st`, then the buffers go, and the stream last.
struct mmg_isoform {
    DevStream st;
    uint32_t G = 0, nq = 0, nr = 0;
    uint64_t n_members = 0;
    // the description on the device: the lists as slots of their slab's matrix (from host traces: the members themselves)
    DevBuf<uint64_t> d_ptr;
    DevBuf<uint32_t> d_slot;
    DevBuf<uint32_t> d_cols;
    std::vector<IsoSlab> slabs;
    uint64_t max_cols = 0, n_cols = 0;
    uint32_t max_groups = 0;
    MemberSource src;
    // the results
    std::vector<uint32_t> n_top, n_second, n_above, major, n_distinct;
    std::vector<uint8_t> status;
    std::vector<double> mean_H, ss_H, mean_P, ss_P, q_H, q_P;
    ~mmg_isoform() { if (st) (void)hipStreamSynchronize(st.get()); }
};

namespace {

// everything of a description that can be wrong, before any device work; limit: the members are < limit
int check_desc(const mmg_isoform_desc *d, uint64_t limit, uint32_t S)
{
    if (S < 1 || S > ISO_MAX_S) return fail(MMG_ERR_ARG, "S = " + std::to_string(S) + " must be in [1, " + std::to_string(ISO_MAX_S) + "]");
    if (d->n_groups == 0) return fail(MMG_ERR_ARG, "n_groups must be at least 1");
    if (!d->ptr || !d->member) return fail(MMG_ERR_ARG, "isoform description: ptr or member is NULL");
    if (d->n_groups >= 0x7fffffffu) return fail(MMG_ERR_ARG, "n_groups: too many groups");
    if (d->n_thresholds > ISO_MAX_THRESHOLDS)
        return fail(MMG_ERR_ARG, "n_thresholds = " + std::to_string(d->n_thresholds) + " is more than " + std::to_string(ISO_MAX_THRESHOLDS));
    if (d->n_thresholds && !d->threshold) return fail(MMG_ERR_ARG, "threshold is NULL with n_thresholds > 0");
    for (uint32_t q = 0; q < d->n_thresholds; ++q)
        if (!(d->threshold[q] >= 0.0 && d->threshold[q] < 1.0))
            return fail(MMG_ERR_ARG, "threshold " + std::to_string(q) + " = " + std::to_string(d->threshold[q]) + " must be finite and in [0, 1)");
    if (d->n_ranks > ISO_MAX_RANKS) return fail(MMG_ERR_ARG, "n_ranks = " + std::to_string(d->n_ranks) + " is more than " + std::to_string(ISO_MAX_RANKS));
    if (d->n_ranks && !d->rank) return fail(MMG_ERR_ARG, "rank is NULL with n_ranks > 0");
    if (d->ptr[0] != 0) return fail(MMG_ERR_ARG, "ptr must start at 0");
    std::vector<uint32_t> seen(limit, 0xffffffffu);   // the last group a member was seen in (n_groups < 2^31: 0xffffffff is no group)
    for (uint32_t g = 0; g < d->n_groups; ++g) {
        if (d->ptr[g + 1] < d->ptr[g]) return fail(MMG_ERR_ARG, "ptr must not decrease (group " + std::to_string(g) + ")");
        if (d->ptr[g + 1] == d->ptr[g]) return fail(MMG_ERR_ARG, "empty group " + std::to_string(g));
        for (uint64_t j = d->ptr[g]; j < d->ptr[g + 1]; ++j) {
            const uint32_t m = d->member[j];
            const std::string where = "member " + std::to_string(m) + " (position " + std::to_string(j - d->ptr[g]) + " of group " + std::to_string(g) + ")";
            if (m >= limit) return fail(MMG_ERR_ARG, where + " out of range (limit " + std::to_string(limit) + ")");
            if (seen[m] == g) return fail(MMG_ERR_ARG, where + " twice in the group");
            seen[m] = g;
        }
    }
    return MMG_OK;
}

uint32_t group_cap(uint32_t G, uint32_t S)
{
    uint64_t cap = std::max<uint64_t>(1, ISO_SLAB_BYTES / (16ull * S));
    cap = std::min<uint64_t>(cap, G);
    const int o = opt(MMG_OPT_ISO_SLAB);
    if (o > 0 && (uint64_t)o < cap) cap = (uint64_t)o;
    return (uint32_t)cap;
}

// consecutive groups, greedily; from a sampler also the slabs' member lists one after the other (cols) and every list entry as the
// slot of its member in its slab's list
void cut_slabs(mmg_isoform *h, const mmg_isoform_desc *d, std::vector<uint32_t> &cols, std::vector<uint32_t> &slot)
{
    const bool from_traces = h->src.from_traces;
    const uint32_t G = h->G, S = h->src.S, gcap = group_cap(G, S);
    const uint64_t mcap = std::max<uint64_t>(1, ISO_SLAB_BYTES / (8ull * S));
    SlabColumns sc(from_traces ? 0 : (size_t)h->src.n + h->src.nv);
    for (uint32_t g0 = 0; g0 < G;) {
        IsoSlab sl;
        sl.g0 = g0; sl.c0 = sc.first();
        uint32_t g = g0;
        for (; g < G && g - g0 < gcap; ++g) {
            if (from_traces) continue;
            uint64_t fresh = 0;
            for (uint64_t j = d->ptr[g]; j < d->ptr[g + 1]; ++j) fresh += sc.fresh(d->member[j]);
            if (g > g0 && sc.count() + fresh > mcap) break;
            for (uint64_t j = d->ptr[g]; j < d->ptr[g + 1]; ++j) sc.add(d->member[j]);
        }
        sl.ng = g - g0;
        if (!from_traces) {
            sl.nm = sc.count();
            sc.close([&](auto slot_of) { for (uint64_t j = d->ptr[g0]; j < d->ptr[g]; ++j) slot[j] = slot_of(d->member[j]); });
            h->max_cols = std::max(h->max_cols, sl.nm);
        }
        h->max_groups = std::max(h->max_groups, sl.ng);
        h->slabs.push_back(sl);
        g0 = g;
    }
    cols = std::move(sc.cols);
    h->n_cols = cols.size();
}

// the rows of the groups [g, g + cnt) of slab sl (all inside it) into row 0 .. cnt - 1 of the outputs; cnt_words null: rows only
void launch_rows(const mmg_isoform *h, const IsoSlab &sl, uint32_t g, uint32_t cnt, uint32_t nq, const IsoTheta &theta, double *M, uint32_t *top,
                 uint32_t *second, double *H, double *P, uint8_t *bad, uint32_t *cnt_words, hipStream_t st)
{
    const double *src = h->src.rows(h->src.from_traces ? nullptr : h->d_cols.get() + sl.c0, (uint32_t)sl.nm, M, st);
    constexpr unsigned per = ISO_BLOCK / ISO_LANES;
    hipLaunchKernelGGL(k_iso_series, dim3((cnt + per - 1) / per), dim3(ISO_BLOCK), 0, st, g, cnt, h->src.S, nq, theta, (const uint64_t *)h->d_ptr.get(),
                       (const uint32_t *)h->d_slot.get(), src, top, second, H, P, bad, cnt_words);
}

// The lists become slots, the description goes to the device, every slab is summarised: what both create calls share.  h->src is set;
// the current device is its device.
int build(mmg_isoform *h, const mmg_isoform_desc *d)
{
    const bool from_traces = h->src.from_traces;
    const uint32_t G = d->n_groups, S = h->src.S, nq = d->n_thresholds, nr = d->n_ranks, stride = 2 + nq;
    h->G = G; h->nq = nq; h->nr = nr; h->n_members = d->ptr[G];
    const uint64_t NM = h->n_members;
    if (NM * stride >= (1ull << 40)) return fail(MMG_ERR_ARG, "member: too many list entries");
    std::vector<uint32_t> cols, slot(d->member, d->member + NM);
    cut_slabs(h, d, cols, slot);
    const uint32_t gx = h->max_groups;
    IsoTheta theta{};
    for (uint32_t q = 0; q < nq; ++q) theta.v[q] = d->threshold[q];
    const uint32_t PP = next_pow2(S);
    const size_t lds = 16 * (size_t)PP;

    HIP_TRY(h->st.create(hipStreamNonBlocking));
    hipStream_t st = h->st.get();
    HIP_TRY(upload(h->d_ptr, d->ptr, (size_t)G + 1, st));
    HIP_TRY(upload(h->d_slot, slot.data(), slot.size(), st));
    if (!from_traces) HIP_TRY(upload(h->d_cols, cols.data(), cols.size(), st));
    // the scratch of creation: the gathered members, a slab's rows and results, the counters of every list entry, the ranks
    DevBuf<double> d_M, d_H, d_P, d_res;
    DevBuf<uint32_t> d_cnt, d_ranks, d_gi;
    DevBuf<uint8_t> d_bad;
    if (!from_traces) HIP_TRY(d_M.alloc((size_t)h->max_cols * S));
    HIP_TRY(d_H.alloc((size_t)gx * S));
    HIP_TRY(d_P.alloc((size_t)gx * S));
    HIP_TRY(d_res.alloc((size_t)gx * (4 + 2 * (size_t)nr)));
    HIP_TRY(d_gi.alloc(2 * (size_t)gx));
    HIP_TRY(d_bad.alloc(gx));
    HIP_TRY(d_cnt.alloc(NM * stride));
    HIP_TRY(upload(d_ranks, d->rank, (size_t)nr, st));
    HIP_TRY(hipMemsetAsync(d_cnt.get(), 0, NM * stride * 4, st));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_iso_summary), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));

    h->status.resize(G); h->major.resize(G); h->n_distinct.resize(G);
    h->mean_H.resize(G); h->ss_H.resize(G); h->mean_P.resize(G); h->ss_P.resize(G);
    h->q_H.resize((size_t)G * nr); h->q_P.resize((size_t)G * nr);
    IsoOut o;
    double *const r = d_res.get();
    o.mean_H = r; o.ss_H = r + gx; o.mean_P = r + 2 * (size_t)gx; o.ss_P = r + 3 * (size_t)gx;
    o.q_H = r + 4 * (size_t)gx; o.q_P = o.q_H + (size_t)gx * nr;
    o.major = d_gi.get(); o.n_distinct = d_gi.get() + gx;
    for (const IsoSlab &sl : h->slabs) {
        const uint32_t g0 = sl.g0, ng = sl.ng;
        launch_rows(h, sl, g0, ng, nq, theta, d_M.get(), nullptr, nullptr, d_H.get(), d_P.get(), d_bad.get(), d_cnt.get(), st);
        hipLaunchKernelGGL(k_iso_summary, dim3(ng), dim3(ISO_BLOCK), lds, st, g0, S, PP, nq, (const uint64_t *)h->d_ptr.get(), (const double *)d_H.get(),
                           (const double *)d_P.get(), (const uint8_t *)d_bad.get(), (const uint32_t *)d_cnt.get(), nr, (const uint32_t *)d_ranks.get(), o);
        HIP_TRY(hipGetLastError());
        double *dst[4] = {h->mean_H.data(), h->ss_H.data(), h->mean_P.data(), h->ss_P.data()};
        for (int k = 0; k < 4; ++k) HIP_TRY(hipMemcpyAsync(dst[k] + g0, r + (size_t)k * gx, (size_t)ng * 8, hipMemcpyDeviceToHost, st));
        if (nr) {
            HIP_TRY(hipMemcpyAsync(h->q_H.data() + (size_t)g0 * nr, o.q_H, (size_t)ng * nr * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(h->q_P.data() + (size_t)g0 * nr, o.q_P, (size_t)ng * nr * 8, hipMemcpyDeviceToHost, st));
        }
        HIP_TRY(hipMemcpyAsync(h->major.data() + g0, o.major, (size_t)ng * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h->n_distinct.data() + g0, o.n_distinct, (size_t)ng * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h->status.data() + g0, d_bad.get(), ng, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));   // (the next slab overwrites the rows and the results)
    }
    std::vector<uint32_t> words(NM * stride);
    HIP_TRY(hipMemcpyAsync(words.data(), d_cnt.get(), words.size() * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    h->n_top.resize(NM); h->n_second.resize(NM); h->n_above.resize(NM * nq);
    for (uint64_t j = 0; j < NM; ++j) {
        h->n_top[j] = words[j * stride];
        h->n_second[j] = words[j * stride + 1];
        for (uint32_t q = 0; q < nq; ++q) h->n_above[j * nq + q] = words[j * stride + 2 + q];
    }
    return MMG_OK;
}

} // namespace

extern "C" int mmg_isoform_create(mmg_sampler *s, mmg_summary *q, const mmg_isoform_desc *d, mmg_isoform **out)
{
    if (!s || !q || !d || !out) return fail(MMG_ERR_ARG, "NULL argument");
    *out = nullptr;
    std::unique_ptr<mmg_isoform> h(new mmg_isoform());
    int rc = h->src.view_summary(s, q, "isoform usage is taken after mmg_summary_finish");
    if (rc) return rc;
    rc = check_desc(d, (uint64_t)h->src.n + h->src.nv, h->src.S);
    if (rc) return rc;
    rc = h->src.acquire(s);
    if (rc) return rc;
    rc = build(h.get(), d);
    if (rc) return rc;
    *out = h.release();
    return MMG_OK;
}

extern "C" int mmg_isoform_of_traces(int device, uint32_t S, uint32_t n_series, const double *traces, const mmg_isoform_desc *d, mmg_isoform **out)
{
    if (!traces || !d || !out) return fail(MMG_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (n_series < 1) return fail(MMG_ERR_ARG, "n_series must be at least 1");
    int rc = check_desc(d, n_series, S);
    if (rc) return rc;
    rc = require_device(device);
    if (rc) return rc;
    std::unique_ptr<mmg_isoform> h(new mmg_isoform());
    rc = h->src.from_host(device, S, n_series, traces);
    if (rc) return rc;
    rc = build(h.get(), d);
    if (rc) return rc;
    *out = h.release();
    return MMG_OK;
}

extern "C" int mmg_isoform_get_members(mmg_isoform *h, uint32_t *n_top, uint32_t *n_second, uint32_t *n_above)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL isoform handle");
    if (n_top) std::memcpy(n_top, h->n_top.data(), h->n_members * 4);
    if (n_second) std::memcpy(n_second, h->n_second.data(), h->n_members * 4);
    if (n_above && h->nq) std::memcpy(n_above, h->n_above.data(), h->n_members * h->nq * 4);
    return MMG_OK;
}

extern "C" int mmg_isoform_get_groups(mmg_isoform *h, uint8_t *status, uint32_t *major, uint32_t *n_distinct, double *mean_H, double *ss_H, double *mean_P,
                                      double *ss_P, double *q_H, double *q_P)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL isoform handle");
    const size_t g = h->G;
    if (status) std::memcpy(status, h->status.data(), g);
    if (major) std::memcpy(major, h->major.data(), g * 4);
    if (n_distinct) std::memcpy(n_distinct, h->n_distinct.data(), g * 4);
    if (mean_H) std::memcpy(mean_H, h->mean_H.data(), g * 8);
    if (ss_H) std::memcpy(ss_H, h->ss_H.data(), g * 8);
    if (mean_P) std::memcpy(mean_P, h->mean_P.data(), g * 8);
    if (ss_P) std::memcpy(ss_P, h->ss_P.data(), g * 8);
    if (q_H && h->nr) std::memcpy(q_H, h->q_H.data(), g * h->nr * 8);
    if (q_P && h->nr) std::memcpy(q_P, h->q_P.data(), g * h->nr * 8);
    return MMG_OK;
}

extern "C" int mmg_isoform_get_rows(mmg_isoform *h, uint32_t first, uint32_t count, uint32_t *top, uint32_t *second, double *H, double *P)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL isoform handle");
    if (first > h->G || count > h->G - first) return fail(MMG_ERR_ARG, "group range out of bounds");
    if (!count) return MMG_OK;
    HIP_TRY(hipSetDevice(h->src.device));
    hipStream_t st = h->st.get();
    const uint32_t S = h->src.S, rows = std::min(h->max_groups, count);
    DevBuf<double> d_M, d_H, d_P;
    DevBuf<uint32_t> d_top, d_second;
    if (!h->src.from_traces) HIP_TRY(d_M.alloc((size_t)h->max_cols * S));
    HIP_TRY(d_H.alloc((size_t)rows * S));
    HIP_TRY(d_P.alloc((size_t)rows * S));
    if (top) HIP_TRY(d_top.alloc((size_t)rows * S));
    if (second) HIP_TRY(d_second.alloc((size_t)rows * S));
    const IsoTheta none{};
    // the slab of `first`: the last one that starts at or before it
    size_t k = (size_t)(std::upper_bound(h->slabs.begin(), h->slabs.end(), first, [](uint32_t g, const IsoSlab &sl) { return g < sl.g0; }) - h->slabs.begin()) - 1;
    for (uint32_t g = first; g < first + count; ++k) {   // the piece of [first, first + count) in each slab it touches
        const IsoSlab &sl = h->slabs[k];
        const uint32_t end = (uint32_t)std::min<uint64_t>((uint64_t)sl.g0 + sl.ng, (uint64_t)first + count), cnt = end - g;
        launch_rows(h, sl, g, cnt, 0, none, d_M.get(), d_top.get(), d_second.get(), d_H.get(), d_P.get(), nullptr, nullptr, st);
        HIP_TRY(hipGetLastError());
        const size_t at = (size_t)(g - first) * S, words = (size_t)cnt * S;
        if (top) HIP_TRY(hipMemcpyAsync(top + at, d_top.get(), words * 4, hipMemcpyDeviceToHost, st));
        if (second) HIP_TRY(hipMemcpyAsync(second + at, d_second.get(), words * 4, hipMemcpyDeviceToHost, st));
        if (H) HIP_TRY(hipMemcpyAsync(H + at, d_H.get(), words * 8, hipMemcpyDeviceToHost, st));
        if (P) HIP_TRY(hipMemcpyAsync(P + at, d_P.get(), words * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        g = end;
    }
    return MMG_OK;
}

extern "C" int mmg_isoform_device_bytes(mmg_isoform *h, uint64_t *bytes)
{
    if (!h || !bytes) return fail(MMG_ERR_ARG, "NULL argument");
    uint64_t b = 8 * ((uint64_t)h->G + 1) + 4 * h->n_members;
    if (h->src.from_traces) b += 8 * (uint64_t)h->src.n * h->src.S;
    else b += 4 * h->n_cols + 16 * (uint64_t)h->src.nv;
    *bytes = b;
    return MMG_OK;
}

extern "C" void mmg_isoform_destroy(mmg_isoform *h) { delete h; }
