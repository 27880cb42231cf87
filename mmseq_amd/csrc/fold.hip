// fold.hip -- device TU + host side of the mmg_fold_* entry points: the posterior log fold change of features between two samples from
// all pairs of their draws.  Kernel in fold_kernels.h; specification in tests/fold_ref.py and DESIGN.md section 16.
//
// The features are cut into slabs of cap = max(1, min(n_features, 256 MiB / (8 (Sa + Sb)), MMG_OPT_FOLD_SLAB if set)) consecutive
// features.  Per slab the two series-major matrices [cap][Sa] and [cap][Sb] are uploaded from the host traces, or gathered out of the
// two chains' sample-major traces (k_contrast_gather, no simulated members), and one workgroup per feature does the rest.  A feature's
// numbers depend on the feature alone, so the results do not depend on the cut.
#include "fold_kernels.h"
#include "mmg_host.h"
#include "mmg_launch.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

using namespace mmg;

static constexpr uint64_t FOLD_SLAB_BYTES = 256ull << 20;

// The results live on the host from creation; nothing on the device outlives it.
struct mmg_fold {
    uint64_t F = 0;
    uint32_t nr = 0;
    uint64_t peak_bytes = 0;
    std::vector<double> mean_a, mean_b, ss_a, ss_b, q;
    std::vector<uint32_t> n_gt, n_eq;
    std::vector<uint8_t> status;
};

namespace {

struct Side {
    uint32_t S = 0;
    // from a sampler: the chain [S][n] sample-major, device numbering, and the caller's transcript of every feature
    const double *trace = nullptr;
    const uint32_t *int_of_ext = nullptr;
    uint32_t n = 0;
    const uint32_t *member = nullptr;
    // from host traces: [n_features][S]
    const double *host = nullptr;
};

// what both create calls check of their common arguments
int check_common(uint32_t n_features, uint32_t Sa, uint32_t Sb, double off, uint32_t n_ranks, const uint32_t *ranks)
{
    if (n_features < 1) return fail(MMG_ERR_ARG, "n_features must be at least 1");
    if (Sa < 1 || Sa > FOLD_MAX_S) return fail(MMG_ERR_ARG, "Sa = " + std::to_string(Sa) + " is outside 1 .. " + std::to_string(FOLD_MAX_S));
    if (Sb < 1 || Sb > FOLD_MAX_S) return fail(MMG_ERR_ARG, "Sb = " + std::to_string(Sb) + " is outside 1 .. " + std::to_string(FOLD_MAX_S));
    if (!std::isfinite(off)) return fail(MMG_ERR_ARG, "off must be finite");
    if (n_ranks > FOLD_MAX_RANKS) return fail(MMG_ERR_ARG, "n_ranks = " + std::to_string(n_ranks) + " is more than " + std::to_string(FOLD_MAX_RANKS));
    if (n_ranks && !ranks) return fail(MMG_ERR_ARG, "ranks is NULL with n_ranks > 0");
    return MMG_OK;
}

uint64_t slab_cap(uint64_t F, uint32_t Sa, uint32_t Sb)
{
    uint64_t cap = std::min<uint64_t>(F, FOLD_SLAB_BYTES / (8ull * ((uint64_t)Sa + Sb)));
    const int o = opt(MMG_OPT_FOLD_SLAB);
    if (o > 0) cap = std::min<uint64_t>(cap, (uint64_t)o);
    return std::max<uint64_t>(cap, 1);
}

// what both create calls share; the current device is the sources'
int build(mmg_fold *h, const Side &sa, const Side &sb, uint64_t F, double off, uint32_t nr, const uint32_t *ranks)
{
    const uint32_t Sa = sa.S, Sb = sb.S, PA = next_pow2(Sa), PB = next_pow2(Sb);
    const uint64_t cap = slab_cap(F, Sa, Sb);
    const bool from_traces = sa.host != nullptr;
    const size_t lds = 8 * ((size_t)PA + PB);
    // everything on the device is scratch of this call, released with these owners (the stream last)
    DevStream stream;
    DevBuf<double> d_a, d_b, d_res, d_q;
    DevBuf<uint32_t> d_cnt, d_ranks, d_cols;
    DevBuf<uint8_t> d_status;
    HIP_TRY(stream.create(hipStreamNonBlocking));
    hipStream_t st = stream.get();
    HIP_TRY(d_a.alloc((size_t)cap * Sa));
    HIP_TRY(d_b.alloc((size_t)cap * Sb));
    HIP_TRY(d_res.alloc(4 * cap));
    HIP_TRY(d_cnt.alloc(2 * cap));
    HIP_TRY(d_status.alloc(cap));
    if (nr) {
        HIP_TRY(d_q.alloc((size_t)cap * nr));
        HIP_TRY(d_ranks.alloc(nr));
        HIP_TRY(hipMemcpyAsync(d_ranks.get(), ranks, (size_t)nr * 4, hipMemcpyHostToDevice, st));
    }
    if (!from_traces) HIP_TRY(d_cols.alloc(2 * cap));
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_fold), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    h->peak_bytes = 8 * cap * ((uint64_t)Sa + Sb) + cap * (41 + 8 * (uint64_t)nr) + 4 * (uint64_t)nr + (from_traces ? 0 : 8 * cap);
    h->F = F; h->nr = nr;
    std::vector<double> *res[4] = {&h->mean_a, &h->mean_b, &h->ss_a, &h->ss_b};
    for (auto *v : res) v->resize(F);
    h->n_gt.resize(F); h->n_eq.resize(F); h->status.resize(F); h->q.resize((size_t)F * nr);
    FoldOut o;
    o.mean_a = d_res.get(); o.mean_b = d_res.get() + cap; o.ss_a = d_res.get() + 2 * cap; o.ss_b = d_res.get() + 3 * cap;
    o.n_gt = d_cnt.get(); o.n_eq = d_cnt.get() + cap;
    o.q = d_q.get(); o.status = d_status.get();
    for (uint64_t f0 = 0; f0 < F; f0 += cap) {
        const uint32_t cnt = (uint32_t)std::min<uint64_t>(cap, F - f0);
        if (from_traces) {
            HIP_TRY(hipMemcpyAsync(d_a.get(), sa.host + f0 * Sa, (size_t)cnt * Sa * 8, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_b.get(), sb.host + f0 * Sb, (size_t)cnt * Sb * 8, hipMemcpyHostToDevice, st));
        } else {
            HIP_TRY(hipMemcpyAsync(d_cols.get(), sa.member + f0, (size_t)cnt * 4, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_cols.get() + cap, sb.member + f0, (size_t)cnt * 4, hipMemcpyHostToDevice, st));
            launch_contrast_gather(cnt, Sa, sa.n, d_cols.get(), sa.int_of_ext, sa.trace, 0, 0.0, nullptr, nullptr, d_a.get(), st);
            launch_contrast_gather(cnt, Sb, sb.n, d_cols.get() + cap, sb.int_of_ext, sb.trace, 0, 0.0, nullptr, nullptr, d_b.get(), st);
        }
        hipLaunchKernelGGL(k_fold, dim3(cnt), dim3(FOLD_BLOCK), lds, st, Sa, Sb, PA, PB, d_a.get(), d_b.get(), off, nr, d_ranks.get(), o);
        HIP_TRY(hipGetLastError());
        for (int k = 0; k < 4; ++k) HIP_TRY(hipMemcpyAsync(res[k]->data() + f0, d_res.get() + (size_t)k * cap, (size_t)cnt * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h->n_gt.data() + f0, o.n_gt, (size_t)cnt * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h->n_eq.data() + f0, o.n_eq, (size_t)cnt * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h->status.data() + f0, o.status, (size_t)cnt, hipMemcpyDeviceToHost, st));
        if (nr) HIP_TRY(hipMemcpyAsync(h->q.data() + f0 * nr, o.q, (size_t)cnt * nr * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));   // (the next slab overwrites the series and the results)
    }
    return MMG_OK;
}

// one side of mmg_fold_create: the sampler's chain, checked as mmg_pairs_create checks its own
int sampler_side(mmg_sampler *s, int chain, const char *which, uint32_t n_features, const uint32_t *member, SamplerView &v, Side &side)
{
    int rc = sampler_view(s, &v);
    if (rc) return rc;
    const std::string w = which;
    if (chain < 0 || chain >= v.cfg.n_chains) return fail(MMG_ERR_ARG, "chain_" + w + " out of range");
    for (uint32_t f = 0; f < n_features; ++f)
        if (member[f] >= v.p->n)
            return fail(MMG_ERR_ARG, "feature " + std::to_string(f) + ": i" + w + " = " + std::to_string(member[f]) + " out of range (n = " + std::to_string(v.p->n) + ")");
    if (!v.d_trace) return fail(MMG_ERR_STATE, "sampler s" + w + " was created with keep_trace == 0");
    if (v.n_kept < (int64_t)v.cfg.trace_len) return fail(MMG_ERR_STATE, "the fold is taken after the last kept sample of sampler s" + w);
    side.S = (uint32_t)v.cfg.trace_len;
    side.n = v.p->n;
    side.trace = v.d_trace + (uint64_t)chain * (uint64_t)v.cfg.trace_len * v.p->n;
    side.int_of_ext = v.p->d_int_of_ext.get();
    side.member = member;
    return MMG_OK;
}

} // namespace

extern "C" int mmg_fold_create(mmg_sampler *sa, int chain_a, mmg_sampler *sb, int chain_b, uint32_t n_features, const uint32_t *ia, const uint32_t *ib,
                               double off, uint32_t n_ranks, const uint32_t *ranks, mmg_fold **out)
{
    if (!sa || !sb || !out) return fail(MMG_ERR_ARG, "NULL argument (sa, sb or out)");
    *out = nullptr;
    if (n_features < 1) return fail(MMG_ERR_ARG, "n_features must be at least 1");
    if (!ia || !ib) return fail(MMG_ERR_ARG, "NULL feature array (ia or ib)");
    SamplerView va, vb;
    Side a, b;
    int rc = sampler_side(sa, chain_a, "a", n_features, ia, va, a);
    if (rc) return rc;
    rc = sampler_side(sb, chain_b, "b", n_features, ib, vb, b);
    if (rc) return rc;
    rc = check_common(n_features, a.S, b.S, off, n_ranks, ranks);
    if (rc) return rc;
    if (va.p->device != vb.p->device) return fail(MMG_ERR_ARG, "samplers sa and sb are on different devices");
    rc = mmg_sampler_sync(sa);   // every sample is final; nothing of the samplers is touched below
    if (rc) return rc;
    if (sb != sa) { rc = mmg_sampler_sync(sb); if (rc) return rc; }
    HIP_TRY(hipSetDevice(va.p->device));
    std::unique_ptr<mmg_fold> h(new mmg_fold());
    rc = build(h.get(), a, b, n_features, off, n_ranks, ranks);
    if (rc) return rc;
    *out = h.release();
    return MMG_OK;
}

extern "C" int mmg_fold_of_traces(int device, uint32_t n_features, uint32_t Sa, const double *a, uint32_t Sb, const double *b, double off,
                                  uint32_t n_ranks, const uint32_t *ranks, mmg_fold **out)
{
    if (!a || !b || !out) return fail(MMG_ERR_ARG, "NULL argument (a, b or out)");
    *out = nullptr;
    int rc = check_common(n_features, Sa, Sb, off, n_ranks, ranks);
    if (rc) return rc;
    rc = require_device(device);
    if (rc) return rc;
    std::unique_ptr<mmg_fold> h(new mmg_fold());
    Side sa, sb;
    sa.S = Sa; sa.host = a;
    sb.S = Sb; sb.host = b;
    rc = build(h.get(), sa, sb, n_features, off, n_ranks, ranks);
    if (rc) return rc;
    *out = h.release();
    return MMG_OK;
}

extern "C" int mmg_fold_get(mmg_fold *h, double *mean_a, double *mean_b, double *ss_a, double *ss_b, uint32_t *n_gt, uint32_t *n_eq, double *quantiles,
                            uint8_t *status)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL fold handle");
    const size_t bytes = (size_t)h->F * 8;
    if (mean_a) std::memcpy(mean_a, h->mean_a.data(), bytes);
    if (mean_b) std::memcpy(mean_b, h->mean_b.data(), bytes);
    if (ss_a) std::memcpy(ss_a, h->ss_a.data(), bytes);
    if (ss_b) std::memcpy(ss_b, h->ss_b.data(), bytes);
    if (n_gt) std::memcpy(n_gt, h->n_gt.data(), (size_t)h->F * 4);
    if (n_eq) std::memcpy(n_eq, h->n_eq.data(), (size_t)h->F * 4);
    if (quantiles && h->nr) std::memcpy(quantiles, h->q.data(), bytes * h->nr);
    if (status) std::memcpy(status, h->status.data(), (size_t)h->F);
    return MMG_OK;
}

extern "C" int mmg_fold_device_bytes(mmg_fold *h, uint64_t *bytes)
{
    if (!h || !bytes) return fail(MMG_ERR_ARG, "NULL argument");
    *bytes = h->peak_bytes;
    return MMG_OK;
}

extern "C" void mmg_fold_destroy(mmg_fold *h) { delete h; }
