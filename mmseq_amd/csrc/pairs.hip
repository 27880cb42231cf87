// pairs.hip -- device TU + host side of the mmg_pairs_* entry points: the posterior correlation of pairs of transcripts of one sample
// from the kept samples of a chain.  Kernels in pair_kernels.h; specification in tests/pairs_ref.py and DESIGN.md section 15.
//
// The pairs are cut into slabs of consecutive pairs whose distinct members' two matrices (the gathered traces and the centred
// logarithms, 16 S bytes per member) fit PAIRS_SLAB_BYTES (at least one pair).  Per slab: the distinct members are compacted on the
// host, their columns gathered out of the chain's sample-major trace into a series-major matrix (k_contrast_gather, no simulated
// members), a wave per member takes its logarithms, mean and centred row, and a wave per pair does the rest.  From host traces the
// uploaded matrix is series-major already and nothing is gathered: the member pass reads the members' rows where they are.
// A member's numbers depend on the member alone, so the results do not depend on the cut.
#include "pair_kernels.h"
#include "mmg_host.h"

#include <algorithm>
#include <memory>
#include <vector>

using namespace mmg;

static constexpr uint64_t PAIRS_SLAB_BYTES = 256ull << 20;
static constexpr uint64_t PAIRS_SLAB_MAX = 1ull << 22;   // pairs per slab at most (68 bytes of slots and results each)

// The results live on the host from creation; nothing on the device outlives it.
struct mmg_pairs {
    uint64_t P = 0;
    uint64_t peak_bytes = 0;
    std::vector<double> mean_a, mean_b, mean_sum, saa, sbb, sab, sss;
    std::vector<uint32_t> n_gt;
};

namespace {

int check_pairs(uint64_t n_pairs, const uint32_t *a, const uint32_t *b, uint32_t n)
{
    if (n_pairs == 0) return fail(MMG_ERR_ARG, "n_pairs must be at least 1");
    if (!a || !b) return fail(MMG_ERR_ARG, "NULL pair array");
    for (uint64_t p = 0; p < n_pairs; ++p) {
        const std::string where = "pair " + std::to_string(p) + ": ";
        if (a[p] >= n || b[p] >= n) return fail(MMG_ERR_ARG, where + "member " + std::to_string(a[p] >= n ? a[p] : b[p]) + " out of range (n = " + std::to_string(n) + ")");
        if (a[p] == b[p]) return fail(MMG_ERR_ARG, where + "a == b (member " + std::to_string(a[p]) + ")");
    }
    return MMG_OK;
}

struct Slab {
    uint64_t p0 = 0, np = 0;   // the pairs [p0, p0 + np)
    uint64_t c0 = 0, nm = 0;   // its distinct members cols[c0 .. c0 + nm), ascending
};

// members per slab at most: 16 S bytes each in PAIRS_SLAB_BYTES, two at least (one pair)
uint64_t member_cap(uint32_t S)
{
    return std::max<uint64_t>(2, PAIRS_SLAB_BYTES / (16ull * S));
}

uint64_t pair_cap()
{
    const int o = opt(MMG_OPT_PAIRS_SLAB);
    return o > 0 ? std::min<uint64_t>((uint64_t)o, PAIRS_SLAB_MAX) : PAIRS_SLAB_MAX;
}

// consecutive pairs, greedily: a slab ends in front of the pair that would bring its distinct members over member_cap or its pairs over
// pair_cap.  cols: the slabs' member lists one after the other; sa / sb: every pair's members as slots of its slab's list.
void cut_slabs(uint64_t P, const uint32_t *a, const uint32_t *b, uint32_t n, uint32_t S, std::vector<Slab> &slabs, std::vector<uint32_t> &cols,
               std::vector<uint32_t> &sa, std::vector<uint32_t> &sb)
{
    const uint64_t mcap = member_cap(S), pcap = pair_cap();
    SlabColumns sc(n);
    sa.resize(P); sb.resize(P);
    for (uint64_t p0 = 0; p0 < P;) {
        Slab sl;
        sl.p0 = p0; sl.c0 = sc.first();
        uint64_t p = p0;
        for (; p < P && p - p0 < pcap; ++p) {
            const uint64_t fresh = (uint64_t)sc.fresh(a[p]) + sc.fresh(b[p]);
            if (p > p0 && sc.count() + fresh > mcap) break;
            sc.add(a[p]);
            sc.add(b[p]);
        }
        sl.np = p - p0; sl.nm = sc.count();
        sc.close([&](auto slot) { for (uint64_t q = p0; q < p; ++q) { sa[q] = slot(a[q]); sb[q] = slot(b[q]); } });
        slabs.push_back(sl);
        p0 = p;
    }
    cols = std::move(sc.cols);
}

// what both create calls share; the current device is the source's, st a stream of it that outlives the call
int build(mmg_pairs *h, const MemberSource &src, hipStream_t st, uint64_t P, const uint32_t *a, const uint32_t *b)
{
    const uint32_t S = src.S;
    std::vector<Slab> slabs;
    std::vector<uint32_t> cols, sa, sb;
    cut_slabs(P, a, b, src.n, S, slabs, cols, sa, sb);
    uint64_t Mx = 0, Px = 0;
    for (const Slab &sl : slabs) { Mx = std::max(Mx, sl.nm); Px = std::max(Px, sl.np); }
    const bool from_traces = src.from_traces;
    // everything on the device is scratch of this call, released with these owners, the caller's source and its stream
    DevBuf<double> d_M, d_C, d_mstat, d_res;
    DevBuf<uint32_t> d_cols, d_slots, d_gt;
    if (!from_traces) HIP_TRY(d_M.alloc((size_t)Mx * S));
    HIP_TRY(d_cols.alloc(Mx));
    HIP_TRY(d_C.alloc((size_t)Mx * S));
    HIP_TRY(d_mstat.alloc(2 * Mx));
    HIP_TRY(d_slots.alloc(2 * Px));
    HIP_TRY(d_res.alloc(7 * Px));
    HIP_TRY(d_gt.alloc(Px));
    h->peak_bytes = 4 * Mx + 8 * (uint64_t)S * Mx + 16 * Mx + 8 * Px + 60 * Px + (from_traces ? 8 * (uint64_t)src.n * S : 8 * (uint64_t)S * Mx);
    h->P = P;
    std::vector<double> *res[7] = {&h->mean_a, &h->mean_b, &h->mean_sum, &h->saa, &h->sbb, &h->sab, &h->sss};
    for (auto *v : res) v->resize(P);
    h->n_gt.resize(P);
    const bool reg = S <= PAIR_REG_SAMPLES;
    constexpr unsigned per = PAIR_BLOCK / PAIR_LANES;
    for (const Slab &sl : slabs) {
        const uint32_t nm = (uint32_t)sl.nm, np = (uint32_t)sl.np;
        HIP_TRY(hipMemcpyAsync(d_cols.get(), cols.data() + sl.c0, (size_t)nm * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_slots.get(), sa.data() + sl.p0, (size_t)np * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(d_slots.get() + Px, sb.data() + sl.p0, (size_t)np * 4, hipMemcpyHostToDevice, st));
        // gathered: member j is row j of X; from host traces: row d_cols[j] of the uploaded matrix
        const double *X = src.rows(d_cols.get(), nm, d_M.get(), st);
        const uint32_t *row = from_traces ? d_cols.get() : nullptr;
        double *mean = d_mstat.get(), *saa = d_mstat.get() + Mx;
        PairOut o;
        double *r = d_res.get();
        o.mean_a = r; o.mean_b = r + Px; o.mean_sum = r + 2 * Px; o.saa = r + 3 * Px; o.sbb = r + 4 * Px; o.sab = r + 5 * Px; o.sss = r + 6 * Px;
        o.n_gt = d_gt.get();
        const dim3 gm((nm + per - 1) / per), gp((np + per - 1) / per), blk(PAIR_BLOCK);
        if (reg) {
            hipLaunchKernelGGL(k_pair_members<true>, gm, blk, 0, st, nm, S, row, X, d_C.get(), mean, saa);
            hipLaunchKernelGGL(k_pair_stats<true>, gp, blk, 0, st, np, S, d_slots.get(), d_slots.get() + Px, row, X, d_C.get(), mean, saa, o);
        } else {
            hipLaunchKernelGGL(k_pair_members<false>, gm, blk, 0, st, nm, S, row, X, d_C.get(), mean, saa);
            hipLaunchKernelGGL(k_pair_stats<false>, gp, blk, 0, st, np, S, d_slots.get(), d_slots.get() + Px, row, X, d_C.get(), mean, saa, o);
        }
        HIP_TRY(hipGetLastError());
        for (int k = 0; k < 7; ++k) HIP_TRY(hipMemcpyAsync(res[k]->data() + sl.p0, r + (size_t)k * Px, (size_t)np * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(h->n_gt.data() + sl.p0, d_gt.get(), (size_t)np * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));   // (the next slab overwrites the lists and the results)
    }
    return MMG_OK;
}

} // namespace

extern "C" int mmg_pairs_create(mmg_sampler *s, int chain, uint64_t n_pairs, const uint32_t *a, const uint32_t *b, mmg_pairs **out)
{
    if (!s || !out) return fail(MMG_ERR_ARG, "NULL argument");
    *out = nullptr;
    SamplerView v;
    int rc = sampler_view(s, &v);
    if (rc) return rc;
    if (chain < 0 || chain >= v.cfg.n_chains) return fail(MMG_ERR_ARG, "chain index out of range");
    rc = check_pairs(n_pairs, a, b, v.p->n);
    if (rc) return rc;
    if (!v.d_trace) return fail(MMG_ERR_STATE, "sampler was created with keep_trace == 0");
    if (v.n_kept < (int64_t)v.cfg.trace_len) return fail(MMG_ERR_STATE, "pairs are taken after the chain's last kept sample");
    rc = mmg_sampler_sync(s);   // every sample is final; nothing of the sampler is touched below
    if (rc) return rc;
    HIP_TRY(hipSetDevice(v.p->device));
    std::unique_ptr<mmg_pairs> h(new mmg_pairs());
    DevStream stream;   // (declared first: destroyed after the source's buffers)
    MemberSource src;
    src.from_chain(v, chain);
    HIP_TRY(stream.create(hipStreamNonBlocking));
    rc = build(h.get(), src, stream.get(), n_pairs, a, b);
    if (rc) return rc;
    *out = h.release();
    return MMG_OK;
}

extern "C" int mmg_pairs_of_traces(int device, uint32_t S, uint32_t n_series, const double *traces, uint64_t n_pairs, const uint32_t *a, const uint32_t *b,
                                   mmg_pairs **out)
{
    if (!traces || !out) return fail(MMG_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (S < 1 || n_series < 1) return fail(MMG_ERR_ARG, "S and n_series must be at least 1");
    int rc = check_pairs(n_pairs, a, b, n_series);
    if (rc) return rc;
    rc = require_device(device);
    if (rc) return rc;
    std::unique_ptr<mmg_pairs> h(new mmg_pairs());
    DevStream stream;   // (declared first: destroyed after the source's buffers)
    MemberSource src;
    HIP_TRY(stream.create(hipStreamNonBlocking));
    rc = src.from_host(device, S, n_series, traces);
    if (rc) return rc;
    rc = build(h.get(), src, stream.get(), n_pairs, a, b);
    if (rc) return rc;
    *out = h.release();
    return MMG_OK;
}

extern "C" int mmg_pairs_get(mmg_pairs *h, double *mean_a, double *mean_b, double *mean_sum, double *saa, double *sbb, double *sab, double *sss,
                             uint32_t *n_gt)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL pairs handle");
    const size_t bytes = (size_t)h->P * 8;
    if (mean_a) std::memcpy(mean_a, h->mean_a.data(), bytes);
    if (mean_b) std::memcpy(mean_b, h->mean_b.data(), bytes);
    if (mean_sum) std::memcpy(mean_sum, h->mean_sum.data(), bytes);
    if (saa) std::memcpy(saa, h->saa.data(), bytes);
    if (sbb) std::memcpy(sbb, h->sbb.data(), bytes);
    if (sab) std::memcpy(sab, h->sab.data(), bytes);
    if (sss) std::memcpy(sss, h->sss.data(), bytes);
    if (n_gt) std::memcpy(n_gt, h->n_gt.data(), (size_t)h->P * 4);
    return MMG_OK;
}

extern "C" int mmg_pairs_device_bytes(mmg_pairs *h, uint64_t *bytes)
{
    if (!h || !bytes) return fail(MMG_ERR_ARG, "NULL argument");
    *bytes = h->peak_bytes;
    return MMG_OK;
}

extern "C" void mmg_pairs_destroy(mmg_pairs *h) { delete h; }
