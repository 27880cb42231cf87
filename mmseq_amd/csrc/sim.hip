// sim.hip -- device TU + host side of the mmg_sim_* entry points: posterior distances and correlations between S samples from their
// joint draws.  Kernels in sim_kernels.h; specification in tests/sim_ref.py and DESIGN.md section 17.
//
// The handle allocates everything at creation (mmg_sim_device_bytes).  mmg_sim_set_sample uploads one sample's trace into its [T][F]
// block of z and prepares it in place; mmg_sim_run finds the used features, zeroes the others, takes the T Gram matrices on the
// matrix cores in chunks of the feature axis (a partial tile per chunk, added in ascending order), and summarises every pair.
#include "sim_kernels.h"
#include "mmg_host.h"

#include <algorithm>
#include <cmath>
#include <memory>
#include <vector>

using namespace mmg;

// Members are destroyed in reverse declaration order: the destructor waits for `st`, then the buffers go, and the stream last.
struct mmg_sim {
    DevStream st;
    int device = 0;
    uint32_t S = 0, F = 0, T = 0, flags = 0;
    uint32_t NT = 0, NB = 0, CH = 0, chunks = 0, n_ut = 0, pairs = 0;
    DevBuf<double> d_z;                  // [S][T][F]
    DevBuf<double> d_centre, d_ones;     // [F]
    DevBuf<uint8_t> d_mask, d_used;      // [F]
    DevBuf<uint8_t> d_bad;               // [S][F]
    DevBuf<double> d_part;               // [T][chunks][n_ut][256]
    DevBuf<double> d_G, d_m, d_n;        // [T][S][S], [T][S], [T]
    DevBuf<unsigned long long> d_count;  // the used features
    DevBuf<double> d_res;                // [4][pairs]: mean_D, ss_D, mean_R, ss_R
    DevBuf<double> d_q;                  // [2][pairs][SIM_MAX_RANKS]: room for the most ranks a run can ask for
    DevBuf<uint8_t> d_pstatus;           // [pairs]
    DevBuf<uint32_t> d_nn;               // [S][S]
    DevBuf<uint32_t> d_ranks;            // [SIM_MAX_RANKS]
    std::vector<uint8_t> have;           // samples set
    bool ran = false;                    // the last mmg_sim_run succeeded: the getters serve it
    bool zeroed = false;                 // k_sim_zero was launched: z no longer holds what set_sample left
    uint64_t device_bytes = 0, n_used = 0;
    uint32_t nr = 0;
    uint8_t status = 0;
    std::vector<double> res, q;          // the last run's summaries, as the device laid them out
    std::vector<uint8_t> pstatus;
    std::vector<uint32_t> nn;
    ~mmg_sim() { if (st) (void)hipStreamSynchronize(st.get()); }
};

namespace {

inline unsigned blocks256(uint64_t n) { return (unsigned)((n + 255) / 256); }

// features per chunk of the Gram kernel: 4096 (a lane's run is 8 KiB and the four runs of a row lie side by side; at 200 000 features
// and 24 samples 2.4 times faster than two chunks a draw, profiles/mmsim_probe.md, "Chunk length"; the partial tiles are U / (16 S) of the
// draws' bytes, 3 % at two samples and 0.8 % at 24); MMG_OPT_SIM_CHUNK sets the length; at most 65535 chunks (the grid's second dimension)
uint32_t chunk_features(uint32_t F)
{
    const int o = opt(MMG_OPT_SIM_CHUNK);
    uint64_t ch = o > 0 ? (uint64_t)o : 4096;
    ch = std::max<uint64_t>(ch, ((uint64_t)F + 65534) / 65535);
    return (uint32_t)std::min<uint64_t>(ch, F);
}

} // namespace

extern "C" int mmg_sim_create(int device, uint32_t S, uint32_t F, uint32_t T, const double *centre, const uint8_t *mask, uint32_t flags, mmg_sim **out)
{
    if (!out) return fail(MMG_ERR_ARG, "NULL argument (out)");
    *out = nullptr;
    if (S < 2 || S > SIM_MAX_S) return fail(MMG_ERR_ARG, "S = " + std::to_string(S) + " is outside 2 .. " + std::to_string(SIM_MAX_S));
    if (F < 1 || F > 0x7fffffffu) return fail(MMG_ERR_ARG, "F = " + std::to_string(F) + " is outside 1 .. 2^31 - 1");
    if (T < 1 || T > SIM_MAX_T) return fail(MMG_ERR_ARG, "T = " + std::to_string(T) + " is outside 1 .. " + std::to_string(SIM_MAX_T));
    if (flags & ~(uint32_t)MMG_SIM_LOGGED) return fail(MMG_ERR_ARG, "flags = " + std::to_string(flags) + " has bits other than MMG_SIM_LOGGED");
    if (centre)
        for (uint32_t f = 0; f < F; ++f)
            if (!std::isfinite(centre[f])) return fail(MMG_ERR_ARG, "centre[" + std::to_string(f) + "] is not finite");
    int rc = require_device(device);
    if (rc) return rc;
    std::unique_ptr<mmg_sim> h(new mmg_sim());
    h->device = device; h->S = S; h->F = F; h->T = T; h->flags = flags;
    h->NT = (S + 1 + SIM_TILE - 1) / SIM_TILE;
    h->NB = (h->NT + SIM_BT - 1) / SIM_BT;
    h->n_ut = h->NT * (h->NT + 1) / 2;
    h->pairs = S * (S - 1) / 2;
    h->CH = chunk_features(F);
    h->chunks = (uint32_t)(((uint64_t)F + h->CH - 1) / h->CH);
    h->have.assign(S, 0);
    const uint64_t Su = S, Fu = F, Tu = T, P = h->pairs;
    const uint64_t z_bytes = 8 * Su * Tu * Fu;
    const uint64_t need = z_bytes + 8 * Fu * 2 + Fu * 2 + Su * Fu + 8 * Tu * h->chunks * h->n_ut * SIM_TILE_WORDS + 8 * Tu * (Su * Su + Su + 1) + 8 +
                          P * (32 + 16 * (uint64_t)SIM_MAX_RANKS + 1) + 4 * Su * Su + 4 * (uint64_t)SIM_MAX_RANKS;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (need > (uint64_t)free_b)
        return fail(MMG_ERR_ARG, "S * T * F * 8 = " + std::to_string(z_bytes) + " bytes of draws and " + std::to_string(need - z_bytes) + " of results (" +
                                     std::to_string(need) + " in all) do not fit the device's free memory of " + std::to_string((uint64_t)free_b) + " bytes");
    auto dalloc = [&](auto &buf, uint64_t count) {
        HIPE_TRY(buf.alloc(count));
        h->device_bytes += count * sizeof(*buf.get());
        return hipSuccess;
    };
    HIP_TRY(h->st.create(hipStreamNonBlocking));
    HIP_TRY(dalloc(h->d_z, Su * Tu * Fu));
    HIP_TRY(dalloc(h->d_centre, Fu));
    HIP_TRY(dalloc(h->d_ones, Fu));
    HIP_TRY(dalloc(h->d_mask, Fu));
    HIP_TRY(dalloc(h->d_used, Fu));
    HIP_TRY(dalloc(h->d_bad, Su * Fu));
    HIP_TRY(dalloc(h->d_part, Tu * h->chunks * h->n_ut * SIM_TILE_WORDS));
    HIP_TRY(dalloc(h->d_G, Tu * Su * Su));
    HIP_TRY(dalloc(h->d_m, Tu * Su));
    HIP_TRY(dalloc(h->d_n, Tu));
    HIP_TRY(dalloc(h->d_count, 1));
    HIP_TRY(dalloc(h->d_res, 4 * P));
    HIP_TRY(dalloc(h->d_q, 2 * P * SIM_MAX_RANKS));
    HIP_TRY(dalloc(h->d_pstatus, P));
    HIP_TRY(dalloc(h->d_nn, Su * Su));
    HIP_TRY(dalloc(h->d_ranks, SIM_MAX_RANKS));
    hipStream_t st = h->st.get();
    if (centre) HIP_TRY(hipMemcpyAsync(h->d_centre.get(), centre, 8 * Fu, hipMemcpyHostToDevice, st));
    else HIP_TRY(hipMemsetAsync(h->d_centre.get(), 0, 8 * Fu, st));
    if (mask) HIP_TRY(hipMemcpyAsync(h->d_mask.get(), mask, Fu, hipMemcpyHostToDevice, st));
    else HIP_TRY(hipMemsetAsync(h->d_mask.get(), 1, Fu, st));
    HIP_TRY(hipStreamSynchronize(st));   // (the caller's arrays were the sources of asynchronous copies)
    *out = h.release();
    return MMG_OK;
}

extern "C" int mmg_sim_set_sample(mmg_sim *h, uint32_t s, const double *trace, double off)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL sim handle");
    if (!trace) return fail(MMG_ERR_ARG, "NULL argument (trace)");
    if (s >= h->S) return fail(MMG_ERR_ARG, "s = " + std::to_string(s) + " is not below S = " + std::to_string(h->S));
    if (!std::isfinite(off)) return fail(MMG_ERR_ARG, "off must be finite");
    if (h->ran || h->zeroed) return fail(MMG_ERR_STATE, "mmg_sim_run has run: the unused features of every sample are zeroed");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = h->st.get();
    const uint64_t F = h->F, T = h->T;
    double *const z = h->d_z.get() + (uint64_t)s * T * F;
    uint8_t *const bad = h->d_bad.get() + (uint64_t)s * F;
    HIP_TRY(hipMemsetAsync(bad, 0, F, st));
    HIP_TRY(hipMemcpyAsync(z, trace, 8 * T * F, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_sim_prepare, dim3(blocks256(F), h->T), dim3(256), 0, st, h->F, z, off, (const double *)h->d_centre.get(),
                       h->flags & MMG_SIM_LOGGED, bad);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));   // (the caller's trace was the source of an asynchronous copy)
    h->have[s] = 1;
    return MMG_OK;
}

extern "C" int mmg_sim_run(mmg_sim *h, uint32_t n_ranks, const uint32_t *ranks)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL sim handle");
    if (n_ranks > SIM_MAX_RANKS) return fail(MMG_ERR_ARG, "n_ranks = " + std::to_string(n_ranks) + " is more than " + std::to_string(SIM_MAX_RANKS));
    if (n_ranks && !ranks) return fail(MMG_ERR_ARG, "ranks is NULL with n_ranks > 0");
    for (uint32_t s = 0; s < h->S; ++s)
        if (!h->have[s]) return fail(MMG_ERR_STATE, "mmg_sim_run before sample " + std::to_string(s) + " was set");
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = h->st.get();
    const uint32_t S = h->S, F = h->F, T = h->T, P = h->pairs;
    h->ran = false;   // (until this run has succeeded: a failed one leaves nothing for the getters)
    // ---- the used features; the others leave every row
    unsigned long long count = 0;
    HIP_TRY(hipMemsetAsync(h->d_count.get(), 0, 8, st));
    hipLaunchKernelGGL(k_sim_used, dim3(blocks256(F)), dim3(256), 0, st, F, S, (const uint8_t *)h->d_mask.get(), (const uint8_t *)h->d_bad.get(),
                       h->d_used.get(), h->d_ones.get(), h->d_count.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&count, h->d_count.get(), 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (!h->zeroed && count < F) {
        h->zeroed = true;
        hipLaunchKernelGGL(k_sim_zero, dim3(blocks256(F), (S * T + 63) / 64), dim3(256), 0, st, F, S * T, (const uint8_t *)h->d_used.get(), h->d_z.get());
        HIP_TRY(hipGetLastError());
    }
    h->n_used = count;
    // ---- stage 1: the Gram matrices
    hipLaunchKernelGGL(k_sim_gram, dim3(h->NB * (h->NB + 1) / 2, h->chunks, T), dim3(256), 0, st, S, T, F, h->NT, h->NB, h->CH,
                       (const double *)h->d_z.get(), (const double *)h->d_ones.get(), h->d_part.get());
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_sim_reduce, dim3(h->n_ut, T), dim3(256), 0, st, S, h->NT, h->chunks, (const double *)h->d_part.get(), h->d_G.get(),
                       h->d_m.get(), h->d_n.get());
    HIP_TRY(hipGetLastError());
    std::vector<double> n_of(T);
    HIP_TRY(hipMemcpyAsync(n_of.data(), h->d_n.get(), 8 * (size_t)T, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (uint32_t t = 0; t < T; ++t)   // the ones' own product is the count, exactly: anything else is a wrong lane map
        if (n_of[t] != (double)count)
            return fail(MMG_ERR_STATE, "draw " + std::to_string(t) + ": the Gram kernel counted " + std::to_string(n_of[t]) + " used features, there are " +
                                           std::to_string(count));
    // ---- stage 2: every pair over the draws
    h->nr = n_ranks;
    const double nan = std::nan("");
    h->res.assign(4 * (size_t)P, nan);
    h->q.assign(2 * (size_t)P * n_ranks, nan);
    h->pstatus.assign(P, 0);
    h->nn.assign((size_t)S * S, 0);
    h->status = count < 2 ? SIM_FEW_FEATURES : 0;
    if (h->status) { h->ran = true; return MMG_OK; }
    if (n_ranks) HIP_TRY(hipMemcpyAsync(h->d_ranks.get(), ranks, 4 * (size_t)n_ranks, hipMemcpyHostToDevice, st));
    const uint32_t PT = next_pow2(T);
    const size_t lds = 16 * (size_t)PT;
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_sim_pair), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    SimOut o;
    o.mean_D = h->d_res.get(); o.ss_D = o.mean_D + P; o.mean_R = o.ss_D + P; o.ss_R = o.mean_R + P;
    o.q_D = h->d_q.get(); o.q_R = o.q_D + (size_t)P * n_ranks;
    o.pair_status = h->d_pstatus.get();
    hipLaunchKernelGGL(k_sim_pair, dim3(P), dim3(SIM_PAIR_BLOCK), lds, st, S, T, PT, (double)count, (const double *)h->d_G.get(), (const double *)h->d_m.get(),
                       n_ranks, (const uint32_t *)h->d_ranks.get(), o);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(h->d_nn.get(), 0, 4 * (size_t)S * S, st));
    hipLaunchKernelGGL(k_sim_nn, dim3(blocks256((uint64_t)S * T)), dim3(256), 0, st, S, T, (const double *)h->d_G.get(), h->d_nn.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->res.data(), h->d_res.get(), 32 * (size_t)P, hipMemcpyDeviceToHost, st));
    if (n_ranks) HIP_TRY(hipMemcpyAsync(h->q.data(), h->d_q.get(), 16 * (size_t)P * n_ranks, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h->pstatus.data(), h->d_pstatus.get(), P, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h->nn.data(), h->d_nn.get(), 4 * (size_t)S * S, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    h->ran = true;
    return MMG_OK;
}

extern "C" int mmg_sim_get_used(mmg_sim *h, uint8_t *used, uint64_t *n)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL sim handle");
    if (!h->ran) return fail(MMG_ERR_STATE, "mmg_sim_run has not run");
    if (n) *n = h->n_used;
    if (!used) return MMG_OK;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(used, h->d_used.get(), h->F, hipMemcpyDeviceToHost, h->st.get()));
    HIP_TRY(hipStreamSynchronize(h->st.get()));
    return MMG_OK;
}

extern "C" int mmg_sim_get_z(mmg_sim *h, uint32_t s, uint32_t first_draw, uint32_t n_draws, double *out)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL sim handle");
    if (s >= h->S) return fail(MMG_ERR_ARG, "s = " + std::to_string(s) + " is not below S = " + std::to_string(h->S));
    if ((uint64_t)first_draw + n_draws > h->T) return fail(MMG_ERR_ARG, "draws first_draw .. first_draw + n_draws are not all below T = " + std::to_string(h->T));
    if (n_draws && !out) return fail(MMG_ERR_ARG, "NULL argument (out)");
    if (!h->have[s]) return fail(MMG_ERR_STATE, "sample " + std::to_string(s) + " is not set");
    if (!n_draws) return MMG_OK;
    HIP_TRY(hipSetDevice(h->device));
    const uint64_t F = h->F;
    HIP_TRY(hipMemcpyAsync(out, h->d_z.get() + ((uint64_t)s * h->T + first_draw) * F, 8 * (uint64_t)n_draws * F, hipMemcpyDeviceToHost, h->st.get()));
    HIP_TRY(hipStreamSynchronize(h->st.get()));
    return MMG_OK;
}

extern "C" int mmg_sim_get_gram(mmg_sim *h, uint32_t first_draw, uint32_t n_draws, double *G, double *m)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL sim handle");
    if ((uint64_t)first_draw + n_draws > h->T) return fail(MMG_ERR_ARG, "draws first_draw .. first_draw + n_draws are not all below T = " + std::to_string(h->T));
    if (!h->ran) return fail(MMG_ERR_STATE, "mmg_sim_run has not run");
    if (!n_draws) return MMG_OK;
    HIP_TRY(hipSetDevice(h->device));
    const uint64_t S = h->S;
    if (G) HIP_TRY(hipMemcpyAsync(G, h->d_G.get() + (uint64_t)first_draw * S * S, 8 * (uint64_t)n_draws * S * S, hipMemcpyDeviceToHost, h->st.get()));
    if (m) HIP_TRY(hipMemcpyAsync(m, h->d_m.get() + (uint64_t)first_draw * S, 8 * (uint64_t)n_draws * S, hipMemcpyDeviceToHost, h->st.get()));
    HIP_TRY(hipStreamSynchronize(h->st.get()));
    return MMG_OK;
}

extern "C" int mmg_sim_get(mmg_sim *h, double *mean_D, double *ss_D, double *q_D, double *mean_R, double *ss_R, double *q_R, uint32_t *nn,
                           uint8_t *pair_status, uint8_t *status)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL sim handle");
    if (!h->ran) return fail(MMG_ERR_STATE, "mmg_sim_run has not run");
    const size_t P = h->pairs, pb = P * 8, qn = P * h->nr;
    if (mean_D) std::memcpy(mean_D, h->res.data(), pb);
    if (ss_D) std::memcpy(ss_D, h->res.data() + P, pb);
    if (mean_R) std::memcpy(mean_R, h->res.data() + 2 * P, pb);
    if (ss_R) std::memcpy(ss_R, h->res.data() + 3 * P, pb);
    if (q_D && qn) std::memcpy(q_D, h->q.data(), qn * 8);
    if (q_R && qn) std::memcpy(q_R, h->q.data() + qn, qn * 8);
    if (nn) std::memcpy(nn, h->nn.data(), 4 * (size_t)h->S * h->S);
    if (pair_status) std::memcpy(pair_status, h->pstatus.data(), P);
    if (status) *status = h->status;
    return MMG_OK;
}

extern "C" int mmg_sim_device_bytes(mmg_sim *h, uint64_t *bytes)
{
    if (!h || !bytes) return fail(MMG_ERR_ARG, "NULL argument");
    *bytes = h->device_bytes;
    return MMG_OK;
}

extern "C" void mmg_sim_destroy(mmg_sim *h) { delete h; }
