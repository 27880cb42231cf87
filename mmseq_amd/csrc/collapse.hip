// collapse.hip -- device TU + host side of the mmg_collapse_* entry points: mmcollapse's correlations and greedy loop
// (src/mmcollapse.cpp:483-561, :713-747, :758-819, collapse() at :398-441).  Kernels in collapse_kernels.h.
#include "collapse_kernels.h"
#include "mmg_host.h"

#include <memory>
#include <vector>

using namespace mmg;

// Members are destroyed in reverse declaration order: the destructor waits for `st`, then the buffers go, and the stream last.
struct mmg_collapse {
    DevStream st;
    int device = 0;
    uint32_t S = 0, C = 0, Cp = 0, N = 0;
    DevBuf<double> d_X;          // [S][N][Cp] centred traces (merged candidates: the sum of their members')
    DevBuf<double> d_var;        // [S][Cp]
    DevBuf<double> d_cov;        // [S][Cp] the merged row's covariances of one iteration
    DevBuf<uint8_t> d_obs;       // [S][Cp]
    DevBuf<double> d_V;          // [Cp][Cp]
    DevBuf<double> d_rowmax, d_cmin;
    DevBuf<uint32_t> d_carg;
    DevBuf<uint8_t> d_dead, d_flag;
    DevBuf<ClPick> d_pick;
    std::vector<uint8_t> have;   // samples uploaded
    bool correlated = false, stopped = false;
    uint64_t device_bytes = 0;
    ~mmg_collapse() { if (st) (void)hipStreamSynchronize(st.get()); }
};

static inline unsigned cl_blocks(uint64_t n) { return (unsigned)((n + 255) / 256); }

extern "C" int mmg_collapse_create(int device, uint32_t n_samples, uint32_t n_cand, uint32_t trace_len, const uint8_t *observed,
                                   mmg_collapse **out)
{
    if (!out || (n_cand && !observed)) return fail(MMG_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (n_samples == 0) return fail(MMG_ERR_ARG, "n_samples must be at least 1");
    if (trace_len < CL_KT || trace_len % CL_KT) return fail(MMG_ERR_ARG, "trace_len must be a positive multiple of 16");
    if (n_cand > 0x7fffff00u) return fail(MMG_ERR_ARG, "too many candidates");
    int rc = require_device(device);
    if (rc) return rc;
    std::unique_ptr<mmg_collapse> h(new mmg_collapse());
    h->device = device; h->S = n_samples; h->C = n_cand; h->N = trace_len;
    h->Cp = (uint32_t)(((uint64_t)n_cand + CL_CT - 1) / CL_CT * CL_CT);
    if (h->Cp == 0) h->Cp = CL_CT;
    h->have.assign(n_samples, 0);
    const uint64_t Cp = h->Cp, S = n_samples, N = trace_len;
    auto dalloc = [&](auto &buf, uint64_t count) { // zeroed on the handle's stream
        HIPE_TRY(buf.alloc(count));
        const uint64_t bytes = count * sizeof(*buf.get());
        h->device_bytes += bytes;
        return hipMemsetAsync(buf.get(), 0, bytes, h->st.get());
    };
    HIP_TRY(h->st.create(hipStreamNonBlocking));
    HIP_TRY(dalloc(h->d_X, S * N * Cp));
    HIP_TRY(dalloc(h->d_var, S * Cp));
    HIP_TRY(dalloc(h->d_cov, S * Cp));
    HIP_TRY(dalloc(h->d_obs, S * Cp));
    HIP_TRY(dalloc(h->d_V, Cp * Cp));
    HIP_TRY(dalloc(h->d_rowmax, Cp));
    HIP_TRY(dalloc(h->d_cmin, Cp));
    HIP_TRY(dalloc(h->d_carg, Cp));
    HIP_TRY(dalloc(h->d_dead, Cp));
    HIP_TRY(dalloc(h->d_flag, Cp));
    HIP_TRY(dalloc(h->d_pick, 1));
    // the mask, transposed to [S][Cp] (padding columns unobserved)
    std::vector<uint8_t> obs(S * Cp, 0);
    for (uint64_t c = 0; c < n_cand; ++c)
        for (uint64_t s = 0; s < S; ++s) obs[s * Cp + c] = observed[c * S + s] ? 1 : 0;
    HIP_TRY(hipMemcpyAsync(h->d_obs.get(), obs.data(), obs.size(), hipMemcpyHostToDevice, h->st.get()));
    HIP_TRY(hipStreamSynchronize(h->st.get()));
    *out = h.release();
    return MMG_OK;
}

extern "C" int mmg_collapse_set_sample(mmg_collapse *h, uint32_t sample, const double *trace)
{
    if (!h || (h->C && !trace)) return fail(MMG_ERR_ARG, "NULL argument");
    if (sample >= h->S) return fail(MMG_ERR_ARG, "sample index out of range");
    if (h->correlated) return fail(MMG_ERR_STATE, "the correlations are computed already");
    HIP_TRY(hipSetDevice(h->device));
    double *X = h->d_X.get() + (uint64_t)sample * h->N * h->Cp;
    if (h->C) {
        HIP_TRY(hipMemcpy2DAsync(X, (size_t)h->Cp * 8, trace, (size_t)h->C * 8, (size_t)h->C * 8, h->N, hipMemcpyHostToDevice, h->st.get()));
        hipLaunchKernelGGL(k_cl_center, dim3(cl_blocks(h->C)), dim3(256), 0, h->st.get(), h->N, h->Cp, h->C, X);
    }
    hipLaunchKernelGGL(k_cl_var, dim3(cl_blocks(h->Cp)), dim3(256), 0, h->st.get(), h->N, h->Cp, (const double *)X, h->d_var.get() + (uint64_t)sample * h->Cp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->st.get()));   // (the caller's trace was the source of an asynchronous copy)
    h->have[sample] = 1;
    return MMG_OK;
}

extern "C" int mmg_collapse_correlate(mmg_collapse *h)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL argument");
    if (h->correlated) return MMG_OK;
    for (uint8_t x : h->have) if (!x) return fail(MMG_ERR_STATE, "mmg_collapse_correlate before every sample was set");
    HIP_TRY(hipSetDevice(h->device));
    const unsigned nt = h->Cp / CL_CT;
    hipLaunchKernelGGL(k_cl_corr_tiles, dim3(nt, nt), dim3(256), 0, h->st.get(), h->N, h->Cp, h->S, (const double *)h->d_X.get(),
                       (const double *)h->d_var.get(), (const uint8_t *)h->d_obs.get(), h->d_V.get());
    if (h->C) hipLaunchKernelGGL(k_cl_scan, dim3(h->C), dim3(256), 0, h->st.get(), h->C, h->Cp, (const double *)h->d_V.get(), (uint8_t *)nullptr, h->d_cmin.get(), h->d_carg.get(), h->d_rowmax.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->st.get()));
    h->correlated = true;
    return MMG_OK;
}

extern "C" int mmg_collapse_get_rows(mmg_collapse *h, uint32_t first, uint32_t count, double *out)
{
    if (!h || (count && !out)) return fail(MMG_ERR_ARG, "NULL argument");
    if (!h->correlated) return fail(MMG_ERR_STATE, "mmg_collapse_correlate has not run");
    if ((uint64_t)first + count > h->C) return fail(MMG_ERR_ARG, "rows out of range");
    if (!count || !h->C) return MMG_OK;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpy2DAsync(out, (size_t)h->C * 8, h->d_V.get() + (uint64_t)first * h->Cp, (size_t)h->Cp * 8, (size_t)h->C * 8, count,
                             hipMemcpyDeviceToHost, h->st.get()));
    HIP_TRY(hipStreamSynchronize(h->st.get()));
    return MMG_OK;
}

extern "C" int mmg_collapse_row_max(mmg_collapse *h, double *out)
{
    if (!h || (h->C && !out)) return fail(MMG_ERR_ARG, "NULL argument");
    if (!h->correlated) return fail(MMG_ERR_STATE, "mmg_collapse_correlate has not run");
    if (!h->C) return MMG_OK;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(out, h->d_rowmax.get(), (size_t)h->C * 8, hipMemcpyDeviceToHost, h->st.get()));
    HIP_TRY(hipStreamSynchronize(h->st.get()));
    return MMG_OK;
}

// One merge per iteration while the minimum of V is below thr (:758-819).  Per iteration: the minimum over the column minima, the
// merge of the traces (S N entries), the merged row's covariances (S N Cp fma), the row / column update, rescans of the flagged
// columns; 24 bytes come back to the host.  Returns after max_merges merges or at the stop; a later call continues.
extern "C" int mmg_collapse_run(mmg_collapse *h, double thr, uint32_t max_merges, uint32_t *pairs, double *values, uint32_t *n_merges,
                                int32_t *stopped)
{
    if (!h || !n_merges || (max_merges && (!pairs || !values))) return fail(MMG_ERR_ARG, "NULL argument");
    if (!h->correlated) return fail(MMG_ERR_STATE, "mmg_collapse_correlate has not run");
    *n_merges = 0;
    if (stopped) *stopped = h->stopped;
    if (h->stopped || !h->C) { h->stopped = true; if (stopped) *stopped = 1; return MMG_OK; }
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t st = h->st.get();
    uint32_t done = 0;
    while (done < max_merges) {
        hipLaunchKernelGGL(k_cl_global_min, dim3(1), dim3(1024), 0, st, h->C, (const double *)h->d_cmin.get(), (const uint32_t *)h->d_carg.get(), h->d_pick.get());
        HIP_TRY(hipGetLastError());
        ClPick pk;
        HIP_TRY(hipMemcpyAsync(&pk, h->d_pick.get(), sizeof pk, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (pk.col == CL_NONE || !(pk.value < thr)) { h->stopped = true; break; }
        const uint32_t a = pk.row < pk.col ? pk.row : pk.col, b = pk.row < pk.col ? pk.col : pk.row;
        if (a == b || b >= h->C) return fail(MMG_ERR_STATE, "collapse: the minimum of V sits on the diagonal or out of range");
        hipLaunchKernelGGL(k_cl_merge, dim3(cl_blocks((uint64_t)h->S * h->N)), dim3(256), 0, st, h->N, h->Cp, h->S, a, b, h->d_X.get(), h->d_dead.get());
        hipLaunchKernelGGL(k_cl_row_cov, dim3(cl_blocks(h->Cp), h->S), dim3(256), 0, st, h->N, h->Cp, a, (const double *)h->d_X.get(), h->d_cov.get());
        hipLaunchKernelGGL(k_cl_row_update, dim3(cl_blocks(h->C)), dim3(256), 0, st, h->C, h->Cp, h->S, a, b, (const double *)h->d_cov.get(), h->d_var.get(),
                           (const uint8_t *)h->d_obs.get(), (const uint8_t *)h->d_dead.get(), h->d_V.get(), h->d_cmin.get(), h->d_carg.get(), h->d_flag.get());
        hipLaunchKernelGGL(k_cl_scan, dim3(h->C), dim3(256), 0, st, h->C, h->Cp, (const double *)h->d_V.get(), h->d_flag.get(), h->d_cmin.get(), h->d_carg.get(), (double *)nullptr);
        HIP_TRY(hipGetLastError());
        pairs[2 * done] = a;
        pairs[2 * done + 1] = b;
        values[done] = pk.value;
        ++done;
    }
    HIP_TRY(hipStreamSynchronize(st));
    *n_merges = done;
    if (stopped) *stopped = h->stopped;
    return MMG_OK;
}

extern "C" int mmg_collapse_device_bytes(mmg_collapse *h, uint64_t *bytes)
{
    if (!h || !bytes) return fail(MMG_ERR_ARG, "NULL argument");
    *bytes = h->device_bytes;
    return MMG_OK;
}

extern "C" void mmg_collapse_destroy(mmg_collapse *h) { delete h; }
