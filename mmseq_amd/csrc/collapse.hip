// collapse.hip -- device TU + host side of the mmg_collapse_* entry points: mmcollapse's correlations and greedy loop
// (src/mmcollapse.cpp:483-561, :713-747, :758-819, collapse() at :398-441).  Kernels in collapse_kernels.h.
#include "collapse_kernels.h"
#include "mmg_host.h"

#include <vector>

using namespace mmg;

struct mmg_collapse {
    int device = 0;
    uint32_t S = 0, C = 0, Cp = 0, N = 0;
    double *d_X = nullptr;       // [S][N][Cp] centred traces (merged candidates: the sum of their members')
    double *d_var = nullptr;     // [S][Cp]
    double *d_cov = nullptr;     // [S][Cp] the merged row's covariances of one iteration
    uint8_t *d_obs = nullptr;    // [S][Cp]
    double *d_V = nullptr;       // [Cp][Cp]
    double *d_rowmax = nullptr, *d_cmin = nullptr;
    uint32_t *d_carg = nullptr;
    uint8_t *d_dead = nullptr, *d_flag = nullptr;
    ClPick *d_pick = nullptr;
    std::vector<uint8_t> have;   // samples uploaded
    bool correlated = false, stopped = false;
    uint64_t device_bytes = 0;
    hipStream_t st = nullptr;
};

static void collapse_free(mmg_collapse *h)
{
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->st) (void)hipStreamSynchronize(h->st);
    for (void *x : {(void *)h->d_X, (void *)h->d_var, (void *)h->d_cov, (void *)h->d_obs, (void *)h->d_V, (void *)h->d_rowmax,
                    (void *)h->d_cmin, (void *)h->d_carg, (void *)h->d_dead, (void *)h->d_flag, (void *)h->d_pick})
        if (x) (void)hipFree(x);
    if (h->st) (void)hipStreamDestroy(h->st);
    delete h;
}

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
    mmg_collapse *h = new mmg_collapse();
    h->device = device; h->S = n_samples; h->C = n_cand; h->N = trace_len;
    h->Cp = (uint32_t)(((uint64_t)n_cand + CL_CT - 1) / CL_CT * CL_CT);
    if (h->Cp == 0) h->Cp = CL_CT;
    h->have.assign(n_samples, 0);
    const uint64_t Cp = h->Cp, S = n_samples, N = trace_len;
    auto bail = [&](int code) { collapse_free(h); return code; };
#define C_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return bail(fail(MMG_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e))); } while (0)
    auto dalloc = [&](void **p, uint64_t bytes) {
        hipError_t e = hipMalloc(p, bytes);
        if (e == hipSuccess) { h->device_bytes += bytes; e = hipMemsetAsync(*p, 0, bytes, h->st); }
        return e;
    };
    C_TRY(hipStreamCreateWithFlags(&h->st, hipStreamNonBlocking));
    C_TRY(dalloc((void **)&h->d_X, S * N * Cp * 8));
    C_TRY(dalloc((void **)&h->d_var, S * Cp * 8));
    C_TRY(dalloc((void **)&h->d_cov, S * Cp * 8));
    C_TRY(dalloc((void **)&h->d_obs, S * Cp));
    C_TRY(dalloc((void **)&h->d_V, Cp * Cp * 8));
    C_TRY(dalloc((void **)&h->d_rowmax, Cp * 8));
    C_TRY(dalloc((void **)&h->d_cmin, Cp * 8));
    C_TRY(dalloc((void **)&h->d_carg, Cp * 4));
    C_TRY(dalloc((void **)&h->d_dead, Cp));
    C_TRY(dalloc((void **)&h->d_flag, Cp));
    C_TRY(dalloc((void **)&h->d_pick, sizeof(ClPick)));
    // the mask, transposed to [S][Cp] (padding columns unobserved)
    std::vector<uint8_t> obs(S * Cp, 0);
    for (uint64_t c = 0; c < n_cand; ++c)
        for (uint64_t s = 0; s < S; ++s) obs[s * Cp + c] = observed[c * S + s] ? 1 : 0;
    C_TRY(hipMemcpyAsync(h->d_obs, obs.data(), obs.size(), hipMemcpyHostToDevice, h->st));
    C_TRY(hipStreamSynchronize(h->st));
#undef C_TRY
    *out = h;
    return MMG_OK;
}

extern "C" int mmg_collapse_set_sample(mmg_collapse *h, uint32_t sample, const double *trace)
{
    if (!h || (h->C && !trace)) return fail(MMG_ERR_ARG, "NULL argument");
    if (sample >= h->S) return fail(MMG_ERR_ARG, "sample index out of range");
    if (h->correlated) return fail(MMG_ERR_STATE, "the correlations are computed already");
    HIP_TRY(hipSetDevice(h->device));
    double *X = h->d_X + (uint64_t)sample * h->N * h->Cp;
    if (h->C) {
        HIP_TRY(hipMemcpy2DAsync(X, (size_t)h->Cp * 8, trace, (size_t)h->C * 8, (size_t)h->C * 8, h->N, hipMemcpyHostToDevice, h->st));
        hipLaunchKernelGGL(k_cl_center, dim3(cl_blocks(h->C)), dim3(256), 0, h->st, h->N, h->Cp, h->C, X);
    }
    hipLaunchKernelGGL(k_cl_var, dim3(cl_blocks(h->Cp)), dim3(256), 0, h->st, h->N, h->Cp, (const double *)X, h->d_var + (uint64_t)sample * h->Cp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->st));   // (the caller's trace was the source of an asynchronous copy)
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
    hipLaunchKernelGGL(k_cl_corr_tiles, dim3(nt, nt), dim3(256), 0, h->st, h->N, h->Cp, h->S, (const double *)h->d_X,
                       (const double *)h->d_var, (const uint8_t *)h->d_obs, h->d_V);
    if (h->C) hipLaunchKernelGGL(k_cl_scan, dim3(h->C), dim3(256), 0, h->st, h->C, h->Cp, (const double *)h->d_V, (uint8_t *)nullptr, h->d_cmin, h->d_carg, h->d_rowmax);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->st));
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
    HIP_TRY(hipMemcpy2DAsync(out, (size_t)h->C * 8, h->d_V + (uint64_t)first * h->Cp, (size_t)h->Cp * 8, (size_t)h->C * 8, count,
                             hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
    return MMG_OK;
}

extern "C" int mmg_collapse_row_max(mmg_collapse *h, double *out)
{
    if (!h || (h->C && !out)) return fail(MMG_ERR_ARG, "NULL argument");
    if (!h->correlated) return fail(MMG_ERR_STATE, "mmg_collapse_correlate has not run");
    if (!h->C) return MMG_OK;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpyAsync(out, h->d_rowmax, (size_t)h->C * 8, hipMemcpyDeviceToHost, h->st));
    HIP_TRY(hipStreamSynchronize(h->st));
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
    hipStream_t st = h->st;
    uint32_t done = 0;
    while (done < max_merges) {
        hipLaunchKernelGGL(k_cl_global_min, dim3(1), dim3(1024), 0, st, h->C, (const double *)h->d_cmin, (const uint32_t *)h->d_carg, h->d_pick);
        HIP_TRY(hipGetLastError());
        ClPick pk;
        HIP_TRY(hipMemcpyAsync(&pk, h->d_pick, sizeof pk, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (pk.col == CL_NONE || !(pk.value < thr)) { h->stopped = true; break; }
        const uint32_t a = pk.row < pk.col ? pk.row : pk.col, b = pk.row < pk.col ? pk.col : pk.row;
        if (a == b || b >= h->C) return fail(MMG_ERR_STATE, "collapse: the minimum of V sits on the diagonal or out of range");
        hipLaunchKernelGGL(k_cl_merge, dim3(cl_blocks((uint64_t)h->S * h->N)), dim3(256), 0, st, h->N, h->Cp, h->S, a, b, h->d_X, h->d_dead);
        hipLaunchKernelGGL(k_cl_row_cov, dim3(cl_blocks(h->Cp), h->S), dim3(256), 0, st, h->N, h->Cp, a, (const double *)h->d_X, h->d_cov);
        hipLaunchKernelGGL(k_cl_row_update, dim3(cl_blocks(h->C)), dim3(256), 0, st, h->C, h->Cp, h->S, a, b, (const double *)h->d_cov, h->d_var,
                           (const uint8_t *)h->d_obs, (const uint8_t *)h->d_dead, h->d_V, h->d_cmin, h->d_carg, h->d_flag);
        hipLaunchKernelGGL(k_cl_scan, dim3(h->C), dim3(256), 0, st, h->C, h->Cp, (const double *)h->d_V, h->d_flag, h->d_cmin, h->d_carg, (double *)nullptr);
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

extern "C" void mmg_collapse_destroy(mmg_collapse *h) { collapse_free(h); }
