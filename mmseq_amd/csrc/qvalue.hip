// qvalue.hip -- device TU + host side of mmg_qvalues, and the two steps mmg_diff_perm_qvalues (diff.hip) is made of.  Kernels in
// qvalue_kernels.h; the two sorts and the scan are rocPRIM's.
#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include "qvalue_kernels.h"
#include "mmg_host.h"

using namespace mmg;

namespace mmg {

int qvalue_stat_on_device(hipStream_t st, const double *d_st, size_t stride, int gsum, int logitp, uint32_t F, uint32_t R, uint32_t sampled,
                          double *d_stat)
{
    hipLaunchKernelGGL(k_qv_stat, dim3((F + QV_BLOCK - 1) / QV_BLOCK, R), dim3(QV_BLOCK), 0, st, d_st, stride, gsum, logitp, F, (double)sampled, d_stat);
    HIP_TRY(hipGetLastError());
    return MMG_OK;
}

// Working memory, released on return: 40 F + 16 n_null + 16 bytes and what the larger of the two sorts asks for.
int qvalues_on_device(hipStream_t st, uint32_t F, const double *d_obs, uint64_t n_null, const double *d_null, uint64_t *d_null_ge, double *d_q)
{
    DevBuf<uint64_t> okey[2], nkey[2], sizes;
    DevBuf<uint32_t> oidx[2];
    DevBuf<double> fdr, qmin;
    DevBuf<uint8_t> tmp;
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(okey[i].alloc(F));
        HIP_TRY(oidx[i].alloc(F));
        HIP_TRY(nkey[i].alloc(n_null));
    }
    HIP_TRY(sizes.alloc(2));
    const uint64_t n_max = n_null > F ? n_null : F;
    hipLaunchKernelGGL(k_qv_keys, dim3((unsigned)((n_max + QV_BLOCK - 1) / QV_BLOCK)), dim3(QV_BLOCK), 0, st, d_obs, F, d_null, n_null, okey[0].get(),
                       oidx[0].get(), nkey[0].get());
    HIP_TRY(hipGetLastError());
    size_t need_o = 0, need_n = 0, need_s = 0;
    HIP_TRY(rocprim::radix_sort_pairs_desc(nullptr, need_o, okey[0].get(), okey[1].get(), oidx[0].get(), oidx[1].get(), (size_t)F, 0, 64, st));
    HIP_TRY(rocprim::radix_sort_keys(nullptr, need_n, nkey[0].get(), nkey[1].get(), (size_t)n_null, 0, 64, st));
    HIP_TRY(rocprim::inclusive_scan(nullptr, need_s, (double *)nullptr, (double *)nullptr, (size_t)F, QvMin(), st));
    size_t need = need_o > need_n ? need_o : need_n;
    need = need > need_s ? need : need_s;
    HIP_TRY(tmp.alloc(need ? need : 8));
    HIP_TRY(rocprim::radix_sort_pairs_desc(tmp.get(), need_o, okey[0].get(), okey[1].get(), oidx[0].get(), oidx[1].get(), (size_t)F, 0, 64, st));
    HIP_TRY(rocprim::radix_sort_keys(tmp.get(), need_n, nkey[0].get(), nkey[1].get(), (size_t)n_null, 0, 64, st));
    hipLaunchKernelGGL(k_qv_sizes, dim3(1), dim3(64), 0, st, okey[1].get(), F, nkey[1].get(), n_null, sizes.get());
    HIP_TRY(hipGetLastError());
    uint64_t h_sizes[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(h_sizes, sizes.get(), 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint64_t m = h_sizes[0];
    // (the unsorted observed keys are free: V takes their place)
    uint64_t *V = okey[0].get();
    HIP_TRY(fdr.alloc(F));
    HIP_TRY(qmin.alloc(F));
    if (m) {
        hipLaunchKernelGGL(k_qv_estimate, dim3((unsigned)((m + QV_BLOCK - 1) / QV_BLOCK)), dim3(QV_BLOCK), 0, st, okey[1].get(), nkey[1].get(), sizes.get(), V,
                           fdr.get());
        HIP_TRY(hipGetLastError());
        HIP_TRY(rocprim::inclusive_scan(tmp.get(), need_s, fdr.get(), qmin.get(), (size_t)m, QvMin(), st));
    }
    hipLaunchKernelGGL(k_qv_scatter, dim3((F + QV_BLOCK - 1) / QV_BLOCK), dim3(QV_BLOCK), 0, st, oidx[1].get(), F, sizes.get(), V, qmin.get(), d_null_ge, d_q);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return MMG_OK;
}

} // namespace mmg

extern "C" int mmg_qvalues(int device, uint32_t F, const double *obs, uint64_t n_null, const double *null, uint64_t *null_ge, double *q)
{
    if (!obs || !null || !null_ge || !q) return fail(MMG_ERR_ARG, "NULL argument");
    if (F == 0) return fail(MMG_ERR_ARG, "the number of observed values must be positive");
    if (n_null == 0 || n_null > 0x7fffffffu) return fail(MMG_ERR_ARG, "the number of null values must be between 1 and 2147483647");
    const int rc = require_device(device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    DevStream st;
    DevBuf<double> d_obs, d_null, d_q;
    DevBuf<uint64_t> d_ge;
    HIP_TRY(st.create(hipStreamNonBlocking));
    HIP_TRY(d_obs.alloc(F));
    HIP_TRY(d_null.alloc(n_null));
    HIP_TRY(d_q.alloc(F));
    HIP_TRY(d_ge.alloc(F));
    HIP_TRY(hipMemcpyAsync(d_obs.get(), obs, (size_t)F * 8, hipMemcpyHostToDevice, st.get()));
    HIP_TRY(hipMemcpyAsync(d_null.get(), null, (size_t)n_null * 8, hipMemcpyHostToDevice, st.get()));
    const int qrc = qvalues_on_device(st.get(), F, d_obs.get(), n_null, d_null.get(), d_ge.get(), d_q.get());
    if (qrc) { (void)hipStreamSynchronize(st.get()); return qrc; }
    HIP_TRY(hipMemcpy(null_ge, d_ge.get(), (size_t)F * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(q, d_q.get(), (size_t)F * 8, hipMemcpyDeviceToHost));
    return MMG_OK;
}
