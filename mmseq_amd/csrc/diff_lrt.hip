// diff_lrt.hip -- device TU + host side of the mmg_diff_lrt_* entry points: mmdiff's per-feature likelihood-ratio test
// (DESIGN.md section 10.5).  Kernels in diff_lrt_kernels.h; the p- and q-values in host/lrt_stats.hpp.
#include "diff_lrt_host.h"
#include "host/lrt_stats.hpp"

#include <cmath>
#include <memory>
#include <vector>

using namespace mmg;

// X_m = [1 unless fixalpha | M unless nil | P_m unless nil], [N][p]
static std::vector<double> lrt_design(uint32_t N, bool fixalpha, bool Mnil, uint32_t K, const double *M, bool Pnil, uint32_t L, const double *P,
                                      uint32_t *p_out)
{
    const uint32_t p = (fixalpha ? 0 : 1) + (Mnil ? 0 : K) + (Pnil ? 0 : L);
    std::vector<double> X((size_t)N * p);
    for (uint32_t i = 0; i < N; ++i) {
        double *row = X.data() + (size_t)i * p;
        if (!fixalpha) *row++ = 1.0;
        if (!Mnil) for (uint32_t k = 0; k < K; ++k) *row++ = M[(size_t)i * K + k];
        if (!Pnil) for (uint32_t l = 0; l < L; ++l) *row++ = P[(size_t)i * L + l];
    }
    *p_out = p;
    return X;
}

namespace mmg {

int lrt_check_args(int device, uint32_t F, uint32_t N, const double *y, const double *e, uint32_t K, const double *M, uint32_t L0, const double *P0,
                   uint32_t L1, const double *P1, const int32_t *C, int nc[2])
{
    // (the caps are mmg_diff_create's: the static_assert of diff.hip)
    int rc;
    if ((rc = df_check_shape(F, N, K)) || (rc = df_check_cols(L0, 1, &L1)) || (rc = df_check_finite(F, N, y, e, K, M, L0, P0, L1, P1))
        || (rc = df_check_classes(C, N, nc)))
        return rc;
    return require_device(device);
}

int lrt_observed(int device, uint32_t F, uint32_t N, const double *y, const double *e, uint32_t K, const double *M, uint32_t L0, const double *P0,
                 uint32_t L1, const double *P1, const int32_t *C, const int nc[2], int fixalpha, uint32_t max_iters, mmg_diff_lrt *h, LrtDevice &D)
{
    h->F = F;
    const bool Mnil = df_nil(M, N, K), Pnil[2] = {df_nil(P0, N, L0), df_nil(P1, N, L1)};
    h->flags[0] = Mnil; h->flags[1] = Pnil[0]; h->flags[2] = Pnil[1];
    h->nc[0] = (uint32_t)nc[0]; h->nc[1] = (uint32_t)nc[1];
    std::vector<double> X[2];
    X[0] = lrt_design(N, fixalpha != 0, Mnil, K, M, Pnil[0], L0, P0, &h->p[0]);
    X[1] = lrt_design(N, fixalpha != 0, Mnil, K, M, Pnil[1], L1, P1, &h->p[1]);
    h->df = (int32_t)(h->p[1] + h->nc[1]) - (int32_t)(h->p[0] + h->nc[0]);
    const uint32_t pm = h->p[0] > h->p[1] ? h->p[0] : h->p[1], ncmax = h->nc[0] > h->nc[1] ? h->nc[0] : h->nc[1];
    const bool small = pm <= (uint32_t)LRT_PSMALL;
    const uint64_t wslots = 2ull * ncmax + (small ? 0 : (uint64_t)pm * (pm + 1) / 2);

    // the device arrays are the caller's (D) and go when it lets them; the host sources of the asynchronous copies are locals, and
    // `drain`, the last local, waits for the stream before they go
    const uint64_t FN = (uint64_t)F * N;
    DiffStaged staged;
    std::vector<int> cls(2 * (size_t)N);
    DevStream &st = D.st;
    DevBuf<double> &d_y = D.d_y, &d_esq = D.d_esq, (&d_X)[2] = D.d_X, (&d_theta)[2] = D.d_theta, (&d_sig)[2] = D.d_sig, &d_ll = D.d_ll, &d_ws = D.d_ws;
    DevBuf<int> &d_cls = D.d_cls;
    DevBuf<uint32_t> &d_iters = D.d_iters, &d_status = D.d_status;
    auto dalloc = [&](auto &buf, uint64_t count) {
        if (count == 0) return hipSuccess;   // (a model without columns: the pointer is never read)
        HIPE_TRY(buf.alloc(count));
        h->device_bytes += count * sizeof(*buf.get());
        return hipSuccess;
    };
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(st.create(hipStreamNonBlocking));
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{st.get()};
    HIP_TRY(dalloc(d_y, FN));
    HIP_TRY(dalloc(d_esq, FN));
    for (int mi = 0; mi < 2; ++mi) {
        HIP_TRY(dalloc(d_X[mi], (uint64_t)N * h->p[mi]));
        HIP_TRY(dalloc(d_theta[mi], (uint64_t)F * h->p[mi]));
        HIP_TRY(dalloc(d_sig[mi], (uint64_t)F * h->nc[mi]));
    }
    HIP_TRY(dalloc(d_ll, 2ull * F));
    HIP_TRY(dalloc(d_ws, wslots * F));
    HIP_TRY(dalloc(d_cls, 2ull * N));
    HIP_TRY(dalloc(d_iters, 2ull * F));
    HIP_TRY(dalloc(d_status, 2ull * F));
    // y and e^2 transposed to [N][F], as mmg_diff_create holds them; the classes as [2][N]
    for (uint32_t i = 0; i < N; ++i) { cls[i] = C[i * 2]; cls[N + i] = C[i * 2 + 1]; }
    const int rc = df_upload_transposed(st.get(), F, N, y, e, d_y.get(), d_esq.get(), staged);
    if (rc) return rc;
    for (int mi = 0; mi < 2; ++mi)
        if (h->p[mi]) HIP_TRY(hipMemcpyAsync(d_X[mi].get(), X[mi].data(), X[mi].size() * 8, hipMemcpyHostToDevice, st.get()));
    HIP_TRY(hipMemcpyAsync(d_cls.get(), cls.data(), cls.size() * 4, hipMemcpyHostToDevice, st.get()));

    LrtParams &q = D.q;
    D.small = small; D.pm = pm;
    q.F = (int)F; q.N = (int)N;
    q.p[0] = (int)h->p[0]; q.p[1] = (int)h->p[1];
    q.nc[0] = nc[0]; q.nc[1] = nc[1];
    q.ncmax = (int)ncmax;
    q.max_iters = max_iters ? max_iters : LRT_MAX_ITERS;
    const dim3 grid((F + LRT_BLOCK - 1) / LRT_BLOCK), block(LRT_BLOCK);
    if (small)
        hipLaunchKernelGGL(k_lrt<LRT_PSMALL>, grid, block, 0, st.get(), q, d_X[0].get(), d_X[1].get(), d_cls.get(), d_y.get(), d_esq.get(),
                           d_theta[0].get(), d_theta[1].get(), d_sig[0].get(), d_sig[1].get(), d_ll.get(), d_iters.get(), d_status.get(), d_ws.get());
    else
        hipLaunchKernelGGL(k_lrt<0>, grid, block, 0, st.get(), q, d_X[0].get(), d_X[1].get(), d_cls.get(), d_y.get(), d_esq.get(),
                           d_theta[0].get(), d_theta[1].get(), d_sig[0].get(), d_sig[1].get(), d_ll.get(), d_iters.get(), d_status.get(), d_ws.get());
    HIP_TRY(hipGetLastError());

    h->ll.resize(2 * (size_t)F); h->iters.resize(2 * (size_t)F); h->status.resize(2 * (size_t)F);
    HIP_TRY(hipMemcpyAsync(h->ll.data(), d_ll.get(), 2 * (size_t)F * 8, hipMemcpyDeviceToHost, st.get()));
    HIP_TRY(hipMemcpyAsync(h->iters.data(), d_iters.get(), 2 * (size_t)F * 4, hipMemcpyDeviceToHost, st.get()));
    HIP_TRY(hipMemcpyAsync(h->status.data(), d_status.get(), 2 * (size_t)F * 4, hipMemcpyDeviceToHost, st.get()));
    for (int mi = 0; mi < 2; ++mi) {
        h->theta[mi].resize((size_t)F * h->p[mi]);
        h->sig[mi].resize((size_t)F * h->nc[mi]);
        if (h->p[mi]) HIP_TRY(hipMemcpyAsync(h->theta[mi].data(), d_theta[mi].get(), h->theta[mi].size() * 8, hipMemcpyDeviceToHost, st.get()));
        HIP_TRY(hipMemcpyAsync(h->sig[mi].data(), d_sig[mi].get(), h->sig[mi].size() * 8, hipMemcpyDeviceToHost, st.get()));
    }
    HIP_TRY(hipStreamSynchronize(st.get()));

    // the derived statistics, on the host
    h->stat.resize(F); h->pv.resize(F); h->qv.resize(F);
    for (size_t f = 0; f < F; ++f) {
        h->stat[f] = 2.0 * (h->ll[F + f] - h->ll[f]);
        h->pv[f] = lrt::chi2_sf(h->df, h->stat[f]);
    }
    lrt::bh_qvalues(F, h->pv.data(), h->qv.data());
    return MMG_OK;
}

} // namespace mmg

extern "C" int mmg_diff_lrt_create(int device, uint32_t F, uint32_t N, const double *y, const double *e, uint32_t K, const double *M,
                                   uint32_t L0, const double *P0, uint32_t L1, const double *P1, const int32_t *C, int fixalpha,
                                   uint32_t max_iters, mmg_diff_lrt **out)
{
    if (!out || !y || !e || !M || !P0 || !P1 || !C) return fail(MMG_ERR_ARG, "NULL argument");
    *out = nullptr;
    int nc[2] = {0, 0};
    int rc = lrt_check_args(device, F, N, y, e, K, M, L0, P0, L1, P1, C, nc);
    if (rc) return rc;
    std::unique_ptr<mmg_diff_lrt> h(new mmg_diff_lrt());
    LrtDevice D;   // released when this function returns
    rc = lrt_observed(device, F, N, y, e, K, M, L0, P0, L1, P1, C, nc, fixalpha, max_iters, h.get(), D);
    if (rc) return rc;
    *out = h.release();
    return MMG_OK;
}

extern "C" int mmg_diff_lrt_get(mmg_diff_lrt *h, double *loglik, double *stat, double *p_value, double *q_value, int32_t *df, double *theta0,
                                double *theta1, double *sigmasq0, double *sigmasq1, uint32_t *iters, uint32_t *status)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL argument");
    auto put = [](auto *dst, const auto &v) { if (dst && !v.empty()) std::memcpy(dst, v.data(), v.size() * sizeof(v[0])); };
    put(loglik, h->ll); put(stat, h->stat); put(p_value, h->pv); put(q_value, h->qv);
    if (df) *df = h->df;
    put(theta0, h->theta[0]); put(theta1, h->theta[1]); put(sigmasq0, h->sig[0]); put(sigmasq1, h->sig[1]);
    put(iters, h->iters); put(status, h->status);
    return MMG_OK;
}

extern "C" int mmg_diff_lrt_info(mmg_diff_lrt *h, int32_t *flags, uint32_t *n_classes, uint32_t *n_cols)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL argument");
    if (flags) { flags[0] = h->flags[0]; flags[1] = h->flags[1]; flags[2] = h->flags[2]; }
    if (n_classes) { n_classes[0] = h->nc[0]; n_classes[1] = h->nc[1]; }
    if (n_cols) { n_cols[0] = h->p[0]; n_cols[1] = h->p[1]; }
    return MMG_OK;
}

extern "C" int mmg_diff_lrt_device_bytes(mmg_diff_lrt *h, uint64_t *bytes)
{
    if (!h || !bytes) return fail(MMG_ERR_ARG, "NULL argument");
    *bytes = h->device_bytes;
    return MMG_OK;
}

extern "C" void mmg_diff_lrt_destroy(mmg_diff_lrt *h) { delete h; }
