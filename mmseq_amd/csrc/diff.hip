// diff.hip -- device TU + host side of the mmg_diff_* entry points: mmdiff's per-feature MCMC (src/bms.cpp driven as
// src/mmdiff.cpp:744-866).  Kernels in diff_kernels.h.
#include "diff_kernels.h"
#include "mmg_host.h"

#include <cmath>
#include <memory>
#include <vector>

using namespace mmg;

namespace {
constexpr uint32_t DF_CHUNK = 512;    // iterations per launch of burn-in and sampling
constexpr int DF_REC_FROM = 102;      // OUTLEN / 10: burn-in iterations before this one are not recorded
}

// Members are destroyed in reverse declaration order: the destructor waits for `st`, then the buffers go, and the stream last.
struct mmg_diff {
    DevStream st;
    int device = 0;
    DiffParams p{};
    uint32_t F = 0, N = 0, K = 0, L[2] = {0, 0};
    size_t nslot = 0;
    DevBuf<double> d_y, d_esq, d_st, d_M, d_P0, d_P1;
    DevBuf<int> d_C, d_gam, d_tuned, d_cnt;
    uint32_t burnin = 0, batches = 0, sampled = 0;
    bool burnt = false;
    uint64_t device_bytes = 0;
    ~mmg_diff() { if (st) (void)hipStreamSynchronize(st.get()); }
};

// the reference's "nil" rule (BMS::BMS): a single column whose entries differ by less than 1e-5 is no covariate at all
static bool df_nil(const double *X, uint32_t N, uint32_t cols)
{
    if (cols != 1 || N == 0) return false;
    double lo = X[0], hi = X[0];
    for (uint32_t i = 1; i < N; ++i) { lo = X[i] < lo ? X[i] : lo; hi = X[i] > hi ? X[i] : hi; }
    return hi - lo < 0.00001;
}

static inline unsigned df_blocks(uint32_t F) { return (F + DF_BLOCK - 1) / DF_BLOCK; }

extern "C" int mmg_diff_create(int device, uint32_t F, uint32_t N, const double *y, const double *e, uint32_t K, const double *M,
                               uint32_t L0, const double *P0, uint32_t L1, const double *P1, const int32_t *C, double d, double s,
                               double pdash, int fixalpha, uint64_t seed, mmg_diff **out)
{
    if (!out || !y || !e || !M || !P0 || !P1 || !C) return fail(MMG_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (F == 0 || F > 0x7fffff00u / DF_BLOCK) return fail(MMG_ERR_ARG, "the number of features must be between 1 and 33554428");
    if (N < 2 || N > (uint32_t)DF_NMAX) return fail(MMG_ERR_ARG, "the number of samples must be between 2 and 512");
    if (K < 1 || K > (uint32_t)DF_KMAX) return fail(MMG_ERR_ARG, "M must have between 1 and 8 columns");
    if (L0 < 1 || L0 > (uint32_t)DF_LMAX || L1 < 1 || L1 > (uint32_t)DF_LMAX) return fail(MMG_ERR_ARG, "P0 and P1 must have between 1 and 16 columns");
    if (!(d > 0) || !(s > 0) || !std::isfinite(d) || !std::isfinite(s) || !(pdash >= 0 && pdash <= 1))
        return fail(MMG_ERR_ARG, "d and s must be positive and finite and pdash in [0, 1]");
    // every input value finite: a NaN or an infinity would reach the log densities and the samplers on the device
    auto finite = [](const double *x, uint64_t n) { for (uint64_t i = 0; i < n; ++i) if (!std::isfinite(x[i])) return false; return true; };
    if (!finite(y, (uint64_t)F * N) || !finite(e, (uint64_t)F * N)) return fail(MMG_ERR_ARG, "y and e must be finite");
    if (!finite(M, (uint64_t)N * K) || !finite(P0, (uint64_t)N * L0) || !finite(P1, (uint64_t)N * L1)) return fail(MMG_ERR_ARG, "M, P0 and P1 must be finite");
    int nc[2] = {0, 0};
    for (int mi = 0; mi < 2; ++mi) {
        std::vector<int> seen(DF_CMAX, 0);
        for (uint32_t i = 0; i < N; ++i) {
            const int c = C[i * 2 + mi];
            if (c < 0 || c >= DF_CMAX) return fail(MMG_ERR_ARG, "class labels must be between 0 and 15");
            seen[c] = 1;
            nc[mi] = c + 1 > nc[mi] ? c + 1 : nc[mi];
        }
        for (int c = 0; c < nc[mi]; ++c)
            if (!seen[c]) return fail(MMG_ERR_ARG, "the class labels of each model must be 0, 1, ..., n - 1 without gaps");
    }
    int rc = require_device(device);
    if (rc) return rc;

    std::unique_ptr<mmg_diff> h(new mmg_diff());
    h->device = device; h->F = F; h->N = N; h->K = K; h->L[0] = L0; h->L[1] = L1;
    DiffParams &p = h->p;
    p.F = (int)F; p.N = (int)N; p.K = (int)K;
    p.Mnil = df_nil(M, N, K) ? 1 : 0;
    p.fixalpha = fixalpha ? 1 : 0;
    p.d = d; p.s = s; p.v_beta = fixalpha ? 25.0 : 4.0;
    p.seed = seed;
    int o = 0;
    for (int mi = 0; mi < 2; ++mi) {
        DiffModel &m = p.m[mi];
        const int Lm = (int)h->L[mi];
        m.L = Lm; m.nc = nc[mi]; m.Pnil = df_nil(mi ? P1 : P0, N, Lm) ? 1 : 0;
        for (int *slot : {&m.alpha, &m.A, &m.Va, &m.aS, &m.aSS, &m.aN, &m.rho, &m.Q, &m.R, &m.rS, &m.rlS}) *slot = o++;
        for (int *slot : {&m.beta, &m.B, &m.Vb, &m.bS, &m.bSS, &m.bN}) { *slot = o; o += (int)K; }
        for (int *slot : {&m.eta, &m.Fm, &m.Ve, &m.eS, &m.eSS, &m.eN, &m.lam, &m.Dm, &m.Si, &m.lS, &m.llS}) { *slot = o; o += Lm; }
        for (int *slot : {&m.sig, &m.J, &m.Lm, &m.sS, &m.slS}) { *slot = o; o += m.nc; }
    }
    p.gsum = o++; p.logitp = o++; p.LOsum = o++;
    const int KK = p.Mnil ? 0 : (int)(K * K), Kv = p.Mnil ? 0 : (int)K, ncmax = nc[0] > nc[1] ? nc[0] : nc[1];
    for (int *slot : {&p.wG, &p.wLg, &p.wLi, &p.wV, &p.wLv}) { *slot = o; o += KK; }
    for (int *slot : {&p.wt, &p.wz}) { *slot = o; o += Kv; }
    for (int *slot : {&p.wlprop, &p.wsum}) { *slot = o; o += ncmax; }
    h->nslot = (size_t)o;

    auto dalloc = [&](auto &buf, uint64_t count) {
        HIPE_TRY(buf.alloc(count));
        h->device_bytes += count * sizeof(*buf.get());
        return hipSuccess;
    };
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(h->st.create(hipStreamNonBlocking));
    const uint64_t FN = (uint64_t)F * N;
    HIP_TRY(dalloc(h->d_y, FN));
    HIP_TRY(dalloc(h->d_esq, FN));
    HIP_TRY(dalloc(h->d_st, (uint64_t)h->nslot * F));
    HIP_TRY(dalloc(h->d_M, (uint64_t)N * K));
    HIP_TRY(dalloc(h->d_P0, (uint64_t)N * L0));
    HIP_TRY(dalloc(h->d_P1, (uint64_t)N * L1));
    HIP_TRY(dalloc(h->d_C, (uint64_t)N * 2));
    HIP_TRY(dalloc(h->d_gam, (uint64_t)F));
    HIP_TRY(dalloc(h->d_tuned, (uint64_t)F));
    HIP_TRY(dalloc(h->d_cnt, 1));
    // y and e^2 transposed to [N][F]: the lanes of a wave read adjacent words
    std::vector<double> ty(FN), te(FN);
    for (uint64_t f = 0; f < F; ++f)
        for (uint64_t i = 0; i < N; ++i) {
            ty[i * F + f] = y[f * N + i];
            const double ei = e[f * N + i];
            te[i * F + f] = ei * ei;
        }
    HIP_TRY(hipMemcpyAsync(h->d_y.get(), ty.data(), FN * 8, hipMemcpyHostToDevice, h->st.get()));
    HIP_TRY(hipMemcpyAsync(h->d_esq.get(), te.data(), FN * 8, hipMemcpyHostToDevice, h->st.get()));
    HIP_TRY(hipMemcpyAsync(h->d_M.get(), M, (size_t)N * K * 8, hipMemcpyHostToDevice, h->st.get()));
    HIP_TRY(hipMemcpyAsync(h->d_P0.get(), P0, (size_t)N * L0 * 8, hipMemcpyHostToDevice, h->st.get()));
    HIP_TRY(hipMemcpyAsync(h->d_P1.get(), P1, (size_t)N * L1 * 8, hipMemcpyHostToDevice, h->st.get()));
    HIP_TRY(hipMemcpyAsync(h->d_C.get(), C, (size_t)N * 2 * 4, hipMemcpyHostToDevice, h->st.get()));
    p.M = h->d_M.get(); p.m[0].P = h->d_P0.get(); p.m[1].P = h->d_P1.get(); p.Cl = h->d_C.get();
    p.y = h->d_y.get(); p.esq = h->d_esq.get(); p.st = h->d_st.get(); p.gam = h->d_gam.get(); p.tuned = h->d_tuned.get();
    const double logitp0 = std::log(pdash) - std::log(1.0 - pdash);
    hipLaunchKernelGGL(k_df_init, dim3(df_blocks(F)), dim3(DF_BLOCK), 0, h->st.get(), p, logitp0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->st.get()));   // (the host buffers were the sources of asynchronous copies)
    *out = h.release();
    return MMG_OK;
}

extern "C" int mmg_diff_burnin(mmg_diff *h, uint32_t iters)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL argument");
    if (h->burnt) return fail(MMG_ERR_STATE, "the burn-in has run already");
    if (iters == 0 || iters % 1024) return fail(MMG_ERR_ARG, "burn-in iterations must be a positive multiple of 1024");
    HIP_TRY(hipSetDevice(h->device));
    for (uint32_t t = 0; t < iters; t += DF_CHUNK) {
        const uint32_t n = iters - t < DF_CHUNK ? iters - t : DF_CHUNK;
        hipLaunchKernelGGL(k_df_run, dim3(df_blocks(h->F)), dim3(DF_BLOCK), 0, h->st.get(), h->p, t, (int)t, (int)n, 0, DF_REC_FROM);
    }
    hipLaunchKernelGGL(k_df_pseudo, dim3(df_blocks(h->F)), dim3(DF_BLOCK), 0, h->st.get(), h->p, (double)(iters - DF_REC_FROM));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->st.get()));
    h->burnin = iters;
    h->burnt = true;
    return MMG_OK;
}

extern "C" int mmg_diff_tune_batch(mmg_diff *h, uint32_t *untuned)
{
    if (!h || !untuned) return fail(MMG_ERR_ARG, "NULL argument");
    if (!h->burnt) return fail(MMG_ERR_STATE, "mmg_diff_tune_batch before mmg_diff_burnin");
    if (h->sampled) return fail(MMG_ERR_STATE, "mmg_diff_tune_batch after sampling has started");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemsetAsync(h->d_cnt.get(), 0, 4, h->st.get()));
    const uint32_t it0 = h->burnin + h->batches * DF_BATCH;
    hipLaunchKernelGGL(k_df_tune, dim3(df_blocks(h->F)), dim3(DF_BLOCK), 0, h->st.get(), h->p, it0, (int)h->batches, h->d_cnt.get());
    HIP_TRY(hipGetLastError());
    int cnt = 0;
    HIP_TRY(hipMemcpyAsync(&cnt, h->d_cnt.get(), 4, hipMemcpyDeviceToHost, h->st.get()));
    HIP_TRY(hipStreamSynchronize(h->st.get()));
    ++h->batches;
    *untuned = (uint32_t)cnt;
    return MMG_OK;
}

extern "C" int mmg_diff_sample(mmg_diff *h, uint32_t iters)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL argument");
    if (!h->burnt) return fail(MMG_ERR_STATE, "mmg_diff_sample before mmg_diff_burnin");
    if (iters == 0) return fail(MMG_ERR_ARG, "iters must be positive");
    HIP_TRY(hipSetDevice(h->device));
    const uint32_t t_first = h->batches * DF_BATCH + h->sampled;
    for (uint32_t j = 0; j < iters; j += DF_CHUNK) {
        const uint32_t n = iters - j < DF_CHUNK ? iters - j : DF_CHUNK;
        hipLaunchKernelGGL(k_df_run, dim3(df_blocks(h->F)), dim3(DF_BLOCK), 0, h->st.get(), h->p, h->burnin + t_first + j, (int)(t_first + j), (int)n, 2, 0);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->st.get()));
    h->sampled += iters;
    return MMG_OK;
}

extern "C" int mmg_diff_get_results(mmg_diff *h, double *gamma_mean, double *logitp, double *alpha, double *beta, double *eta)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL argument");
    if (!h->sampled) return fail(MMG_ERR_STATE, "mmg_diff_get_results before mmg_diff_sample");
    HIP_TRY(hipSetDevice(h->device));
    const size_t F = h->F;
    auto slot = [&](int o, std::vector<double> &v) {
        v.resize(F);
        return hipMemcpy(v.data(), h->d_st.get() + (size_t)o * F, F * 8, hipMemcpyDeviceToHost);
    };
    std::vector<double> a, b;
    // the means as BMS::gammamean / alphamean / betamean / etamean form them: sum / count, on the host
    if (gamma_mean) {
        HIP_TRY(slot(h->p.gsum, a));
        for (size_t f = 0; f < F; ++f) gamma_mean[f] = a[f] / (double)h->sampled;
    }
    if (logitp) {
        HIP_TRY(slot(h->p.logitp, a));
        for (size_t f = 0; f < F; ++f) logitp[f] = a[f];
    }
    for (int mi = 0; mi < 2; ++mi) {
        const DiffModel &m = h->p.m[mi];
        if (alpha) {
            HIP_TRY(slot(m.aS, a)); HIP_TRY(slot(m.aN, b));
            for (size_t f = 0; f < F; ++f) alpha[mi * F + f] = a[f] / b[f];
        }
        if (beta)
            for (uint32_t k = 0; k < h->K; ++k) {
                HIP_TRY(slot(m.bS + (int)k, a)); HIP_TRY(slot(m.bN + (int)k, b));
                for (size_t f = 0; f < F; ++f) beta[((size_t)mi * h->K + k) * F + f] = a[f] / b[f];
            }
        if (eta)
            for (uint32_t l = 0; l < h->L[mi]; ++l) {
                HIP_TRY(slot(m.eS + (int)l, a)); HIP_TRY(slot(m.eN + (int)l, b));
                for (size_t f = 0; f < F; ++f) eta[((mi ? h->L[0] : 0) + l) * F + f] = a[f] / b[f];
            }
    }
    return MMG_OK;
}

extern "C" int mmg_diff_info(mmg_diff *h, int32_t *flags, uint32_t *n_classes, uint32_t *batches)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL argument");
    if (flags) { flags[0] = h->p.Mnil; flags[1] = h->p.m[0].Pnil; flags[2] = h->p.m[1].Pnil; }
    if (n_classes) { n_classes[0] = (uint32_t)h->p.m[0].nc; n_classes[1] = (uint32_t)h->p.m[1].nc; }
    if (batches) *batches = h->batches;
    return MMG_OK;
}

extern "C" int mmg_diff_device_bytes(mmg_diff *h, uint64_t *bytes)
{
    if (!h || !bytes) return fail(MMG_ERR_ARG, "NULL argument");
    *bytes = h->device_bytes;
    return MMG_OK;
}

extern "C" void mmg_diff_destroy(mmg_diff *h) { delete h; }
