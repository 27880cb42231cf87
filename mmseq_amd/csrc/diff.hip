// diff.hip -- device TU + host side of the mmg_diff_* entry points: mmdiff's per-feature MCMC (src/bms.cpp driven as
// src/mmdiff.cpp:744-866).  Kernels in diff_kernels.h.
#include "diff_kernels.h"
#include "diff_perm_kernels.h"
#include "diff_lrt_kernels.h"
#include "mmg_host.h"

#include <cmath>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

using namespace mmg;

namespace {
constexpr uint32_t DF_CHUNK = 512;    // iterations per launch of burn-in and sampling
constexpr int DF_REC_FROM = 102;      // OUTLEN / 10: burn-in iterations before this one are not recorded
}
static_assert(LRT_KMAX == DF_KMAX && LRT_LMAX == DF_LMAX && LRT_CMAX == DF_CMAX && LRT_NMAX == DF_NMAX && LRT_BLOCK == DF_BLOCK,
              "the likelihood-ratio test (diff_lrt_kernels.h) takes the designs mmg_diff_create takes");

// What mmg_diff_trace_open adds to a handle: the copy stream, two row buffers on the device and two in pinned host memory, and the
// events between them.  Launch i records into d_rows[i & 1]; the copy stream waits for it and copies to h_rows[i & 1]; the host hands
// launch i - 1's rows to the sink while launch i runs.
struct DiffTracing {
    DevStream copy;
    DevEvent ran[2], copied[2];
    DevBuf<double> d_rows[2];
    PinnedBuf<double> h_rows[2];
    DevBuf<DiffTrace> d_q;         // [2] the descriptor of the launch that records into d_rows[b], copied from h_q[b] ahead of it
    PinnedBuf<DiffTrace> h_q;      // [2]
    DiffTrace q{};                 // the slot table; tr, P, every, tt0 are set per launch
    int P = 0;                     // traced parameters, gamma (the last one, sampling only) included
    uint32_t every[2] = {1, 1};    // burn-in, sampling
    uint32_t cap = 0;              // rows a buffer holds
    mmg_diff_trace_sink sink = nullptr;
    void *user = nullptr;
    bool stopped = false;          // the sink returned non-zero: the chain is part way through a phase
};

// What mmg_diff_effects_open adds to a handle: one resident buffer of sampling rows and the descriptor of the launch that records
// into it.  Nothing is copied out: mmg_diff_effects_summarize reads the rows where they are.
struct DiffEffectsRows {
    DevBuf<double> d_rows;         // [max_rows][P][F]
    DevBuf<DiffTrace> d_q;         // [1] written ahead of every sampling launch, in stream order
    DiffTrace q{};                 // the slot table; tr, tt0, cap are set per launch
    int P = 0;                     // traced parameters, gamma (the last one) included
    uint32_t every = 1, max_rows = 0;
    std::vector<uint8_t> model_of; // [P - 1] the model of each traced parameter
};

// Members are destroyed in reverse declaration order: the destructor waits for the streams, then the buffers go, and `st` last.
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
    std::unique_ptr<DiffTracing> tr;
    std::unique_ptr<DiffEffectsRows> fx;
    ~mmg_diff()
    {
        if (st) (void)hipStreamSynchronize(st.get());
        if (tr && tr->copy) (void)hipStreamSynchronize(tr->copy.get());
    }
};

// the reference's "nil" rule (BMS::BMS): a single column whose entries differ by less than 1e-5 is no covariate at all
bool mmg::df_nil(const double *X, uint32_t N, uint32_t cols)
{
    if (cols != 1 || N == 0) return false;
    double lo = X[0], hi = X[0];
    for (uint32_t i = 1; i < N; ++i) { lo = X[i] < lo ? X[i] : lo; hi = X[i] > hi ? X[i] : hi; }
    return hi - lo < 0.00001;
}

static inline unsigned df_blocks(uint32_t F) { return (F + DF_BLOCK - 1) / DF_BLOCK; }

// the classes of one model, C[i * stride]: labels 0 .. *nc - 1, every one of them used
int mmg::df_classes(const int32_t *C, uint32_t stride, uint32_t N, int *nc)
{
    std::vector<int> seen(DF_CMAX, 0);
    *nc = 0;
    for (uint32_t i = 0; i < N; ++i) {
        const int c = C[i * stride];
        if (c < 0 || c >= DF_CMAX) return fail(MMG_ERR_ARG, "class labels must be between 0 and 15");
        seen[c] = 1;
        *nc = c + 1 > *nc ? c + 1 : *nc;
    }
    for (int c = 0; c < *nc; ++c)
        if (!seen[c]) return fail(MMG_ERR_ARG, "the class labels of each model must be 0, 1, ..., n - 1 without gaps");
    return MMG_OK;
}

// ---- the argument checks every create entry of mmdiff makes, in the order it makes them (mmg_host.h) ---------------------------------
int mmg::df_check_shape(uint32_t F, uint32_t N, uint32_t K)
{
    if (F == 0 || F > 0x7fffff00u / DF_BLOCK) return fail(MMG_ERR_ARG, "the number of features must be between 1 and 33554428");
    if (N < 2 || N > (uint32_t)DF_NMAX) return fail(MMG_ERR_ARG, "the number of samples must be between 2 and 512");
    if (K < 1 || K > (uint32_t)DF_KMAX) return fail(MMG_ERR_ARG, "M must have between 1 and 8 columns");
    return MMG_OK;
}

int mmg::df_check_cols(uint32_t L0, uint32_t J, const uint32_t *L1)
{
    bool ok = L0 >= 1 && L0 <= (uint32_t)DF_LMAX;
    for (uint32_t j = 0; j < J; ++j) ok = ok && L1[j] >= 1 && L1[j] <= (uint32_t)DF_LMAX;
    return ok ? (int)MMG_OK : fail(MMG_ERR_ARG, "P0 and P1 must have between 1 and 16 columns");
}

int mmg::df_check_prior(double d, double s, double pdash)
{
    if (!(d > 0) || !(s > 0) || !std::isfinite(d) || !std::isfinite(s) || !(pdash >= 0 && pdash <= 1))
        return fail(MMG_ERR_ARG, "d and s must be positive and finite and pdash in [0, 1]");
    return MMG_OK;
}

// every input value finite: a NaN or an infinity would reach the log densities and the samplers on the device
int mmg::df_check_finite(uint32_t F, uint32_t N, const double *y, const double *e, uint32_t K, const double *M, uint32_t L0, const double *P0,
                         uint64_t L1, const double *P1)
{
    auto finite = [](const double *x, uint64_t n) { for (uint64_t i = 0; i < n; ++i) if (!std::isfinite(x[i])) return false; return true; };
    if (!finite(y, (uint64_t)F * N) || !finite(e, (uint64_t)F * N)) return fail(MMG_ERR_ARG, "y and e must be finite");
    if (!finite(M, (uint64_t)N * K) || !finite(P0, (uint64_t)N * L0) || !finite(P1, (uint64_t)N * L1)) return fail(MMG_ERR_ARG, "M, P0 and P1 must be finite");
    return MMG_OK;
}

int mmg::df_check_classes(const int32_t *C, uint32_t N, int nc[2])
{
    nc[0] = nc[1] = 0;
    for (int mi = 0; mi < 2; ++mi) {
        const int rc = df_classes(C + mi, 2, N, &nc[mi]);
        if (rc) return rc;
    }
    return MMG_OK;
}

int mmg::df_upload_transposed(hipStream_t st, uint32_t F, uint32_t N, const double *y, const double *e, double *d_y, double *d_esq, DiffStaged &staged)
{
    const uint64_t FN = (uint64_t)F * N;
    std::vector<double> &ty = staged.ty, &te = staged.te;
    ty.resize(FN); te.resize(FN);
    for (uint64_t f = 0; f < F; ++f)
        for (uint64_t i = 0; i < N; ++i) {
            ty[i * F + f] = y[f * N + i];
            const double ei = e[f * N + i];
            te[i * F + f] = ei * ei;
        }
    HIP_TRY(hipMemcpyAsync(d_y, ty.data(), FN * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_esq, te.data(), FN * 8, hipMemcpyHostToDevice, st));
    return MMG_OK;
}

// what every handle's DiffParams start from: the sizes, the nil flags, the hyperparameters and the seed (the pointers, `chain` and
// the slot layout are the caller's)
static DiffParams df_params(uint32_t F, uint32_t N, uint32_t K, const double *M, uint32_t L0, const double *P0, uint32_t L1, const double *P1,
                            double d, double s, int fixalpha, uint64_t seed)
{
    DiffParams p{};
    p.F = (int)F; p.N = (int)N; p.K = (int)K;
    p.Mnil = df_nil(M, N, K) ? 1 : 0;
    p.fixalpha = fixalpha ? 1 : 0;
    p.d = d; p.s = s; p.v_beta = fixalpha ? 25.0 : 4.0;
    p.seed = seed;
    p.m[0].Pnil = df_nil(P0, N, L0) ? 1 : 0;
    p.m[1].Pnil = df_nil(P1, N, L1) ? 1 : 0;
    return p;
}

// the slot offsets of one comparison's state and workspace (p.K and p.Mnil set); the number of slots per feature:
// for each model 11 + 6 K + 11 L + 5 classes, then 3, then (M not nil) 5 K^2 + 2 K, then 2 max(classes)
static size_t df_layout(DiffParams &p, const uint32_t L[2], const int nc[2])
{
    const int K = p.K;
    int o = 0;
    for (int mi = 0; mi < 2; ++mi) {
        DiffModel &m = p.m[mi];
        const int Lm = (int)L[mi];
        m.L = Lm; m.nc = nc[mi];
        for (int *slot : {&m.alpha, &m.A, &m.Va, &m.aS, &m.aSS, &m.aN, &m.rho, &m.Q, &m.R, &m.rS, &m.rlS}) *slot = o++;
        for (int *slot : {&m.beta, &m.B, &m.Vb, &m.bS, &m.bSS, &m.bN}) { *slot = o; o += K; }
        for (int *slot : {&m.eta, &m.Fm, &m.Ve, &m.eS, &m.eSS, &m.eN, &m.lam, &m.Dm, &m.Si, &m.lS, &m.llS}) { *slot = o; o += Lm; }
        for (int *slot : {&m.sig, &m.J, &m.Lm, &m.sS, &m.slS}) { *slot = o; o += m.nc; }
    }
    p.gsum = o++; p.logitp = o++; p.LOsum = o++;
    const int KK = p.Mnil ? 0 : K * K, Kv = p.Mnil ? 0 : K, ncmax = nc[0] > nc[1] ? nc[0] : nc[1];
    for (int *slot : {&p.wG, &p.wLg, &p.wLi, &p.wV, &p.wLv}) { *slot = o; o += KK; }
    for (int *slot : {&p.wt, &p.wz}) { *slot = o; o += Kv; }
    for (int *slot : {&p.wlprop, &p.wsum}) { *slot = o; o += ncmax; }
    return (size_t)o;
}

// the posterior means of one comparison from its state block, as mmg_diff_get_results documents them
static int df_results(const DiffParams &p, const double *d_st, size_t F, uint32_t K, const uint32_t L[2], uint32_t sampled, double *gamma_mean,
                      double *logitp, double *alpha, double *beta, double *eta)
{
    auto slot = [&](int o, std::vector<double> &v) {
        v.resize(F);
        return hipMemcpy(v.data(), d_st + (size_t)o * F, F * 8, hipMemcpyDeviceToHost);
    };
    std::vector<double> a, b;
    // the means as BMS::gammamean / alphamean / betamean / etamean form them: sum / count, on the host
    if (gamma_mean) {
        HIP_TRY(slot(p.gsum, a));
        for (size_t f = 0; f < F; ++f) gamma_mean[f] = a[f] / (double)sampled;
    }
    if (logitp) {
        HIP_TRY(slot(p.logitp, a));
        for (size_t f = 0; f < F; ++f) logitp[f] = a[f];
    }
    for (int mi = 0; mi < 2; ++mi) {
        const DiffModel &m = p.m[mi];
        if (alpha) {
            HIP_TRY(slot(m.aS, a)); HIP_TRY(slot(m.aN, b));
            for (size_t f = 0; f < F; ++f) alpha[mi * F + f] = a[f] / b[f];
        }
        if (beta)
            for (uint32_t k = 0; k < K; ++k) {
                HIP_TRY(slot(m.bS + (int)k, a)); HIP_TRY(slot(m.bN + (int)k, b));
                for (size_t f = 0; f < F; ++f) beta[((size_t)mi * K + k) * F + f] = a[f] / b[f];
            }
        if (eta)
            for (uint32_t l = 0; l < L[mi]; ++l) {
                HIP_TRY(slot(m.eS + (int)l, a)); HIP_TRY(slot(m.eN + (int)l, b));
                for (size_t f = 0; f < F; ++f) eta[((mi ? L[0] : 0) + l) * F + f] = a[f] / b[f];
            }
    }
    return MMG_OK;
}

extern "C" int mmg_diff_create(int device, uint32_t F, uint32_t N, const double *y, const double *e, uint32_t K, const double *M,
                               uint32_t L0, const double *P0, uint32_t L1, const double *P1, const int32_t *C, double d, double s,
                               double pdash, int fixalpha, uint64_t seed, mmg_diff **out)
{
    if (!out || !y || !e || !M || !P0 || !P1 || !C) return fail(MMG_ERR_ARG, "NULL argument");
    *out = nullptr;
    int nc[2] = {0, 0}, rc;
    if ((rc = df_check_shape(F, N, K)) || (rc = df_check_cols(L0, 1, &L1)) || (rc = df_check_prior(d, s, pdash))
        || (rc = df_check_finite(F, N, y, e, K, M, L0, P0, L1, P1)) || (rc = df_check_classes(C, N, nc)) || (rc = require_device(device)))
        return rc;

    std::unique_ptr<mmg_diff> h(new mmg_diff());
    h->device = device; h->F = F; h->N = N; h->K = K; h->L[0] = L0; h->L[1] = L1;
    DiffParams &p = h->p;
    p = df_params(F, N, K, M, L0, P0, L1, P1, d, s, fixalpha, seed);
    h->nslot = df_layout(p, h->L, nc);

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
    DiffStaged staged;
    if ((rc = df_upload_transposed(h->st.get(), F, N, y, e, h->d_y.get(), h->d_esq.get(), staged))) return rc;
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

// ---- traces ------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(DiffTrace) == 496, "mmg_diff_device_bytes with tracing open is documented with this size (include/mmgibbs.h)");
constexpr uint64_t DF_TRACE_BUF_BYTES = 64u << 20;   // the most one row buffer takes (Traces), one row at least

// the traced parameters in the order of BMS::initialise_streams: their names, state slots and models (each if asked for); the count
static int df_trace_table(const mmg_diff *h, std::vector<std::string> *names, int *slot, std::vector<uint8_t> *model = nullptr)
{
    const DiffParams &p = h->p;
    int n = 0;
    auto add = [&](const char *stem, int mi, int idx, int o) {
        if (names) names->push_back(std::string(stem) + std::to_string(mi) + (idx < 0 ? std::string() : "_" + std::to_string(idx)));
        if (slot) slot[n] = o;
        if (model) model->push_back((uint8_t)mi);
        ++n;
    };
    for (int mi = 0; mi < 2; ++mi) add("alpha", mi, -1, p.m[mi].alpha);
    for (int mi = 0; mi < 2; ++mi)
        for (int k = 0; k < p.K; ++k) add("beta", mi, k, p.m[mi].beta + k);
    for (int mi = 0; mi < 2; ++mi)
        for (int l = 0; l < p.m[mi].L; ++l) add("eta", mi, l, p.m[mi].eta + l);
    for (int mi = 0; mi < 2; ++mi)
        for (int l = 0; l < p.m[mi].L; ++l) add("lambda", mi, l, p.m[mi].lam + l);
    for (int mi = 0; mi < 2; ++mi)
        for (int c = 0; c < p.m[mi].nc; ++c) add("sigmasq", mi, c, p.m[mi].sig + c);
    for (int mi = 0; mi < 2; ++mi) add("rho", mi, -1, p.m[mi].rho);
    if (names) names->push_back("gamma");
    if (slot) slot[n] = -1;
    return n + 1;
}

// the columns of BMS::print_pseudo per model: A, Valpha; B, Vbeta per column of M; F, Veta, S per column of P; J, L per class; Q, R
static uint32_t df_pseudo_cols(const mmg_diff *h)
{
    uint32_t n = 0;
    for (int mi = 0; mi < 2; ++mi) n += 2 + 2 * h->K + 3 * h->L[mi] + 2 * (uint32_t)h->p.m[mi].nc + 2;
    return n;
}

extern "C" int mmg_diff_trace_layout(mmg_diff *h, uint32_t *n_params, uint32_t *n_pseudo)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL argument");
    if (n_params) *n_params = (uint32_t)df_trace_table(h, nullptr, nullptr);
    if (n_pseudo) *n_pseudo = df_pseudo_cols(h);
    return MMG_OK;
}

extern "C" int mmg_diff_trace_name(mmg_diff *h, uint32_t param, char *name, uint32_t len)
{
    if (!h || !name || len == 0) return fail(MMG_ERR_ARG, "NULL argument");
    std::vector<std::string> names;
    df_trace_table(h, &names, nullptr);
    if (param >= names.size()) return fail(MMG_ERR_ARG, "no such traced parameter");
    if (names[param].size() + 1 > len) return fail(MMG_ERR_ARG, "the name buffer is too short");
    std::snprintf(name, len, "%s", names[param].c_str());
    return MMG_OK;
}

extern "C" int mmg_diff_trace_open(mmg_diff *h, uint32_t every_burnin, uint32_t every_sample, mmg_diff_trace_sink sink, void *user)
{
    // (the intervals first: the row arithmetic of the launcher and the kernel is written for this range)
    if (every_burnin == 0 || every_sample == 0 || every_burnin > DF_TRACE_EVERY_MAX || every_sample > DF_TRACE_EVERY_MAX)
        return fail(MMG_ERR_ARG, "the thinning intervals must be at least 1 and at most 1073741824");
    if (!h || !sink) return fail(MMG_ERR_ARG, "NULL argument");
    if (h->burnt) return fail(MMG_ERR_ARG, "mmg_diff_trace_open after the burn-in has started");
    if (h->tr) return fail(MMG_ERR_STATE, "tracing is open already");
    if (h->fx) return fail(MMG_ERR_STATE, "mmg_diff_effects_open was called on this handle: traces and effects exclude each other");
    std::unique_ptr<DiffTracing> T(new DiffTracing());
    T->P = df_trace_table(h, nullptr, T->q.slot);
    T->every[0] = every_burnin; T->every[1] = every_sample;
    T->sink = sink; T->user = user;
    const int max_rows = opt(MMG_OPT_DIFF_TRACE_ROWS);
    T->cap = df_trace_cap((uint32_t)T->P, h->F, every_burnin < every_sample ? every_burnin : every_sample, DF_CHUNK, DF_TRACE_BUF_BYTES,
                          max_rows > 0 ? (uint32_t)max_rows : 0);
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(T->copy.create(hipStreamNonBlocking));
    const uint64_t count = (uint64_t)T->cap * T->P * h->F;
    for (int b = 0; b < 2; ++b) {
        HIP_TRY(T->ran[b].create(hipEventDisableTiming));
        HIP_TRY(T->copied[b].create(hipEventDisableTiming));
        HIP_TRY(T->d_rows[b].alloc(count));
        HIP_TRY(T->h_rows[b].alloc(count));
    }
    HIP_TRY(T->d_q.alloc(2));
    HIP_TRY(T->h_q.alloc(2));
    h->device_bytes += 2 * count * 8 + 2 * sizeof(DiffTrace);
    h->tr = std::move(T);
    return MMG_OK;
}

// iters iterations of one phase (0 burn-in, 1 sampling) with rows recorded: the launches of the untraced loop, shortened where a
// buffer would not hold their rows.  it_first: the stream index; t_first: the index k_df_run takes as t0; tt_first: the phase index.
static int df_run_traced(mmg_diff *h, int phase, uint32_t it_first, uint32_t t_first, uint32_t tt_first, uint32_t iters)
{
    DiffTracing &T = *h->tr;
    // (phase indices below 2^30 and intervals up to 2^30: the kernel's tt + every - 1 stays inside int)
    if ((uint64_t)tt_first + iters > (1u << 30)) return fail(MMG_ERR_ARG, "a traced phase takes at most 1073741824 iterations");
    const uint32_t every = T.every[phase];
    const int P = phase ? T.P : T.P - 1;
    const size_t rowlen = (size_t)P * h->F;
    uint32_t first[2] = {0, 0}, rows[2] = {0, 0};
    // launch b's rows, once its copy has ended, to the sink
    auto hand = [&](int b) {
        HIP_TRY(hipEventSynchronize(T.copied[b].get()));
        if (!rows[b]) return (int)MMG_OK;
        const int rc = T.sink(T.user, phase, first[b], rows[b], T.h_rows[b].get());
        if (rc) {
            T.stopped = true;
            (void)hipStreamSynchronize(h->st.get());
            (void)hipStreamSynchronize(T.copy.get());
            return fail(MMG_ERR_IO, "the trace sink returned " + std::to_string(rc));
        }
        return (int)MMG_OK;
    };
    uint32_t i = 0;
    for (uint32_t j = 0; j < iters; ++i) {
        const int b = (int)(i & 1);
        const uint32_t tt = tt_first + j;
        const uint32_t n = df_trace_plan(tt, iters - j, every, T.cap, DF_CHUNK, &first[b], &rows[b]);
        // (buffer b and its descriptor are free: the host waited for launch i - 2's copy before it handed those rows on)
        DiffTrace &q = T.h_q.get()[b];
        q = T.q;
        q.tr = T.d_rows[b].get(); q.P = P; q.every = (int)every; q.tt0 = (int)tt; q.cap = (int)T.cap;
        HIP_TRY(hipMemcpyAsync(T.d_q.get() + b, &q, sizeof(DiffTrace), hipMemcpyHostToDevice, h->st.get()));
        hipLaunchKernelGGL(k_df_run_traced, dim3(df_blocks(h->F)), dim3(DF_BLOCK), 0, h->st.get(), h->p, it_first + j, (int)(t_first + j), (int)n,
                           phase ? 2 : 0, phase ? 0 : DF_REC_FROM, (const DiffTrace *)(T.d_q.get() + b));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(T.ran[b].get(), h->st.get()));
        HIP_TRY(hipStreamWaitEvent(T.copy.get(), T.ran[b].get(), 0));
        if (rows[b]) HIP_TRY(hipMemcpyAsync(T.h_rows[b].get(), T.d_rows[b].get(), rows[b] * rowlen * 8, hipMemcpyDeviceToHost, T.copy.get()));
        HIP_TRY(hipEventRecord(T.copied[b].get(), T.copy.get()));
        if (i >= 1) {
            const int rc = hand(b ^ 1);
            if (rc) return rc;
        }
        j += n;
    }
    return i ? hand((int)((i - 1) & 1)) : (int)MMG_OK;
}

extern "C" int mmg_selftest_diff_trace_plan(uint32_t n_params, uint32_t n_features, uint32_t every_min, uint32_t max_rows, uint32_t tt, uint32_t left,
                                            uint32_t every, uint32_t *cap, uint32_t *first_row, uint32_t *rows, uint32_t *n)
{
    if (!cap || !first_row || !rows || !n) return fail(MMG_ERR_ARG, "NULL argument");
    if (!n_params || !n_features || !every_min || !every || !left || every_min > DF_TRACE_EVERY_MAX || every > DF_TRACE_EVERY_MAX)
        return fail(MMG_ERR_ARG, "counts and intervals must be positive, the intervals at most 1073741824");
    *cap = df_trace_cap(n_params, n_features, every_min, DF_CHUNK, DF_TRACE_BUF_BYTES, max_rows);
    *n = df_trace_plan(tt, left, every, *cap, DF_CHUNK, first_row, rows);
    return MMG_OK;
}

// ---- effects: sampling rows kept on the device ---------------------------------------------------------
extern "C" int mmg_diff_effects_open(mmg_diff *h, uint32_t every, uint32_t max_rows)
{
    if (every == 0 || every > DF_TRACE_EVERY_MAX) return fail(MMG_ERR_ARG, "the thinning interval must be at least 1 and at most 1073741824");
    if (max_rows == 0 || max_rows > 4096) return fail(MMG_ERR_ARG, "max_rows must be between 1 and 4096");
    if (!h) return fail(MMG_ERR_ARG, "NULL argument");
    if (h->burnt) return fail(MMG_ERR_ARG, "mmg_diff_effects_open after the burn-in has started");
    if (h->tr) return fail(MMG_ERR_STATE, "tracing is open on this handle: traces and effects exclude each other");
    if (h->fx) return fail(MMG_ERR_STATE, "effects are open already");
    std::unique_ptr<DiffEffectsRows> X(new DiffEffectsRows());
    X->P = df_trace_table(h, nullptr, X->q.slot, &X->model_of);
    X->every = every; X->max_rows = max_rows;
    X->q.P = X->P; X->q.every = (int)every;
    HIP_TRY(hipSetDevice(h->device));
    const uint64_t count = (uint64_t)max_rows * X->P * h->F;
    HIP_TRY(X->d_rows.alloc(count));
    HIP_TRY(X->d_q.alloc(1));
    h->device_bytes += count * 8 + sizeof(DiffTrace);
    h->fx = std::move(X);
    return MMG_OK;
}

// iters sampling iterations from sampling index tt_first with rows recorded into the resident buffer: the launches of the untraced
// loop, k_df_run_traced in place of k_df_run.  The launch at index tt starts at row ceil(tt / every) and may fill the rest of the buffer.
static int df_sample_effects(mmg_diff *h, uint32_t it_first, uint32_t t_first, uint32_t tt_first, uint32_t iters)
{
    DiffEffectsRows &X = *h->fx;
    // (indices below 2^30 and intervals up to 2^30: the kernel's tt + every - 1 stays inside int)
    if ((uint64_t)tt_first + iters > (1u << 30)) return fail(MMG_ERR_ARG, "a recorded sampling phase takes at most 1073741824 iterations");
    if (((uint64_t)tt_first + iters + X.every - 1) / X.every > X.max_rows)
        return fail(MMG_ERR_ARG, "these iterations need more rows than mmg_diff_effects_open reserved (max_rows)");
    const size_t rowlen = (size_t)X.P * h->F;
    // the descriptors of this call's launches: sources of asynchronous copies, alive until the caller has synchronised
    std::vector<DiffTrace> q((iters + DF_CHUNK - 1) / DF_CHUNK, X.q);
    size_t i = 0;
    for (uint32_t j = 0; j < iters; j += DF_CHUNK, ++i) {
        const uint32_t n = iters - j < DF_CHUNK ? iters - j : DF_CHUNK, tt = tt_first + j;
        const uint32_t row0 = (uint32_t)(((uint64_t)tt + X.every - 1) / X.every);   // <= max_rows
        q[i].tr = X.d_rows.get() + (size_t)row0 * rowlen;
        q[i].tt0 = (int)tt; q[i].cap = (int)(X.max_rows - row0);
        HIP_TRY(hipMemcpyAsync(X.d_q.get(), &q[i], sizeof(DiffTrace), hipMemcpyHostToDevice, h->st.get()));
        hipLaunchKernelGGL(k_df_run_traced, dim3(df_blocks(h->F)), dim3(DF_BLOCK), 0, h->st.get(), h->p, it_first + j, (int)(t_first + j), (int)n, 2, 0,
                           (const DiffTrace *)X.d_q.get());
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipStreamSynchronize(h->st.get()));
    return MMG_OK;
}

extern "C" int mmg_diff_effects_summarize(mmg_diff *h, uint32_t np, const double *percentiles, mmg_effects **out)
{
    if (!h || !out) return fail(MMG_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (!h->fx) return fail(MMG_ERR_STATE, "mmg_diff_effects_summarize without mmg_diff_effects_open");
    if (!h->sampled) return fail(MMG_ERR_STATE, "mmg_diff_effects_summarize before a sampling row exists");
    const DiffEffectsRows &X = *h->fx;
    const uint32_t S = (uint32_t)(((uint64_t)h->sampled + X.every - 1) / X.every);
    const int rc = effects_check(S, (uint32_t)X.P, np, percentiles);
    if (rc) return rc;
    return effects_of_device_rows(h->device, S, (uint32_t)X.P, h->F, X.d_rows.get(), X.model_of.data(), np, percentiles, out);
}

extern "C" int mmg_diff_get_tune_state(mmg_diff *h, double *mean_lo, double *logitp)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL argument");
    if (!h->burnt) return fail(MMG_ERR_STATE, "mmg_diff_get_tune_state before mmg_diff_burnin");
    HIP_TRY(hipSetDevice(h->device));
    const size_t F = h->F;
    if (mean_lo) {
        HIP_TRY(hipMemcpy(mean_lo, h->d_st.get() + (size_t)h->p.LOsum * F, F * 8, hipMemcpyDeviceToHost));
        for (size_t f = 0; f < F; ++f) mean_lo[f] = mean_lo[f] / (double)DF_BATCH;
    }
    if (logitp) HIP_TRY(hipMemcpy(logitp, h->d_st.get() + (size_t)h->p.logitp * F, F * 8, hipMemcpyDeviceToHost));
    return MMG_OK;
}

extern "C" int mmg_diff_get_pseudo(mmg_diff *h, double *out)
{
    if (!h || !out) return fail(MMG_ERR_ARG, "NULL argument");
    if (!h->burnt) return fail(MMG_ERR_STATE, "mmg_diff_get_pseudo before mmg_diff_burnin");
    HIP_TRY(hipSetDevice(h->device));
    const size_t F = h->F;
    size_t col = 0;
    auto slot = [&](int o) { return hipMemcpy(out + col++ * F, h->d_st.get() + (size_t)o * F, F * 8, hipMemcpyDeviceToHost); };
    for (int mi = 0; mi < 2; ++mi) {
        const DiffModel &m = h->p.m[mi];
        HIP_TRY(slot(m.A)); HIP_TRY(slot(m.Va));
        for (int k = 0; k < h->p.K; ++k) { HIP_TRY(slot(m.B + k)); HIP_TRY(slot(m.Vb + k)); }
        for (int l = 0; l < m.L; ++l) {
            HIP_TRY(slot(m.Fm + l)); HIP_TRY(slot(m.Ve + l)); HIP_TRY(slot(m.Si + l));
            double *S = out + (col - 1) * F;   // the file's S is 1 / S_inv
            for (size_t f = 0; f < F; ++f) S[f] = 1.0 / S[f];
        }
        for (int c = 0; c < m.nc; ++c) { HIP_TRY(slot(m.J + c)); HIP_TRY(slot(m.Lm + c)); }
        HIP_TRY(slot(m.Q)); HIP_TRY(slot(m.R));
    }
    return MMG_OK;
}

extern "C" int mmg_diff_burnin(mmg_diff *h, uint32_t iters)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL argument");
    if (h->burnt) return fail(MMG_ERR_STATE, "the burn-in has run already");
    if (h->tr && h->tr->stopped) return fail(MMG_ERR_STATE, "the trace sink stopped this run");
    // (the pseudopriors are the variances of iters - 102 recorded iterations: two of them at least)
    if (iters < (uint32_t)DF_REC_FROM + 2) return fail(MMG_ERR_ARG, "burn-in iterations must be at least 104");
    HIP_TRY(hipSetDevice(h->device));
    if (h->tr) {
        const int rc = df_run_traced(h, 0, 0, 0, 0, iters);
        if (rc) return rc;
    } else {
        for (uint32_t t = 0; t < iters; t += DF_CHUNK) {
            const uint32_t n = iters - t < DF_CHUNK ? iters - t : DF_CHUNK;
            hipLaunchKernelGGL(k_df_run, dim3(df_blocks(h->F)), dim3(DF_BLOCK), 0, h->st.get(), h->p, t, (int)t, (int)n, 0, DF_REC_FROM);
        }
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
    if (h->tr && h->tr->stopped) return fail(MMG_ERR_STATE, "the trace sink stopped this run");
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
    if (h->tr && h->tr->stopped) return fail(MMG_ERR_STATE, "the trace sink stopped this run");
    HIP_TRY(hipSetDevice(h->device));
    const uint32_t t_first = h->batches * DF_BATCH + h->sampled;
    if (h->tr) {
        const int rc = df_run_traced(h, 1, h->burnin + t_first, t_first, h->sampled, iters);
        if (rc) return rc;
    } else if (h->fx) {
        const int rc = df_sample_effects(h, h->burnin + t_first, t_first, h->sampled, iters);
        if (rc) return rc;
    } else {
        for (uint32_t j = 0; j < iters; j += DF_CHUNK) {
            const uint32_t n = iters - j < DF_CHUNK ? iters - j : DF_CHUNK;
            hipLaunchKernelGGL(k_df_run, dim3(df_blocks(h->F)), dim3(DF_BLOCK), 0, h->st.get(), h->p, h->burnin + t_first + j, (int)(t_first + j), (int)n, 2, 0);
        }
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
    return df_results(h->p, h->d_st.get(), h->F, h->K, h->L, h->sampled, gamma_mean, logitp, alpha, beta, eta);
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

// ---- what the handles of several replicas share on the host ---------------------------------------------------------------------
// A replica is a comparison of mmg_diff_poly_*, a chain of mmg_diff_chains_* or a data set of mmg_diff_perm_*.  Per replica a DiffParams
// (in h_p and, for the kernels, in d_p) with its own state block and gam / tuned; what else is its own is the handle's business.  The
// launches cover every replica (grid.y); each replica tunes on its own: one whose untuned count reached 0 has ended, leaves the tuning
// launches and keeps its batch count nb, and its sampling stream index starts at burnin + 128 * nb (h_off / d_off).
// `entry` and `unit` are the handle's words in the messages: "mmg_diff_poly" and "comparison".
static_assert(sizeof(DiffParams) == 480, "mmg_diff_poly_device_bytes is documented with this size (DESIGN.md section 10)");
constexpr uint32_t DF_RMAX = 32;   // k_dfp_tune's `active` mask has 32 bits

struct DiffReplicas {
    const std::string entry, unit;
    DevStream st;
    int device = 0;
    uint32_t F = 0, R = 0;
    uint32_t sample_total = 0;         // chains: the whole sampling length, which sample() may not pass (0: no such length)
    std::vector<DiffParams> h_p;
    std::vector<uint32_t> h_off, nb;   // per replica: 128 * (its batches); its batches
    std::vector<char> ended;
    DevBuf<DiffParams> d_p;
    DevBuf<uint32_t> d_off;
    DevBuf<int> d_cnt;                 // [R]
    uint32_t burnin = 0, batches = 0, sampled = 0;
    bool burnt = false;
    uint64_t device_bytes = 0;

    DiffReplicas(const char *entry_, const char *unit_) : entry(entry_), unit(unit_) {}
    virtual ~DiffReplicas() = default;
    // (a handle's destructor calls this first: its own buffers go before the members above, and none while the stream still runs)
    void drain() { if (st) (void)hipStreamSynchronize(st.get()); }
    dim3 grid() const { return dim3(df_blocks(F), R); }

    template <typename B> hipError_t dalloc(B &buf, uint64_t count)
    {
        HIPE_TRY(buf.alloc(count));
        device_bytes += count * sizeof(*buf.get());
        return hipSuccess;
    }

    // the stream and the per-replica arrays of a new handle
    int start(int device_, uint32_t F_, uint32_t R_)
    {
        device = device_; F = F_; R = R_;
        h_p.resize(R);
        h_off.assign(R, 0);
        nb.assign(R, 0);
        ended.assign(R, 0);
        HIP_TRY(hipSetDevice(device));
        HIP_TRY(st.create(hipStreamNonBlocking));
        HIP_TRY(dalloc(d_p, R));
        HIP_TRY(dalloc(d_off, R));
        HIP_TRY(dalloc(d_cnt, R));
        return MMG_OK;
    }

    // h_p, complete, to the device and every offset 0: in stream order, ahead of the handle's init launch
    int upload_params()
    {
        HIP_TRY(hipMemcpyAsync(d_p.get(), h_p.data(), (size_t)R * sizeof(DiffParams), hipMemcpyHostToDevice, st.get()));
        HIP_TRY(hipMemsetAsync(d_off.get(), 0, (size_t)R * 4, st.get()));
        return MMG_OK;
    }

    // One launch of n iterations of every replica.  t: the burn-in or sampling index of the first one; k_dfp_run needs none in sampling.
    virtual void launch_run(uint32_t it0, int t, int n, int mode, int rec_from)
    {
        hipLaunchKernelGGL(k_dfp_run, grid(), dim3(DF_BLOCK), 0, st.get(), d_p.get(), d_off.get(), it0, mode == 2 ? 0 : t, n, mode, rec_from);
    }

    int run_burnin(uint32_t iters)
    {
        if (burnt) return fail(MMG_ERR_STATE, "the burn-in has run already");
        if (iters == 0 || iters % 1024) return fail(MMG_ERR_ARG, "burn-in iterations must be a positive multiple of 1024");
        HIP_TRY(hipSetDevice(device));
        for (uint32_t t = 0; t < iters; t += DF_CHUNK) {
            const uint32_t n = iters - t < DF_CHUNK ? iters - t : DF_CHUNK;
            launch_run(t, (int)t, (int)n, 0, DF_REC_FROM);
        }
        hipLaunchKernelGGL(k_dfp_pseudo, grid(), dim3(DF_BLOCK), 0, st.get(), d_p.get(), (double)(iters - DF_REC_FROM));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st.get()));
        burnin = iters;
        burnt = true;
        return MMG_OK;
    }

    int tune_batch(uint32_t *untuned, int32_t *ended_out)
    {
        if (!untuned) return fail(MMG_ERR_ARG, "NULL argument");
        if (!burnt) return fail(MMG_ERR_STATE, entry + "_tune_batch before " + entry + "_burnin");
        if (sampled) return fail(MMG_ERR_STATE, entry + "_tune_batch after sampling has started");
        uint32_t active = 0;
        for (uint32_t r = 0; r < R; ++r)
            if (!ended[r]) active |= 1u << r;
        for (uint32_t r = 0; r < R; ++r) untuned[r] = 0;
        if (active) {
            HIP_TRY(hipSetDevice(device));
            HIP_TRY(hipMemsetAsync(d_cnt.get(), 0, (size_t)R * 4, st.get()));
            const uint32_t it0 = burnin + batches * DF_BATCH;
            hipLaunchKernelGGL(k_dfp_tune, grid(), dim3(DF_BLOCK), 0, st.get(), d_p.get(), active, it0, (int)batches, d_cnt.get());
            HIP_TRY(hipGetLastError());
            int cnt[DF_RMAX] = {0};
            HIP_TRY(hipMemcpyAsync(cnt, d_cnt.get(), (size_t)R * 4, hipMemcpyDeviceToHost, st.get()));
            HIP_TRY(hipStreamSynchronize(st.get()));
            ++batches;
            for (uint32_t r = 0; r < R; ++r) {
                if (ended[r]) continue;
                nb[r] = batches;
                untuned[r] = (uint32_t)cnt[r];
                if (cnt[r] == 0) ended[r] = 1;
            }
        }
        if (ended_out)
            for (uint32_t r = 0; r < R; ++r) ended_out[r] = ended[r] ? 1 : 0;
        return MMG_OK;
    }

    int sample(uint32_t iters)
    {
        if (!burnt) return fail(MMG_ERR_STATE, entry + "_sample before " + entry + "_burnin");
        if (iters == 0) return fail(MMG_ERR_ARG, "iters must be positive");
        // (chains: the batch slot of sampling index t is t / (T / 16) < 16 only while t < T)
        if (sample_total && iters > sample_total - sampled)
            return fail(MMG_ERR_ARG, "sampling beyond the total sampling length the handle was created with");
        HIP_TRY(hipSetDevice(device));
        if (!sampled) {
            // replica r's sampling starts at its own running index, burnin + 128 * (its batches)
            for (uint32_t r = 0; r < R; ++r) h_off[r] = nb[r] * DF_BATCH;
            HIP_TRY(hipMemcpyAsync(d_off.get(), h_off.data(), (size_t)R * 4, hipMemcpyHostToDevice, st.get()));
        }
        for (uint32_t j = 0; j < iters; j += DF_CHUNK) {
            const uint32_t n = iters - j < DF_CHUNK ? iters - j : DF_CHUNK;
            launch_run(burnin + sampled + j, (int)(sampled + j), (int)n, 2, 0);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(st.get()));
        sampled += iters;
        return MMG_OK;
    }

    int results(uint32_t r, double *gamma_mean, double *logitp, double *alpha, double *beta, double *eta)
    {
        if (r >= R) return fail(MMG_ERR_ARG, "no such " + unit);
        if (!sampled) return fail(MMG_ERR_STATE, entry + "_get_results before " + entry + "_sample");
        HIP_TRY(hipSetDevice(device));
        const DiffParams &p = h_p[r];
        const uint32_t L[2] = {(uint32_t)p.m[0].L, (uint32_t)p.m[1].L};
        return df_results(p, p.st, F, (uint32_t)p.K, L, sampled, gamma_mean, logitp, alpha, beta, eta);
    }

    int info(uint32_t r, int32_t *flags, uint32_t *n_classes, uint32_t *batches_out, int32_t *ended_out) const
    {
        if (r >= R) return fail(MMG_ERR_ARG, "no such " + unit);
        const DiffParams &p = h_p[r];
        if (flags) { flags[0] = p.Mnil; flags[1] = p.m[0].Pnil; flags[2] = p.m[1].Pnil; }
        if (n_classes) { n_classes[0] = (uint32_t)p.m[0].nc; n_classes[1] = (uint32_t)p.m[1].nc; }
        if (batches_out) *batches_out = nb[r];
        if (ended_out) *ended_out = ended[r] ? 1 : 0;
        return MMG_OK;
    }
};

static int df_null() { return fail(MMG_ERR_ARG, "NULL argument"); }

static int df_device_bytes(const DiffReplicas *h, uint64_t *bytes)
{
    if (!h || !bytes) return df_null();
    *bytes = h->device_bytes;
    return MMG_OK;
}

// ---- several alternatives against one model 0 on one handle -----------------------------------------------------------------
// y / e^2 / M / P0 once; per comparison its own slot layout, state block, gam / tuned, P1 and class table.
struct mmg_diff_poly : DiffReplicas {
    struct Cmp {
        DevBuf<double> d_st, d_P1;
        DevBuf<int> d_C, d_gam, d_tuned;
    };
    DevBuf<double> d_y, d_esq, d_M, d_P0;
    std::vector<Cmp> cmp;
    mmg_diff_poly() : DiffReplicas("mmg_diff_poly", "comparison") {}
    ~mmg_diff_poly() { drain(); }
};

extern "C" int mmg_diff_poly_create(int device, uint32_t F, uint32_t N, const double *y, const double *e, uint32_t K, const double *M,
                                    uint32_t L0, const double *P0, const int32_t *C0, uint32_t J, const uint32_t *L1, const double *P1,
                                    const int32_t *C1, double d, double s, double pdash, int fixalpha, uint64_t seed, mmg_diff_poly **out)
{
    if (!out || !y || !e || !M || !P0 || !C0 || !L1 || !P1 || !C1) return df_null();
    *out = nullptr;
    int rc;
    if ((rc = df_check_shape(F, N, K))) return rc;
    if (J < 1 || J > (uint32_t)DF_JMAX) return fail(MMG_ERR_ARG, "the number of comparisons must be between 1 and 16");
    if ((rc = df_check_cols(L0, J, L1))) return rc;
    uint64_t sumL1 = 0;
    for (uint32_t c = 0; c < J; ++c) sumL1 += L1[c];
    if ((rc = df_check_prior(d, s, pdash)) || (rc = df_check_finite(F, N, y, e, K, M, L0, P0, sumL1, P1))) return rc;
    int nc0 = 0;
    if ((rc = df_classes(C0, 1, N, &nc0))) return rc;
    std::vector<int> nc1(J, 0);
    for (uint32_t c = 0; c < J; ++c)
        if ((rc = df_classes(C1 + (size_t)c * N, 1, N, &nc1[c]))) return rc;
    if ((rc = require_device(device))) return rc;

    std::unique_ptr<mmg_diff_poly> h(new mmg_diff_poly());
    h->cmp.resize(J);
    if ((rc = h->start(device, F, J))) return rc;
    const hipStream_t st = h->st.get();
    const uint64_t FN = (uint64_t)F * N;
    HIP_TRY(h->dalloc(h->d_y, FN));
    HIP_TRY(h->dalloc(h->d_esq, FN));
    HIP_TRY(h->dalloc(h->d_M, (uint64_t)N * K));
    HIP_TRY(h->dalloc(h->d_P0, (uint64_t)N * L0));
    DiffStaged staged;                     // (this and hC: sources of asynchronous copies, alive until the synchronize below)
    std::vector<std::vector<int>> hC(J);
    if ((rc = df_upload_transposed(st, F, N, y, e, h->d_y.get(), h->d_esq.get(), staged))) return rc;
    HIP_TRY(hipMemcpyAsync(h->d_M.get(), M, (size_t)N * K * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->d_P0.get(), P0, (size_t)N * L0 * 8, hipMemcpyHostToDevice, st));
    const double *P1c = P1;
    for (uint32_t c = 0; c < J; ++c) {
        mmg_diff_poly::Cmp &q = h->cmp[c];
        DiffParams &p = h->h_p[c];
        p = df_params(F, N, K, M, L0, P0, L1[c], P1c, d, s, fixalpha, seed);
        const uint32_t L[2] = {L0, L1[c]};
        const int nc[2] = {nc0, nc1[c]};
        const size_t nslot = df_layout(p, L, nc);
        HIP_TRY(h->dalloc(q.d_st, (uint64_t)nslot * F));
        HIP_TRY(h->dalloc(q.d_P1, (uint64_t)N * L1[c]));
        HIP_TRY(h->dalloc(q.d_C, (uint64_t)N * 2));
        HIP_TRY(h->dalloc(q.d_gam, (uint64_t)F));
        HIP_TRY(h->dalloc(q.d_tuned, (uint64_t)F));
        hC[c].resize((size_t)N * 2);
        for (uint32_t i = 0; i < N; ++i) { hC[c][i * 2] = C0[i]; hC[c][i * 2 + 1] = C1[(size_t)c * N + i]; }
        HIP_TRY(hipMemcpyAsync(q.d_P1.get(), P1c, (size_t)N * L1[c] * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(q.d_C.get(), hC[c].data(), (size_t)N * 2 * 4, hipMemcpyHostToDevice, st));
        p.M = h->d_M.get(); p.m[0].P = h->d_P0.get(); p.m[1].P = q.d_P1.get(); p.Cl = q.d_C.get();
        p.y = h->d_y.get(); p.esq = h->d_esq.get(); p.st = q.d_st.get(); p.gam = q.d_gam.get(); p.tuned = q.d_tuned.get();
        P1c += (size_t)N * L1[c];
    }
    if ((rc = h->upload_params())) return rc;
    const double logitp0 = std::log(pdash) - std::log(1.0 - pdash);
    hipLaunchKernelGGL(k_dfp_init, h->grid(), dim3(DF_BLOCK), 0, st, h->d_p.get(), logitp0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    *out = h.release();
    return MMG_OK;
}

extern "C" int mmg_diff_poly_burnin(mmg_diff_poly *h, uint32_t iters) { return h ? h->run_burnin(iters) : df_null(); }

extern "C" int mmg_diff_poly_tune_batch(mmg_diff_poly *h, uint32_t *untuned, int32_t *ended) { return h ? h->tune_batch(untuned, ended) : df_null(); }

extern "C" int mmg_diff_poly_sample(mmg_diff_poly *h, uint32_t iters) { return h ? h->sample(iters) : df_null(); }

extern "C" int mmg_diff_poly_get_results(mmg_diff_poly *h, uint32_t j, double *gamma_mean, double *logitp, double *alpha, double *beta, double *eta)
{
    return h ? h->results(j, gamma_mean, logitp, alpha, beta, eta) : df_null();
}

extern "C" int mmg_diff_poly_info(mmg_diff_poly *h, uint32_t j, int32_t *flags, uint32_t *n_classes, uint32_t *batches, int32_t *ended)
{
    return h ? h->info(j, flags, n_classes, batches, ended) : df_null();
}

extern "C" int mmg_diff_poly_device_bytes(mmg_diff_poly *h, uint64_t *bytes) { return df_device_bytes(h, bytes); }

extern "C" void mmg_diff_poly_destroy(mmg_diff_poly *h) { delete h; }

// ---- several chains of one comparison on one handle ---------------------------------------------------------------------------
// y / e^2 / M / P0 / P1 and the class table once; per chain a DiffParams (chain c in the stream key), a state block of nslot + DF_NB slots
// (the last DF_NB: the batch sums of gamma), gam / tuned.  The run launches are k_dfc_run, which fills the batch slots in sampling.
struct mmg_diff_chains : DiffReplicas {
    size_t nslot = 0, npool = 0;   // slots per feature of one chain (without the batch slots) and of the pooled output
    DevBuf<double> d_y, d_esq, d_M, d_P0, d_P1, d_st, d_pool;
    DevBuf<int> d_C, d_gam, d_tuned;
    bool pooled = false;
    mmg_diff_chains() : DiffReplicas("mmg_diff_chains", "chain") {}
    ~mmg_diff_chains() { drain(); }
    int gb() const { return (int)nslot; }
    // in sampling t is the sampling index of the launch's first iteration, the same for every chain
    void launch_run(uint32_t it0, int t, int n, int mode, int rec_from) override
    {
        hipLaunchKernelGGL(k_dfc_run, grid(), dim3(DF_BLOCK), 0, st.get(), d_p.get(), d_off.get(), it0, t, n, mode, rec_from, gb(),
                           (int)(sample_total / DF_NB));
    }
};

extern "C" int mmg_diff_chains_create(int device, uint32_t F, uint32_t N, const double *y, const double *e, uint32_t K, const double *M,
                                      uint32_t L0, const double *P0, uint32_t L1, const double *P1, const int32_t *C, double d, double s,
                                      double pdash, int fixalpha, uint64_t seed, uint32_t n_chains, uint32_t sample_total, mmg_diff_chains **out)
{
    if (!out || !y || !e || !M || !P0 || !P1 || !C) return df_null();
    *out = nullptr;
    int nc[2] = {0, 0}, rc;
    if ((rc = df_check_shape(F, N, K)) || (rc = df_check_cols(L0, 1, &L1))) return rc;
    if (n_chains < 1 || n_chains > (uint32_t)DF_CHAINS_MAX) return fail(MMG_ERR_ARG, "the number of chains must be between 1 and 16");
    if (sample_total == 0 || sample_total % DF_NB || sample_total > 0x7fffffffu)
        return fail(MMG_ERR_ARG, "the total sampling length must be a positive multiple of 16");
    if ((rc = df_check_prior(d, s, pdash)) || (rc = df_check_finite(F, N, y, e, K, M, L0, P0, L1, P1)) || (rc = df_check_classes(C, N, nc))
        || (rc = require_device(device)))
        return rc;

    std::unique_ptr<mmg_diff_chains> h(new mmg_diff_chains());
    h->sample_total = sample_total;
    DiffParams p = df_params(F, N, K, M, L0, P0, L1, P1, d, s, fixalpha, seed);
    const uint32_t L[2] = {L0, L1};
    h->nslot = df_layout(p, L, nc);
    h->npool = (size_t)DF_POOL_STATS + 2 * (size_t)(2 + 2 * K + L0 + L1);
    const uint64_t per_chain = (uint64_t)(h->nslot + DF_NB) * F;   // doubles of one chain's state block

    if ((rc = h->start(device, F, n_chains))) return rc;
    const hipStream_t st = h->st.get();
    HIP_TRY(h->dalloc(h->d_y, (uint64_t)F * N));
    HIP_TRY(h->dalloc(h->d_esq, (uint64_t)F * N));
    HIP_TRY(h->dalloc(h->d_M, (uint64_t)N * K));
    HIP_TRY(h->dalloc(h->d_P0, (uint64_t)N * L0));
    HIP_TRY(h->dalloc(h->d_P1, (uint64_t)N * L1));
    HIP_TRY(h->dalloc(h->d_C, (uint64_t)N * 2));
    HIP_TRY(h->dalloc(h->d_st, per_chain * n_chains));
    HIP_TRY(h->dalloc(h->d_gam, (uint64_t)F * n_chains));
    HIP_TRY(h->dalloc(h->d_tuned, (uint64_t)F * n_chains));
    HIP_TRY(h->dalloc(h->d_pool, (uint64_t)h->npool * F));
    DiffStaged staged;   // (sources of asynchronous copies: alive until the synchronize below)
    if ((rc = df_upload_transposed(st, F, N, y, e, h->d_y.get(), h->d_esq.get(), staged))) return rc;
    HIP_TRY(hipMemcpyAsync(h->d_M.get(), M, (size_t)N * K * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->d_P0.get(), P0, (size_t)N * L0 * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->d_P1.get(), P1, (size_t)N * L1 * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->d_C.get(), C, (size_t)N * 2 * 4, hipMemcpyHostToDevice, st));
    p.M = h->d_M.get(); p.m[0].P = h->d_P0.get(); p.m[1].P = h->d_P1.get(); p.Cl = h->d_C.get();
    p.y = h->d_y.get(); p.esq = h->d_esq.get();
    for (uint32_t c = 0; c < n_chains; ++c) {
        DiffParams &q = h->h_p[c];
        q = p;
        q.chain = (int)c;
        q.st = h->d_st.get() + per_chain * c;
        q.gam = h->d_gam.get() + (size_t)F * c;
        q.tuned = h->d_tuned.get() + (size_t)F * c;
    }
    if ((rc = h->upload_params())) return rc;
    const double logitp0 = std::log(pdash) - std::log(1.0 - pdash);
    hipLaunchKernelGGL(k_dfc_init, h->grid(), dim3(DF_BLOCK), 0, st, h->d_p.get(), logitp0, h->gb());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    *out = h.release();
    return MMG_OK;
}

extern "C" int mmg_diff_chains_burnin(mmg_diff_chains *h, uint32_t iters) { return h ? h->run_burnin(iters) : df_null(); }

extern "C" int mmg_diff_chains_tune_batch(mmg_diff_chains *h, uint32_t *untuned, int32_t *ended) { return h ? h->tune_batch(untuned, ended) : df_null(); }

extern "C" int mmg_diff_chains_sample(mmg_diff_chains *h, uint32_t iters)
{
    if (!h) return df_null();
    const int rc = h->sample(iters);
    if (!rc) h->pooled = false;
    return rc;
}

extern "C" int mmg_diff_chains_pool(mmg_diff_chains *h)
{
    if (!h) return df_null();
    if (h->sampled != h->sample_total) return fail(MMG_ERR_STATE, "mmg_diff_chains_pool before the total sampling length has been sampled");
    HIP_TRY(hipSetDevice(h->device));
    hipLaunchKernelGGL(k_dfc_pool, dim3(df_blocks(h->F)), dim3(DF_BLOCK), 0, h->st.get(), h->d_p.get(), (int)h->R, (int)h->sample_total, h->gb(),
                       h->d_pool.get());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->st.get()));
    h->pooled = true;
    return MMG_OK;
}

extern "C" int mmg_diff_chains_get_results(mmg_diff_chains *h, uint32_t c, double *gamma_mean, double *logitp, double *alpha, double *beta, double *eta)
{
    return h ? h->results(c, gamma_mean, logitp, alpha, beta, eta) : df_null();
}

extern "C" int mmg_diff_chains_get_batch_sums(mmg_diff_chains *h, uint32_t c, double *sums)
{
    if (!h || !sums) return df_null();
    if (c >= h->R) return fail(MMG_ERR_ARG, "no such chain");
    if (!h->sampled) return fail(MMG_ERR_STATE, "mmg_diff_chains_get_batch_sums before mmg_diff_chains_sample");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpy(sums, h->h_p[c].st + h->nslot * h->F, (size_t)DF_NB * h->F * 8, hipMemcpyDeviceToHost));
    return MMG_OK;
}

extern "C" int mmg_diff_chains_get_pooled(mmg_diff_chains *h, double *log_bf, double *log_bf_sd, double *log_bf_mcse, uint32_t *chains_mixed,
                                          double *alpha, double *beta, double *eta)
{
    if (!h) return df_null();
    if (!h->pooled) return fail(MMG_ERR_STATE, "mmg_diff_chains_get_pooled before mmg_diff_chains_pool");
    HIP_TRY(hipSetDevice(h->device));
    const size_t F = h->F;
    std::vector<double> v(h->npool * F);
    HIP_TRY(hipMemcpy(v.data(), h->d_pool.get(), v.size() * 8, hipMemcpyDeviceToHost));
    for (size_t f = 0; f < F; ++f) {
        if (log_bf) log_bf[f] = v[f];
        if (log_bf_sd) log_bf_sd[f] = v[F + f];
        if (log_bf_mcse) log_bf_mcse[f] = v[2 * F + f];
        if (chains_mixed) chains_mixed[f] = (uint32_t)v[3 * F + f];
    }
    // the means: summed sums / summed counts, the quotient on the host as df_results takes it
    const DiffParams &p = h->h_p[0];
    const size_t nq[3] = {2, 2 * (size_t)p.K, (size_t)p.m[0].L + (size_t)p.m[1].L};
    double *dst[3] = {alpha, beta, eta};
    size_t q = 0;
    for (int a = 0; a < 3; ++a)
        for (size_t i = 0; i < nq[a]; ++i, ++q) {
            if (!dst[a]) continue;
            const double *S = &v[(DF_POOL_STATS + 2 * q) * F], *Nn = &v[(DF_POOL_STATS + 2 * q + 1) * F];
            for (size_t f = 0; f < F; ++f) dst[a][i * F + f] = S[f] / Nn[f];
        }
    return MMG_OK;
}

extern "C" int mmg_diff_chains_info(mmg_diff_chains *h, uint32_t c, int32_t *flags, uint32_t *n_classes, uint32_t *batches, int32_t *ended)
{
    return h ? h->info(c, flags, n_classes, batches, ended) : df_null();
}

extern "C" int mmg_diff_chains_device_bytes(mmg_diff_chains *h, uint64_t *bytes) { return df_device_bytes(h, bytes); }

extern "C" void mmg_diff_chains_destroy(mmg_diff_chains *h) { delete h; }

// ---- a permutation null: the data and B shuffled copies of it on one handle ----------------------------------------------------
// M / P0 / P1 and the class table once; per replica its y / e^2 ([R][N][F]: replica 0 as given, replica b >= 1 shuffled by
// k_dfq_shuffle), a DiffParams (replica b in the stream key), a state block, gam / tuned.  stat / null_ge / q: what
// mmg_diff_perm_qvalues leaves on the device.
constexpr uint32_t DF_PERM_MAX = DF_RMAX - 1;   // the data and 31 shuffles

struct mmg_diff_perm : DiffReplicas {
    size_t nslot = 0;
    DevBuf<double> d_y, d_esq, d_M, d_P0, d_P1, d_st, d_stat, d_q;
    DevBuf<uint64_t> d_null_ge;
    DevBuf<int> d_C, d_gam, d_tuned;
    bool have_q = false;
    mmg_diff_perm() : DiffReplicas("mmg_diff_perm", "replica") {}
    ~mmg_diff_perm() { drain(); }
};

extern "C" int mmg_diff_perm_create(int device, uint32_t F, uint32_t N, const double *y, const double *e, uint32_t K, const double *M,
                                    uint32_t L0, const double *P0, uint32_t L1, const double *P1, const int32_t *C, double d, double s,
                                    double pdash, int fixalpha, uint64_t seed, uint32_t n_perm, mmg_diff_perm **out)
{
    if (!out || !y || !e || !M || !P0 || !P1 || !C) return df_null();
    *out = nullptr;
    int nc[2] = {0, 0}, rc;
    if ((rc = df_check_shape(F, N, K)) || (rc = df_check_cols(L0, 1, &L1))) return rc;
    if (n_perm < 1 || n_perm > DF_PERM_MAX) return fail(MMG_ERR_ARG, "the number of permutations must be between 1 and 31");
    if ((rc = df_check_prior(d, s, pdash)) || (rc = df_check_finite(F, N, y, e, K, M, L0, P0, L1, P1)) || (rc = df_check_classes(C, N, nc))
        || (rc = require_device(device)))
        return rc;

    const uint32_t R = n_perm + 1;
    std::unique_ptr<mmg_diff_perm> h(new mmg_diff_perm());
    DiffParams p = df_params(F, N, K, M, L0, P0, L1, P1, d, s, fixalpha, seed);
    const uint32_t L[2] = {L0, L1};
    h->nslot = df_layout(p, L, nc);
    const uint64_t FN = (uint64_t)F * N, per_replica = (uint64_t)h->nslot * F;

    if ((rc = h->start(device, F, R))) return rc;
    const hipStream_t st = h->st.get();
    HIP_TRY(h->dalloc(h->d_y, FN * R));
    HIP_TRY(h->dalloc(h->d_esq, FN * R));
    HIP_TRY(h->dalloc(h->d_M, (uint64_t)N * K));
    HIP_TRY(h->dalloc(h->d_P0, (uint64_t)N * L0));
    HIP_TRY(h->dalloc(h->d_P1, (uint64_t)N * L1));
    HIP_TRY(h->dalloc(h->d_C, (uint64_t)N * 2));
    HIP_TRY(h->dalloc(h->d_st, per_replica * R));
    HIP_TRY(h->dalloc(h->d_gam, (uint64_t)F * R));
    HIP_TRY(h->dalloc(h->d_tuned, (uint64_t)F * R));
    HIP_TRY(h->dalloc(h->d_stat, (uint64_t)F * R));
    HIP_TRY(h->dalloc(h->d_q, (uint64_t)F));
    HIP_TRY(h->dalloc(h->d_null_ge, (uint64_t)F));
    // replica 0 as mmg_diff_create holds the data, copied on the device to every other replica and shuffled there
    DiffStaged staged;   // (sources of asynchronous copies: alive until the synchronize below)
    if ((rc = df_upload_transposed(st, F, N, y, e, h->d_y.get(), h->d_esq.get(), staged))) return rc;
    for (uint32_t b = 1; b < R; ++b) {
        HIP_TRY(hipMemcpyAsync(h->d_y.get() + FN * b, h->d_y.get(), FN * 8, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(h->d_esq.get() + FN * b, h->d_esq.get(), FN * 8, hipMemcpyDeviceToDevice, st));
    }
    hipLaunchKernelGGL(k_dfq_shuffle, dim3(df_blocks(F), n_perm), dim3(DF_BLOCK), 0, st, h->d_y.get(), h->d_esq.get(), (int)F, (int)N, seed);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h->d_M.get(), M, (size_t)N * K * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->d_P0.get(), P0, (size_t)N * L0 * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->d_P1.get(), P1, (size_t)N * L1 * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(h->d_C.get(), C, (size_t)N * 2 * 4, hipMemcpyHostToDevice, st));
    p.M = h->d_M.get(); p.m[0].P = h->d_P0.get(); p.m[1].P = h->d_P1.get(); p.Cl = h->d_C.get();
    for (uint32_t b = 0; b < R; ++b) {
        DiffParams &q = h->h_p[b];
        q = p;
        q.chain = (int)b;
        q.y = h->d_y.get() + FN * b;
        q.esq = h->d_esq.get() + FN * b;
        q.st = h->d_st.get() + per_replica * b;
        q.gam = h->d_gam.get() + (size_t)F * b;
        q.tuned = h->d_tuned.get() + (size_t)F * b;
    }
    if ((rc = h->upload_params())) return rc;
    const double logitp0 = std::log(pdash) - std::log(1.0 - pdash);
    hipLaunchKernelGGL(k_dfp_init, h->grid(), dim3(DF_BLOCK), 0, st, h->d_p.get(), logitp0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    *out = h.release();
    return MMG_OK;
}

extern "C" int mmg_diff_perm_burnin(mmg_diff_perm *h, uint32_t iters) { return h ? h->run_burnin(iters) : df_null(); }

extern "C" int mmg_diff_perm_tune_batch(mmg_diff_perm *h, uint32_t *untuned, int32_t *ended) { return h ? h->tune_batch(untuned, ended) : df_null(); }

extern "C" int mmg_diff_perm_sample(mmg_diff_perm *h, uint32_t iters)
{
    if (!h) return df_null();
    const int rc = h->sample(iters);
    if (!rc) h->have_q = false;
    return rc;
}

extern "C" int mmg_diff_perm_get_results(mmg_diff_perm *h, uint32_t b, double *gamma_mean, double *logitp, double *alpha, double *beta, double *eta)
{
    return h ? h->results(b, gamma_mean, logitp, alpha, beta, eta) : df_null();
}

extern "C" int mmg_diff_perm_info(mmg_diff_perm *h, uint32_t b, int32_t *flags, uint32_t *n_classes, uint32_t *batches, int32_t *ended)
{
    return h ? h->info(b, flags, n_classes, batches, ended) : df_null();
}

extern "C" int mmg_diff_perm_qvalues(mmg_diff_perm *h)
{
    if (!h) return df_null();
    if (!h->sampled) return fail(MMG_ERR_STATE, "mmg_diff_perm_qvalues before mmg_diff_perm_sample");
    HIP_TRY(hipSetDevice(h->device));
    const DiffParams &p = h->h_p[0];
    int rc = qvalue_stat_on_device(h->st.get(), h->d_st.get(), h->nslot * (size_t)h->F, p.gsum, p.logitp, h->F, h->R, h->sampled, h->d_stat.get());
    if (rc) return rc;
    // replica 0's statistics against those of replicas 1 .. B, which follow them in d_stat
    rc = qvalues_on_device(h->st.get(), h->F, h->d_stat.get(), (uint64_t)(h->R - 1) * h->F, h->d_stat.get() + h->F, h->d_null_ge.get(), h->d_q.get());
    if (rc) { (void)hipStreamSynchronize(h->st.get()); return rc; }
    h->have_q = true;
    return MMG_OK;
}

extern "C" int mmg_diff_perm_get_qvalues(mmg_diff_perm *h, double *stat, uint64_t *null_ge, double *q)
{
    if (!h) return df_null();
    if (!h->have_q) return fail(MMG_ERR_STATE, "mmg_diff_perm_get_qvalues before mmg_diff_perm_qvalues");
    HIP_TRY(hipSetDevice(h->device));
    const size_t F = h->F;
    if (stat) HIP_TRY(hipMemcpy(stat, h->d_stat.get(), (size_t)h->R * F * 8, hipMemcpyDeviceToHost));
    if (null_ge) HIP_TRY(hipMemcpy(null_ge, h->d_null_ge.get(), F * 8, hipMemcpyDeviceToHost));
    if (q) HIP_TRY(hipMemcpy(q, h->d_q.get(), F * 8, hipMemcpyDeviceToHost));
    return MMG_OK;
}

extern "C" int mmg_diff_perm_device_bytes(mmg_diff_perm *h, uint64_t *bytes) { return df_device_bytes(h, bytes); }

extern "C" void mmg_diff_perm_destroy(mmg_diff_perm *h) { delete h; }
