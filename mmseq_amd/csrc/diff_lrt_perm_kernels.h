// diff_lrt_perm_kernels.h -- mmdiff -lrt FILE -lrtperm B: the likelihood-ratio test on B shuffled copies of the data (DESIGN.md
// section 10.6).
//
// k_lrt_perm: one lane per (copy, feature), blocks of LRT_BLOCK lanes over the features, blockIdx.y the copy within a slab of Sc
// copies.  Lane (f, s) of the slab that starts after copy b0 works on copy b = b0 + s + 1:
//   1. it copies column f of the resident y and e^2 ([N][F]) into column f of its copy of the slab ([Sc][N][F]),
//   2. shuffles that column in place with the swap loop of k_dfq_shuffle (diff_perm_kernels.h), drawn from
//      SeqStream(Stream(seed, b, TAG_DIFF_PERM, f, 0)): copy b is replica b of mmg_diff_perm_*,
//   3. runs lrt_fit (diff_lrt_kernels.h) for model 0, then model 1, on it,
//   4. writes T = 2 (l_1 - l_0) and status0 | status1 << 4 to row b - 1 of the [B][F] arrays.
// The column lives in the slab and not in a private array, so N = 512 does not go to scratch; i and j stay wave-uniform, so X and the
// classes stay scalar loads as in k_lrt.  Every per-lane vector of lrt_fit is an SoA slot of the slab's workspace [Sc][W'][F]:
// sigma^2, the candidate and the step (ncmax slots each), then, for PM == 0, the triangle (pm (pm + 1) / 2) and theta (pm).  Both
// models use the same slots, one after the other; only T and the status survive.  Every sum runs in lrt_fit's order, no atomics.
//
// k_lrt_perm_count: one lane per feature walks its B statistics (row b of [B][F]: a wave reads consecutive words).
#pragma once
#include "diff_lrt_kernels.h"

namespace mmg {

// the workspace slots of one copy and feature
MMG_HD uint64_t lrt_perm_wslots(uint32_t ncmax, uint32_t pm)
{
    return 3ull * ncmax + (pm <= (uint32_t)LRT_PSMALL ? 0ull : (uint64_t)pm * (pm + 1) / 2 + pm);
}

template <int PM>
__global__ void __launch_bounds__(LRT_BLOCK)
k_lrt_perm(LrtParams q, uint32_t wslots, uint32_t b0, uint64_t seed, const double *__restrict__ X0, const double *__restrict__ X1,
           const int *__restrict__ cls, const double *__restrict__ y, const double *__restrict__ esq, double *__restrict__ slab_y,
           double *__restrict__ slab_e, double *__restrict__ ws, double *__restrict__ T, uint8_t *__restrict__ status)
{
    const int f = (int)(blockIdx.x * LRT_BLOCK + threadIdx.x);
    if (f >= q.F) return;
    const size_t F = (size_t)q.F, N = (size_t)q.N, s = blockIdx.y;
    const uint32_t b = b0 + (uint32_t)s + 1;
    double *yb = slab_y + s * N * F + (size_t)f, *eb = slab_e + s * N * F + (size_t)f;
    for (size_t i = 0; i < N; ++i) {
        yb[i * F] = y[i * F + (size_t)f];
        eb[i * F] = esq[i * F + (size_t)f];
    }
    SeqStream u(Stream(seed, b, TAG_DIFF_PERM, (uint64_t)f, 0));
    for (size_t j = N - 1; j > 0; --j) {
        size_t k = (size_t)(u.next() * (double)(j + 1));
        if (k > j) k = j;
        const double ty = yb[j * F], te = eb[j * F];
        yb[j * F] = yb[k * F]; eb[j * F] = eb[k * F];
        yb[k * F] = ty; eb[k * F] = te;
    }
    const int pm = q.p[0] > q.p[1] ? q.p[0] : q.p[1];
    double *w = ws + s * (size_t)wslots * F + (size_t)f;
    double *sig = w, *cand = w + (size_t)q.ncmax * F, *step = w + (size_t)2 * q.ncmax * F;
    const double nan = __builtin_nan("");
    double l0 = nan, l1 = nan;
    uint32_t st0 = 0, st1 = 0;
    for (int mi = 0; mi < 2; ++mi) {
        LrtStore<PM> S;
        S.F = F;
        S.ga = w + (size_t)3 * q.ncmax * F;
        S.gt = S.ga + (size_t)(pm * (pm + 1) / 2) * F;
        double l = nan;
        uint32_t it = 0;
        uint32_t st = lrt_fit<PM>(S, q.N, q.p[mi], q.nc[mi], F, q.max_iters, mi ? X1 : X0, cls + mi * q.N, yb, eb, sig, cand, step, &l, &it);
        // (as k_lrt reports a fit: status 2 stands alone and its l is NaN)
        if (st & LRT_ST_SINGULAR) { l = nan; st = (uint32_t)LRT_ST_SINGULAR; }
        if (mi) { l1 = l; st1 = st; } else { l0 = l; st0 = st; }
    }
    const size_t o = (size_t)(b - 1) * F + (size_t)f;
    T[o] = 2.0 * (l1 - l0);
    status[o] = (uint8_t)(st0 | st1 << 4);
}

// ll: the observed [2][F]; T: [B][F].  obs[f] = 2 (l_1 - l_0) as the host forms the observed statistic, perm_ge, perm_n, perm_p as
// include/mmgibbs.h defines them.
__global__ void __launch_bounds__(LRT_BLOCK)
k_lrt_perm_count(int F, uint32_t B, const double *__restrict__ ll, const double *__restrict__ T, double *__restrict__ obs,
                 uint64_t *__restrict__ perm_ge, uint64_t *__restrict__ perm_n, double *__restrict__ perm_p)
{
    const int f = (int)(blockIdx.x * LRT_BLOCK + threadIdx.x);
    if (f >= F) return;
    const double t0 = 2.0 * (ll[(size_t)F + f] - ll[f]);
    uint64_t ge = 0, n = 0;
    for (uint32_t b = 0; b < B; ++b) {
        const double t = T[(size_t)b * (size_t)F + f];
        if (t == t) ++n;
        if (t >= t0) ++ge;      // (false when either is NaN; -0.0 >= 0.0)
    }
    obs[f] = t0;
    perm_ge[f] = ge;
    perm_n[f] = n;
    perm_p[f] = t0 == t0 ? (double)(1 + ge) / (double)(1 + n) : __builtin_nan("");
}

} // namespace mmg
