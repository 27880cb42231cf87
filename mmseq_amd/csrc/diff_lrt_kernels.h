// diff_lrt_kernels.h -- mmdiff -lrt: the per-feature likelihood-ratio test on the device.
//
// One lane per feature, blocks of LRT_BLOCK lanes as k_df_run: a lane fits model 0, then model 1, by maximum likelihood.
//   y_i ~ N((X theta)_i, v_i),  v_i = e_i^2 + sigma^2_{C(i)},  l = -1/2 sum_i [log 2 pi + log v_i + r_i^2 / v_i],  r = y - X theta.
// For fixed sigma^2, theta is weighted least squares (Cholesky of X'WX); sigma^2 moves by projected Fisher scoring with step halving.
// Every loop is bounded by a constant below or by max_iters; a lane whose X'WX is not positive definite or whose weight is not
// finite leaves at once with status 2 and never iterates on NaN.
//
// X (intercept | M | P as the model has them, [N][p]) and the classes are the same for every lane: they are read through
// wave-uniform addresses from __restrict__ const kernel arguments, so they arrive as scalar loads.  y and e^2 are [N][F].
// Per-lane vectors whose length is not a compile-time constant (sigma^2 per class, the candidate and the step per class, and in
// the general instantiation the triangle of X'WX and theta) are SoA slots in device memory, slot j of feature f at [j * F + f], for
// the reason the beta update of diff_kernels.h gives: nothing is runtime-indexed private memory.  The instantiation PM = 4 (both
// models have p <= 4, every -de design) keeps the triangle, its factor and theta in registers.
//
// Every sum runs in a fixed order, no atomics; tests/mmdiff_lrt_ref.py restates every operation in numpy.  lrt_eval and lrt_fit are
// MMG_HD like the math they call, so a host program can run one lane.
#pragma once
#include "mmg_math.h"

namespace mmg {

// the caps and the block of diff_kernels.h (that header defines kernels, so only diff.hip includes it; diff.hip asserts the equalities)
constexpr int LRT_KMAX = 8, LRT_LMAX = 16, LRT_CMAX = 16, LRT_NMAX = 512, LRT_BLOCK = 64;

// ---- the algorithm's constants (DESIGN.md section 10.5 states them) ----
constexpr uint32_t LRT_MAX_ITERS = 200;   // scoring iterations per model when the call passes 0
constexpr int LRT_MAX_HALVINGS = 30;      // halvings of one scoring step (the full step and 30 halved ones are tried)
constexpr double LRT_TOL = 1e-12;         // stop once an accepted step raised l by no more than this (absolute)
constexpr double LRT_PIVOT_TOL = 1e-10;   // a Cholesky pivot must exceed this fraction of its diagonal entry of X'WX
constexpr double LRT_LOG2PI = 1.8378770664093453;
constexpr int LRT_PSMALL = 4;             // the register instantiation holds p <= 4
constexpr int LRT_PMAX = 1 + LRT_KMAX + LRT_LMAX;
// the start: sigma^2_c = the mean of e_i^2 over the class

enum { LRT_ST_CAP = 1, LRT_ST_SINGULAR = 2, LRT_ST_BOUNDARY = 4 };

struct LrtParams {
    int F, N;
    int p[2], nc[2];
    int ncmax;            // max(nc[0], nc[1]): the candidate and the step take ncmax slots each
    uint32_t max_iters;
};

// the triangle of X'WX (then its Cholesky factor) and the vector X'Wy (then theta): registers for PM > 0, SoA slots for PM == 0
template <int PM>
struct LrtStore {
    double a[PM ? PM * (PM + 1) / 2 : 1], t[PM ? PM : 1];
    double *ga, *gt;      // PM == 0: the lane's first word of the triangle / of theta
    size_t F;
    static constexpr int UNROLL = PM ? PM : 1;   // the column loops: fully unrolled over registers, left alone over slots
    MMG_HD double A(int k) const { if constexpr (PM > 0) return a[k]; else return ga[(size_t)k * F]; }
    MMG_HD void setA(int k, double v) { if constexpr (PM > 0) a[k] = v; else ga[(size_t)k * F] = v; }
    MMG_HD double T(int k) const { if constexpr (PM > 0) return t[k]; else return gt[(size_t)k * F]; }
    MMG_HD void setT(int k, double v) { if constexpr (PM > 0) t[k] = v; else gt[(size_t)k * F] = v; }
};

#define LRT_TRI(j, k) ((j) * ((j) + 1) / 2 + (k))
// loops over columns: a compile-time bound with a guard (registers, fully unrolled) or the run-time bound (slots)
#define LRT_UNROLL _Pragma("unroll LrtStore<PM>::UNROLL")
#define LRT_FOR(j, from, p) LRT_UNROLL for (int j = (from); j < (PM ? PM : (p)); ++j) if (!PM || j < (p))

// theta and l at the variances sig[c * F] (the lane's slots): false when a weight is not finite or X'WX is not positive definite
template <int PM>
MMG_HD bool lrt_eval(LrtStore<PM> &S, int N, int p, size_t F, const double *__restrict__ X, const int *__restrict__ cls,
                                         const double *__restrict__ y, const double *__restrict__ esq, const double *sig, double *l_out)
{
    LRT_FOR(j, 0, p) {
        S.setT(j, 0.0);
        LRT_FOR(k, 0, j + 1) S.setA(LRT_TRI(j, k), 0.0);
    }
    // (the weights are judged after the loop: with no lane leaving inside it, i stays wave-uniform and X and the classes stay scalar loads)
    bool bad = false;
    for (int i = 0; i < N; ++i) {
        const double v = esq[(size_t)i * F] + sig[(size_t)cls[i] * F];
        const double w = 1.0 / v;
        bad = bad || !(v > 0.0) || !(v < __builtin_huge_val()) || !(w < __builtin_huge_val());
        const double yi = y[(size_t)i * F];
        LRT_FOR(j, 0, p) {
            const double xw = X[i * p + j] * w;
            S.setT(j, S.T(j) + xw * yi);
            LRT_FOR(k, 0, j + 1) S.setA(LRT_TRI(j, k), S.A(LRT_TRI(j, k)) + xw * X[i * p + k]);
        }
    }
    if (bad) return false;
    // Cholesky in place, row by row
    LRT_FOR(j, 0, p) {
        LRT_FOR(k, 0, j) {
            double s = S.A(LRT_TRI(j, k));
            LRT_FOR(q, 0, k) s -= S.A(LRT_TRI(j, q)) * S.A(LRT_TRI(k, q));
            S.setA(LRT_TRI(j, k), s / S.A(LRT_TRI(k, k)));
        }
        const double ajj = S.A(LRT_TRI(j, j));
        double d = ajj;
        LRT_FOR(q, 0, j) d -= S.A(LRT_TRI(j, q)) * S.A(LRT_TRI(j, q));
        if (!(d > LRT_PIVOT_TOL * ajj)) return false;
        S.setA(LRT_TRI(j, j), dsqrt(d));
    }
    // L z = X'Wy, then L' theta = z, in place
    LRT_FOR(j, 0, p) {
        double s = S.T(j);
        LRT_FOR(k, 0, j) s -= S.A(LRT_TRI(j, k)) * S.T(k);
        S.setT(j, s / S.A(LRT_TRI(j, j)));
    }
    LRT_UNROLL for (int jj = (PM ? PM : p) - 1; jj >= 0; --jj)
        if (!PM || jj < p) {
            double s = S.T(jj);
            LRT_FOR(k, jj + 1, p) s -= S.A(LRT_TRI(k, jj)) * S.T(k);
            S.setT(jj, s / S.A(LRT_TRI(jj, jj)));
        }
    double acc = 0.0;
    for (int i = 0; i < N; ++i) {
        const double v = esq[(size_t)i * F] + sig[(size_t)cls[i] * F];
        double m = 0.0;
        LRT_FOR(j, 0, p) m += X[i * p + j] * S.T(j);
        const double r = y[(size_t)i * F] - m;
        acc += (LRT_LOG2PI + dlog(v)) + r * r / v;
    }
    *l_out = -0.5 * acc;
    return true;
}

// One model of one feature.  sig, cand, step: the lane's slots [nc].  Returns the status bits; *l_out and *it_out as documented.
template <int PM>
MMG_HD uint32_t lrt_fit(LrtStore<PM> &S, int N, int p, int nc, size_t F, uint32_t max_iters, const double *__restrict__ X,
                                            const int *__restrict__ cls, const double *__restrict__ y, const double *__restrict__ esq,
                                            double *sig, double *cand, double *step, double *l_out, uint32_t *it_out)
{
    *it_out = 0;
    for (int c = 0; c < nc; ++c) {
        double sum = 0.0, n = 0.0;
        for (int i = 0; i < N; ++i)
            if (cls[i] == c) { sum += esq[(size_t)i * F]; n += 1.0; }
        sig[(size_t)c * F] = sum / n;
    }
    double l;
    if (!lrt_eval<PM>(S, N, p, F, X, cls, y, esq, sig, &l)) return LRT_ST_SINGULAR;
    uint32_t it = 0;
    bool converged = false;
    while (it < max_iters) {
        ++it;
        // the scoring step of every class at the current theta (the halves of U_c and I_c cancel)
        bool move = false, finite = true;
        for (int c = 0; c < nc; ++c) {
            double U = 0.0, I = 0.0;
            for (int i = 0; i < N; ++i)
                if (cls[i] == c) {
                    const double v = esq[(size_t)i * F] + sig[(size_t)c * F];
                    const double w = 1.0 / v;
                    double m = 0.0;
                    LRT_FOR(j, 0, p) m += X[i * p + j] * S.T(j);
                    const double r = y[(size_t)i * F] - m;
                    const double w2 = w * w;
                    U += r * r * w2 - w;
                    I += w2;
                }
            const double dl = U / I;
            if (!(dabs(dl) < __builtin_huge_val())) finite = false;
            const double s0 = sig[(size_t)c * F], s1 = s0 + dl;
            const double sc = s1 > 0.0 ? s1 : 0.0;
            step[(size_t)c * F] = dl;
            cand[(size_t)c * F] = sc;
            if (sc != s0) move = true;
        }
        if (!finite) return LRT_ST_SINGULAR;
        if (!move) { converged = true; break; }
        double h = 1.0, lnew = l;
        bool accepted = false;
        for (int hv = 0; hv <= LRT_MAX_HALVINGS; ++hv) {
            if (hv > 0) {
                h = h * 0.5;
                for (int c = 0; c < nc; ++c) {
                    const double s1 = sig[(size_t)c * F] + h * step[(size_t)c * F];
                    cand[(size_t)c * F] = s1 > 0.0 ? s1 : 0.0;
                }
            }
            if (!lrt_eval<PM>(S, N, p, F, X, cls, y, esq, cand, &lnew)) return LRT_ST_SINGULAR;
            if (lnew > l) { accepted = true; break; }
        }
        if (!accepted) {
            // no halved step raises l: the current point stands; theta is fitted there again (the candidates overwrote it)
            if (!lrt_eval<PM>(S, N, p, F, X, cls, y, esq, sig, &l)) return LRT_ST_SINGULAR;
            converged = true;
            break;
        }
        const double gain = lnew - l;
        for (int c = 0; c < nc; ++c) sig[(size_t)c * F] = cand[(size_t)c * F];
        l = lnew;
        if (gain <= LRT_TOL) { converged = true; break; }
    }
    uint32_t st = converged ? 0u : (uint32_t)LRT_ST_CAP;
    for (int c = 0; c < nc; ++c)
        if (sig[(size_t)c * F] == 0.0) st |= LRT_ST_BOUNDARY;
    *l_out = l;
    *it_out = it;
    return st;
}

// Both models of every feature.  theta0 / theta1: [p][F]; sig0 / sig1: [nc][F]; ll, iters, status: [2][F]; ws: [2 ncmax + T][F] with
// T = pm (pm + 1) / 2 slots for the triangle when PM == 0 (pm = max p), none when PM > 0.
template <int PM>
__global__ void __launch_bounds__(LRT_BLOCK)
k_lrt(LrtParams q, const double *__restrict__ X0, const double *__restrict__ X1, const int *__restrict__ cls, const double *__restrict__ y,
      const double *__restrict__ esq, double *__restrict__ theta0, double *__restrict__ theta1, double *__restrict__ sig0,
      double *__restrict__ sig1, double *__restrict__ ll, uint32_t *__restrict__ iters, uint32_t *__restrict__ status, double *__restrict__ ws)
{
    const int f = (int)(blockIdx.x * LRT_BLOCK + threadIdx.x);
    if (f >= q.F) return;
    const size_t F = (size_t)q.F;
    const double nan = __builtin_nan("");
    for (int mi = 0; mi < 2; ++mi) {
        const int p = q.p[mi], nc = q.nc[mi];
        const double *X = mi ? X1 : X0;
        double *theta = (mi ? theta1 : theta0) + f, *sig = (mi ? sig1 : sig0) + f;
        double *cand = ws + f, *step = ws + (size_t)q.ncmax * F + f;
        LrtStore<PM> S;
        S.F = F;
        S.ga = ws + (size_t)2 * q.ncmax * F + f;
        S.gt = theta;
        double l = nan;
        uint32_t it = 0;
        const uint32_t st = lrt_fit<PM>(S, q.N, p, nc, F, q.max_iters, X, cls + mi * q.N, y + f, esq + f, sig, cand, step, &l, &it);
        if (st & LRT_ST_SINGULAR) {
            l = nan;
            for (int j = 0; j < p; ++j) theta[(size_t)j * F] = nan;
            for (int c = 0; c < nc; ++c) sig[(size_t)c * F] = nan;
        } else if (PM > 0) {
            LRT_FOR(j, 0, p) theta[(size_t)j * F] = S.T(j);
        }
        ll[(size_t)mi * F + f] = l;
        iters[(size_t)mi * F + f] = it;
        status[(size_t)mi * F + f] = (st & LRT_ST_SINGULAR) ? (uint32_t)LRT_ST_SINGULAR : st;
    }
}

} // namespace mmg
