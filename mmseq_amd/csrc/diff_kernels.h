// diff_kernels.h -- mmdiff's Bayesian model selection (src/bms.cpp, driven as src/mmdiff.cpp:744-866 drives it) on the device.
//
// One lane per feature: a lane runs every update of its feature for a run of iterations, in the reference's order (alpha, beta,
// eta, lambda, sigma^2 by random walk, rho -- each for model 0 then model 1 -- and, outside burn-in, gamma).  Features never
// interact, so a launch covers many iterations; the host drives the phases (burn-in, pseudopriors, tuning batches, sampling).
// The state is SoA in global memory, slot j of feature f at st[j * F + f]: adjacent lanes touch adjacent words.
//
// Randomness: Stream(seed, chain, TAG_DIFF, feature, it), `it` one running iteration index over burn-in, tuning and sampling; the
// block counter runs on through the updates of the iteration.  The chain is 0 except in the handles of mmg_diff_chains_* and mmg_diff_perm_*.  Every sum runs in a fixed order, no floating-point atomics:
// reruns are bit-identical and tests/mmdiff_ref.py restates every operation in numpy.
#pragma once
#include "mmg_math.h"

namespace mmg {

// size caps (checked by the host, recorded in DESIGN.md section 10)
constexpr int DF_KMAX = 8;     // columns of M (covariates)
constexpr int DF_LMAX = 16;    // columns of P0, P1
constexpr int DF_CMAX = 16;    // variance classes per model
constexpr int DF_NMAX = 512;   // samples
constexpr int DF_BATCH = 128;  // tuning batch length (src/mmdiff.cpp: batchlen)
constexpr int DF_BLOCK = 64;   // lanes (features) per block: the iteration kernels declare it, so they may use the whole VGPR file

// slot offsets of one model's state (vectors: slot + index)
struct DiffModel {
    int L, nc, Pnil;
    const double *P;   // [N][L]
    int alpha, A, Va, aS, aSS, aN;
    int rho, Q, R, rS, rlS;
    int beta, B, Vb, bS, bSS, bN;            // K each
    int eta, Fm, Ve, eS, eSS, eN;            // L each
    int lam, Dm, Si, lS, llS;                // L each
    int sig, J, Lm, sS, slS;                 // nc each
};

struct DiffParams {
    int F, N, K, Mnil, fixalpha;
    int chain;            // the chain of the stream key (in what was padding: the size stays 480); 0 but for mmg_diff_chains_* and mmg_diff_perm_*
    double d, s, v_beta;
    uint64_t seed;
    const double *M;      // [N][K]
    const int *Cl;        // [N][2] class of sample i in model m
    const double *y, *esq;  // [N][F]
    double *st;           // [nslot][F]
    int *gam, *tuned;     // [F]
    int gsum, logitp, LOsum;
    // per-lane workspace slots (SoA like the state, so no per-lane arrays in scratch): the beta update's K x K matrices and
    // K-vectors (only when M is not nil), the sigma^2 random walk's proposals and sums per class
    int wG, wLg, wLi, wV, wLv, wt, wz, wlprop, wsum;
    DiffModel m[2];
};

#define DF_S(o) p.st[(size_t)(o) * (size_t)p.F + (size_t)f]

MMG_HD double df_uniform(Stream &rs)
{
    double ua, ub;
    rs.pair(ua, ub);
    return ua;
}

MMG_HD double df_mb(const DiffParams &p, int f, const DiffModel &m, int i)
{
    if (p.Mnil) return 0.0;
    double acc = 0.0;
    for (int j = 0; j < p.K; ++j) acc += p.M[i * p.K + j] * DF_S(m.beta + j);
    return acc;
}

MMG_HD double df_pe(const DiffParams &p, int f, const DiffModel &m, int i)
{
    if (m.Pnil) return 0.0;
    double acc = 0.0;
    for (int l = 0; l < m.L; ++l) acc += m.P[i * m.L + l] * DF_S(m.eta + l);
    return acc;
}

MMG_HD double df_esq(const DiffParams &p, int f, int i) { return p.esq[(size_t)i * p.F + f]; }
MMG_HD double df_y(const DiffParams &p, int f, int i) { return p.y[(size_t)i * p.F + f]; }
MMG_HD double df_ec(const DiffParams &p, int f, const DiffModel &m, int mi, int i)
{
    return df_esq(p, f, i) + DF_S(m.sig + p.Cl[i * 2 + mi]);
}

// moment matching of a Gamma shape from the mean and the mean logarithm (src/bms.cpp set_pseudoprior_*)
MMG_HD double df_shape(double res, double res2)
{
    const double s_ = dlog(res) - res2;
    const double t = s_ - 3.0;
    return ((3.0 - s_) + dsqrt(t * t + 24.0 * s_)) / (12.0 * s_);
}

MMG_HD void df_update_alpha(const DiffParams &p, int f, int mi, bool fit, bool rec, Stream &rs)
{
    if (p.fixalpha) return;
    const DiffModel &m = p.m[mi];
    double a;
    if (fit) {
        double V = 0.0;
        for (int i = 0; i < p.N; ++i) V += 1.0 / df_ec(p, f, m, mi, i);
        V += 1.0 / 25.0;
        V = 1.0 / V;
        double sum = 0.0;
        for (int i = 0; i < p.N; ++i) sum += ((df_y(p, f, i) - df_mb(p, f, m, i)) - df_pe(p, f, m, i)) / df_ec(p, f, m, mi, i);
        a = normal(rs) * dsqrt(V) + V * sum;
    } else {
        a = normal(rs) * dsqrt(DF_S(m.Va)) + DF_S(m.A);
    }
    DF_S(m.alpha) = a;
    if (rec && fit) {
        DF_S(m.aS) += a;
        DF_S(m.aSS) += a * a;
        DF_S(m.aN) += 1.0;
    }
}

MMG_HD void df_update_beta(const DiffParams &p, int f, int mi, bool fit, bool rec, Stream &rs)
{
    if (p.Mnil) return;
    const DiffModel &m = p.m[mi];
    const int K = p.K;
    if (fit) {
#define G(i) DF_S(p.wG + (i))
#define Lg(i) DF_S(p.wLg + (i))
#define Li(i) DF_S(p.wLi + (i))
#define V(i) DF_S(p.wV + (i))
#define Lv(i) DF_S(p.wLv + (i))
#define t(i) DF_S(p.wt + (i))
#define z(i) DF_S(p.wz + (i))
        const double alpha = DF_S(m.alpha);
        for (int a = 0; a < K; ++a) {
            t(a) = 0.0;
            for (int b = 0; b < K; ++b) G(a * K + b) = 0.0;
        }
        // G = M' W M + I / v_beta and t = M' W r, W = diag(1 / (e^2 + sigma^2)), r = y - alpha - P eta; sums over samples in order
        for (int i = 0; i < p.N; ++i) {
            const double w = 1.0 / df_ec(p, f, m, mi, i);
            const double r = (df_y(p, f, i) - alpha) - df_pe(p, f, m, i);
            for (int a = 0; a < K; ++a) {
                const double mw = p.M[i * K + a] * w;
                for (int b = 0; b < K; ++b) G(a * K + b) += mw * p.M[i * K + b];
                t(a) += mw * r;
            }
        }
        for (int a = 0; a < K; ++a) G(a * K + a) += 1.0 / p.v_beta;
        // V = G^-1 through the Cholesky factor of G and its triangular inverse, then V's own Cholesky factor
        for (int j = 0; j < K; ++j) {
            double sd = G(j * K + j);
            for (int k = 0; k < j; ++k) sd -= Lg(j * K + k) * Lg(j * K + k);
            Lg(j * K + j) = dsqrt(sd);
            for (int i = j + 1; i < K; ++i) {
                double u = G(i * K + j);
                for (int k = 0; k < j; ++k) u -= Lg(i * K + k) * Lg(j * K + k);
                Lg(i * K + j) = u / Lg(j * K + j);
            }
        }
        for (int j = 0; j < K; ++j) {
            Li(j * K + j) = 1.0 / Lg(j * K + j);
            for (int i = j + 1; i < K; ++i) {
                double u = 0.0;
                for (int k = j; k < i; ++k) u -= Lg(i * K + k) * Li(k * K + j);
                Li(i * K + j) = u / Lg(i * K + i);
            }
        }
        for (int a = 0; a < K; ++a)
            for (int b = 0; b < K; ++b) {
                double u = 0.0;
                for (int k = (a > b ? a : b); k < K; ++k) u += Li(k * K + a) * Li(k * K + b);
                V(a * K + b) = u;
            }
        for (int j = 0; j < K; ++j) {
            double sd = V(j * K + j);
            for (int k = 0; k < j; ++k) sd -= Lv(j * K + k) * Lv(j * K + k);
            Lv(j * K + j) = dsqrt(sd);
            for (int i = j + 1; i < K; ++i) {
                double u = V(i * K + j);
                for (int k = 0; k < j; ++k) u -= Lv(i * K + k) * Lv(j * K + k);
                Lv(i * K + j) = u / Lv(j * K + j);
            }
        }
        for (int a = 0; a < K; ++a) z(a) = normal(rs);
        for (int a = 0; a < K; ++a) {
            double c = 0.0;
            for (int b = 0; b <= a; ++b) c += Lv(a * K + b) * z(b);
            double mu = 0.0;
            for (int b = 0; b < K; ++b) mu += V(a * K + b) * t(b);
            DF_S(m.beta + a) = c + mu;
        }
    } else {
        for (int a = 0; a < K; ++a) DF_S(m.beta + a) = normal(rs) * dsqrt(DF_S(m.Vb + a)) + DF_S(m.B + a);
    }
#undef G
#undef Lg
#undef Li
#undef V
#undef Lv
#undef t
#undef z
    if (rec) {
        for (int a = 0; a < K; ++a) {
            const double b = DF_S(m.beta + a);
            DF_S(m.bS + a) += b;
            DF_S(m.bSS + a) += b * b;
            DF_S(m.bN + a) += 1.0;
        }
    }
}

MMG_HD void df_update_eta(const DiffParams &p, int f, int mi, bool fit, bool rec, Stream &rs)
{
    const DiffModel &m = p.m[mi];
    if (m.Pnil) return;
    if (fit) {
        const double alpha = DF_S(m.alpha);
        for (int l = 0; l < m.L; ++l) {
            double V = 1.0 / DF_S(m.lam + l);
            for (int i = 0; i < p.N; ++i) {
                const double pil = m.P[i * m.L + l];
                V += (pil * pil) / df_ec(p, f, m, mi, i);
            }
            V = 1.0 / V;
            const double el = DF_S(m.eta + l);
            double sum = 0.0;
            for (int i = 0; i < p.N; ++i) {
                const double pil = m.P[i * m.L + l];
                const double pev = df_pe(p, f, m, i) - pil * el;
                sum += (pil * (((df_y(p, f, i) - df_mb(p, f, m, i)) - alpha) - pev)) / df_ec(p, f, m, mi, i);
            }
            DF_S(m.eta + l) = normal(rs) * dsqrt(V) + V * sum;
        }
    } else {
        for (int l = 0; l < m.L; ++l) DF_S(m.eta + l) = normal(rs) * dsqrt(DF_S(m.Ve + l)) + DF_S(m.Fm + l);
    }
    if (rec && fit) {
        for (int l = 0; l < m.L; ++l) {
            const double e = DF_S(m.eta + l);
            DF_S(m.eS + l) += e;
            DF_S(m.eSS + l) += e * e;
            DF_S(m.eN + l) += 1.0;
        }
    }
}

MMG_HD void df_update_lambda(const DiffParams &p, int f, int mi, bool fit, bool rec, Stream &rs)
{
    const DiffModel &m = p.m[mi];
    if (m.Pnil) return;
    for (int l = 0; l < m.L; ++l) {
        double lam;
        if (fit) {
            const double e = DF_S(m.eta + l);
            lam = 1.0 / (gamma_unit(rs, p.d + 0.5) * (1.0 / (p.s + (0.5 * e) * e)));
        } else {
            lam = 1.0 / (gamma_unit(rs, DF_S(m.Dm + l)) * DF_S(m.Si + l));
        }
        DF_S(m.lam + l) = lam;
    }
    if (rec) {
        for (int l = 0; l < m.L; ++l) {
            const double tmp = 1.0 / DF_S(m.lam + l);
            DF_S(m.lS + l) += tmp;
            DF_S(m.llS + l) += dlog(tmp);
        }
    }
}

MMG_HD void df_update_sigmasq(const DiffParams &p, int f, int mi, bool fit, bool rec, Stream &rs)
{
    const DiffModel &m = p.m[mi];
    const double k = 4.0, g = 2.0;
    if (fit) {
        // log sigma^2 and the proposal exp(log proposal) are recomputed where needed (the same values); the log proposals and
        // the per-class sums live in the workspace slots
        const double alpha = DF_S(m.alpha), rho = DF_S(m.rho);
        for (int c = 0; c < m.nc; ++c) {
            DF_S(p.wlprop + c) = normal(rs) * g + dlog(DF_S(m.sig + c));
            DF_S(p.wsum + c) = 0.0;
        }
        for (int i = 0; i < p.N; ++i) {
            const int c = p.Cl[i * 2 + mi];
            const double tmp = ((df_y(p, f, i) - alpha) - df_mb(p, f, m, i)) - df_pe(p, f, m, i);
            const double es = df_esq(p, f, i), sc = DF_S(m.sig + c), prop = dexp(DF_S(p.wlprop + c));
            DF_S(p.wsum + c) += (dlog(es + prop) - dlog(es + sc)) + (tmp * tmp) * ((1.0 / (es + prop)) - (1.0 / (es + sc)));
        }
        for (int c = 0; c < m.nc; ++c) {
            const double sc = DF_S(m.sig + c), lprop = DF_S(p.wlprop + c), prop = dexp(lprop);
            const double logar = ((-0.5 * DF_S(p.wsum + c)) - ((0.5 * k) * rho) * ((1.0 / prop) - (1.0 / sc))) - (0.5 * k) * (lprop - dlog(sc));
            if (logar > dlog(df_uniform(rs))) DF_S(m.sig + c) = prop;
        }
    } else {
        for (int c = 0; c < m.nc; ++c) DF_S(m.sig + c) = 1.0 / (gamma_unit(rs, DF_S(m.J + c)) * (1.0 / DF_S(m.Lm + c)));
    }
    if (rec) {
        for (int c = 0; c < m.nc; ++c) {
            const double tmp = 1.0 / DF_S(m.sig + c);
            DF_S(m.sS + c) += tmp;
            DF_S(m.slS + c) += dlog(tmp);
        }
    }
}

MMG_HD void df_update_rho(const DiffParams &p, int f, int mi, bool fit, bool rec, Stream &rs)
{
    const DiffModel &m = p.m[mi];
    const double k = 4.0, q = 1.2, r = 2.0;
    double rho;
    if (fit) {
        double sum = 0.0;
        for (int c = 0; c < m.nc; ++c) sum += 1.0 / DF_S(m.sig + c);
        rho = gamma_unit(rs, ((double)m.nc * 0.5) * k + q) * (1.0 / (r + (0.5 * k) * sum));
    } else {
        rho = gamma_unit(rs, DF_S(m.Q)) * (1.0 / DF_S(m.R));
    }
    DF_S(m.rho) = rho;
    if (rec) {
        DF_S(m.rS) += rho;
        DF_S(m.rlS) += dlog(rho);
    }
}

MMG_HD double df_log_posterior(const DiffParams &p, int f, int mi)
{
    const DiffModel &m = p.m[mi];
    const double k = 4.0, q = 1.2, r = 2.0;
    const double alpha = DF_S(m.alpha), rho = DF_S(m.rho);
    double sum = 0.0, sum2 = 0.0;
    for (int i = 0; i < p.N; ++i) {
        const double e = df_ec(p, f, m, mi, i);
        sum += dlog(e);
        const double dd = ((df_y(p, f, i) - alpha) - df_mb(p, f, m, i)) - df_pe(p, f, m, i);
        sum2 += (dd * dd) / e;
    }
    double res = 0.0;
    res += (-0.5 * sum) - 0.5 * sum2;
    res += ((-0.5 * alpha) * alpha) / 25.0;
    if (!p.Mnil) {
        double ss = 0.0;
        for (int j = 0; j < p.K; ++j) ss += DF_S(m.beta + j) * DF_S(m.beta + j);
        res += (-0.5 / p.v_beta) * ss;
    }
    sum = 0.0;
    if (!m.Pnil) {
        const double lgd = dlgamma(p.d), lss = dlog(p.s);
        for (int l = 0; l < m.L; ++l) {
            const double e = DF_S(m.eta + l), lam = DF_S(m.lam + l);
            sum += (((((-0.5 * e) * e) / lam - (1.5 + p.d) * dlog(lam)) + p.d * lss) - lgd) - p.s / lam;
        }
    }
    for (int c = 0; c < m.nc; ++c) {
        const double sg = DF_S(m.sig + c);
        sum += ((k / 2.0) * dlog(rho) - (k * rho) / (2.0 * sg)) - (1.0 + k / 2.0) * dlog(sg);
    }
    res += sum;
    res += ((k * (double)m.nc) / 2.0) * dlog(k / 2.0) - (double)m.nc * dlgamma(k / 2.0);
    res += (q - 1.0) * dlog(rho) - r * rho;
    return res;
}

MMG_HD double df_log_pseudo(const DiffParams &p, int f, int mi)
{
    const DiffModel &m = p.m[mi];
    double res = 0.0, sum = 0.0;
    if (!p.fixalpha) {
        const double da = DF_S(m.alpha) - DF_S(m.A), va = DF_S(m.Va);
        res += (-0.5 * dlog(va)) - (0.5 * (da * da)) / va;
    }
    if (!p.Mnil) {
        for (int l = 0; l < p.K; ++l) {
            const double db = DF_S(m.beta + l) - DF_S(m.B + l), vb = DF_S(m.Vb + l);
            res += (-0.5 * dlog(vb)) - (0.5 * (db * db)) / vb;
        }
    }
    sum = 0.0;
    if (!m.Pnil) {
        for (int l = 0; l < m.L; ++l) {
            const double de = DF_S(m.eta + l) - DF_S(m.Fm + l), ve = DF_S(m.Ve + l);
            const double D = DF_S(m.Dm + l), Si = DF_S(m.Si + l), lam = DF_S(m.lam + l);
            sum += (-0.5 * dlog(ve)) - (0.5 * (de * de)) / ve;
            sum += D * dlog(1.0 / Si) - (D + 1.0) * dlog(lam);
            sum += (-dlgamma(D)) - 1.0 / (Si * lam);
        }
    }
    for (int c = 0; c < m.nc; ++c) {
        const double J = DF_S(m.J + c), L = DF_S(m.Lm + c), sg = DF_S(m.sig + c);
        sum += J * dlog(L) - dlgamma(J);
        sum += (-J - 1.0) * dlog(sg) - L / sg;
    }
    res += sum;
    const double Q = DF_S(m.Q), R = DF_S(m.R), rho = DF_S(m.rho);
    res += Q * dlog(R) - dlgamma(Q);
    res += (Q - 1.0) * dlog(rho) - R * rho;
    return res;
}

// one iteration of one feature (src/mmdiff.cpp:786-846): fit = burn-in, or the model gamma currently selects
MMG_HD void df_iteration(const DiffParams &p, int f, uint32_t it, bool inburnin, bool rec)
{
    Stream rs(p.seed, (uint32_t)p.chain, TAG_DIFF, (uint64_t)f, it);
    const int g = p.gam[f];
    for (int mi = 0; mi < 2; ++mi) df_update_alpha(p, f, mi, inburnin || g == mi, rec, rs);
    for (int mi = 0; mi < 2; ++mi) df_update_beta(p, f, mi, inburnin || g == mi, rec, rs);
    for (int mi = 0; mi < 2; ++mi) df_update_eta(p, f, mi, inburnin || g == mi, rec, rs);
    for (int mi = 0; mi < 2; ++mi) df_update_lambda(p, f, mi, inburnin || g == mi, rec, rs);
    for (int mi = 0; mi < 2; ++mi) df_update_sigmasq(p, f, mi, inburnin || g == mi, rec, rs);
    for (int mi = 0; mi < 2; ++mi) df_update_rho(p, f, mi, inburnin || g == mi, rec, rs);
    if (!inburnin) {
        const double LO = (((df_log_posterior(p, f, 1) + df_log_pseudo(p, f, 0)) - df_log_posterior(p, f, 0)) - df_log_pseudo(p, f, 1))
                          + DF_S(p.logitp);
        const double u = df_uniform(rs);
        const double x = dlog(u) - dlog(1.0 - u);
        DF_S(p.LOsum) += LO;
        const int ng = x < LO ? 1 : 0;
        p.gam[f] = ng;
        if (rec) DF_S(p.gsum) += (double)ng;
    }
}

// the BMS constructor's starting values
MMG_HD void df_init(const DiffParams &p, int f, double logitp0)
{
    for (int mi = 0; mi < 2; ++mi) {
        const DiffModel &m = p.m[mi];
        DF_S(m.alpha) = 0.0; DF_S(m.A) = 0.0; DF_S(m.Va) = 25.0; DF_S(m.aS) = 0.0; DF_S(m.aSS) = 0.0; DF_S(m.aN) = 0.0;
        DF_S(m.rho) = 0.2; DF_S(m.Q) = 2.0; DF_S(m.R) = 10.0; DF_S(m.rS) = 0.0; DF_S(m.rlS) = 0.0;
        for (int a = 0; a < p.K; ++a) {
            DF_S(m.beta + a) = 0.0; DF_S(m.B + a) = 0.0; DF_S(m.Vb + a) = 1.0; DF_S(m.bS + a) = 0.0; DF_S(m.bSS + a) = 0.0; DF_S(m.bN + a) = 0.0;
        }
        for (int l = 0; l < m.L; ++l) {
            DF_S(m.eta + l) = 0.0; DF_S(m.Fm + l) = 0.0; DF_S(m.Ve + l) = 1.0; DF_S(m.eS + l) = 0.0; DF_S(m.eSS + l) = 0.0; DF_S(m.eN + l) = 0.0;
            DF_S(m.lam + l) = p.s / (p.d - 1.0); DF_S(m.Dm + l) = 0.0; DF_S(m.Si + l) = 1.0 / p.s; DF_S(m.lS + l) = 0.0; DF_S(m.llS + l) = 0.0;
        }
        for (int c = 0; c < m.nc; ++c) {
            DF_S(m.sig + c) = 0.5; DF_S(m.J + c) = 2.0; DF_S(m.Lm + c) = 0.5; DF_S(m.sS + c) = 0.0; DF_S(m.slS + c) = 0.0;
        }
    }
    DF_S(p.gsum) = 0.0; DF_S(p.logitp) = logitp0; DF_S(p.LOsum) = 0.0;
    p.gam[f] = 0;
    p.tuned[f] = 0;
}

__global__ void k_df_init(DiffParams p, double logitp0)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < p.F) df_init(p, f, logitp0);
}

// n burn-in (mode 0) or sampling (mode 2) iterations t0 .. t0 + n - 1, stream index it0 + (t - t0); burn-in records from t = rec_from
__global__ void __launch_bounds__(DF_BLOCK) k_df_run(DiffParams p, uint32_t it0, int t0, int n, int mode, int rec_from)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= p.F) return;
    for (int j = 0; j < n; ++j) {
        const int t = t0 + j;
        df_iteration(p, f, it0 + (uint32_t)j, mode == 0, mode == 2 || t >= rec_from);
    }
}

// ---- traces (mmg_diff_trace_open): thinned rows of the parameters recorded by the run kernel itself ---------------------------------
// The parameters of BMS::initialise_streams in its order (alpha, beta, eta, lambda, sigma^2, rho of model 0 then 1 within each kind;
// gamma last, in sampling only): slot[s] is the state slot of traced parameter s, -1 for gamma.  A row is the state after an iteration
// whose phase index tt (the burn-in's t, or the sampling iteration counted from the first one) is a multiple of `every`; the rows of
// a launch start at row0 = ceil(tt0 / every) and go to tr[((row - row0) * P + s) * F + f]: a wave stores adjacent words, like every
// other state access.  cap is the number of rows the buffer holds; the launcher sizes its launches to it, and the kernel never
// stores beyond it.
constexpr int DF_TRACE_PMAX = 2 + 2 * DF_KMAX + 4 * DF_LMAX + 2 * DF_CMAX + 2 + 1;

struct DiffTrace {
    double *tr;       // [cap][P][F]
    int P, every, tt0, cap;
    int slot[DF_TRACE_PMAX];
};

// rows with index in [ceil(a / every), ceil(b / every)): those of the iterations a .. b - 1 (t < 2^31 and every <= DF_TRACE_EVERY_MAX, so
// the sum stays inside int)
constexpr uint32_t DF_TRACE_EVERY_MAX = 1u << 30;
MMG_HD int df_trace_row_ceil(int t, int every) { return (t + every - 1) / every; }

// rows a trace buffer holds: those of a full launch of `chunk` iterations at the denser thinning, cut to what `limit` bytes hold (one
// row at least) and to `max_rows` if that is not 0
MMG_HD uint32_t df_trace_cap(uint32_t P, uint32_t F, uint32_t every_min, uint32_t chunk, uint64_t limit, uint32_t max_rows)
{
    uint64_t cap = ((uint64_t)chunk + every_min - 1) / every_min;
    const uint64_t fit = limit / ((uint64_t)P * F * 8);
    if (cap > fit) cap = fit ? fit : 1;
    if (max_rows && cap > max_rows) cap = max_rows;
    return (uint32_t)cap;
}

// the launch that starts at phase index tt with `left` iterations to go: it ends after `chunk` iterations, or before the iteration of
// the row after the buffer's last.  Returns its length (>= 1 for left >= 1); *first_row = ceil(tt / every), *rows <= cap.
MMG_HD uint32_t df_trace_plan(uint32_t tt, uint32_t left, uint32_t every, uint32_t cap, uint32_t chunk, uint32_t *first_row, uint32_t *rows)
{
    const uint64_t r0 = ((uint64_t)tt + every - 1) / every;
    const uint64_t room = (r0 + cap) * every - tt;
    uint64_t n = left < chunk ? left : chunk;
    if (n > room) n = room;
    *first_row = (uint32_t)r0;
    *rows = (uint32_t)(((uint64_t)tt + n + every - 1) / every - r0);
    return (uint32_t)n;
}

// k_df_run recording rows: the same df_iteration calls in the same order, and reads of the state after them -- it draws nothing.
// The descriptor is read from device memory where a row is stored, not held in registers across the iterations: as kernel arguments
// its fields cost two more VGPRs (169) and with them the third wave per SIMD.
__global__ void __launch_bounds__(DF_BLOCK) k_df_run_traced(DiffParams p, uint32_t it0, int t0, int n, int mode, int rec_from, const DiffTrace *q)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= p.F) return;
    for (int j = 0; j < n; ++j) {
        const int t = t0 + j;
        df_iteration(p, f, it0 + (uint32_t)j, mode == 0, mode == 2 || t >= rec_from);
        const int tt = q->tt0 + j, every = q->every;
        if (tt % every) continue;
        const int row = tt / every - df_trace_row_ceil(q->tt0, every);
        if (row >= q->cap) continue;
        const int P = q->P;
        double *dst = q->tr + (size_t)row * (size_t)P * (size_t)p.F + (size_t)f;
        for (int s = 0; s < P; ++s) {
            const int o = q->slot[s];
            dst[(size_t)s * (size_t)p.F] = o >= 0 ? DF_S(o) : (double)p.gam[f];
        }
    }
}

// tuning batch b (src/mmdiff.cpp:781-790, BMS::tunep): iterations 128 b .. 128 b + 127.  A feature tuned before the batch is frozen;
// from the second batch on, its first iteration tunes logit p' from the mean log odds of the previous batch.  untuned counts the
// features still untuned after that step (an integer atomic: the count is order-free).
// returns 1 if the feature is still untuned after the batch's tuning step
MMG_HD int df_tune(const DiffParams &p, int f, uint32_t it0, int b)
{
    const double LOGIT07 = 0.8472979;
    const int t0 = b * DF_BATCH;
    int n = DF_BATCH;
    if (b > 0) {
        if (p.tuned[f]) return 0;
        const double mp = DF_S(p.LOsum) / (double)DF_BATCH;
        if (mp > -LOGIT07 && mp < LOGIT07) {
            p.tuned[f] = 1;
            n = 1;   // tuned now: this iteration still runs, the rest of the batch is frozen
        } else {
            const double step = 1.0 / dsqrt((double)(2 + t0 / DF_BATCH));
            if (mp > 0) DF_S(p.logitp) -= step;
            else DF_S(p.logitp) += step;
            DF_S(p.LOsum) = 0.0;
        }
    }
    for (int j = 0; j < n; ++j) df_iteration(p, f, it0 + (uint32_t)j, false, false);
    return n == DF_BATCH ? 1 : 0;
}

__global__ void __launch_bounds__(DF_BLOCK) k_df_tune(DiffParams p, uint32_t it0, int b, int *untuned)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= p.F) return;
    if (df_tune(p, f, it0, b)) atomicAdd(untuned, 1);
}

// pseudopriors from the recorded burn-in sums (BMS::set_pseudoprior_*), then BMS::reset()
MMG_HD void df_pseudo(const DiffParams &p, int f, double runlen)
{
    const double n = runlen;
    for (int mi = 0; mi < 2; ++mi) {
        const DiffModel &m = p.m[mi];
        if (!p.fixalpha) {
            const double S = DF_S(m.aS), SS = DF_S(m.aSS);
            DF_S(m.A) = S / n;
            DF_S(m.Va) = (SS - (S * S) / n) / (n - 1.0);
        }
        if (!p.Mnil)
            for (int a = 0; a < p.K; ++a) {
                const double S = DF_S(m.bS + a), SS = DF_S(m.bSS + a);
                DF_S(m.B + a) = S / n;
                DF_S(m.Vb + a) = (SS - (S * S) / n) / (n - 1.0);
            }
        if (!m.Pnil)
            for (int l = 0; l < m.L; ++l) {
                const double S = DF_S(m.eS + l), SS = DF_S(m.eSS + l);
                DF_S(m.Fm + l) = S / n;
                DF_S(m.Ve + l) = (SS - (S * S) / n) / (n - 1.0);
                const double res = DF_S(m.lS + l) / n, res2 = DF_S(m.llS + l) / n;
                const double D = df_shape(res, res2);
                DF_S(m.Dm + l) = D;
                DF_S(m.Si + l) = res / D;
            }
        for (int c = 0; c < m.nc; ++c) {
            const double res = DF_S(m.sS + c) / n, res2 = DF_S(m.slS + c) / n;
            const double J = df_shape(res, res2);
            DF_S(m.J + c) = J;
            DF_S(m.Lm + c) = J / res;
        }
        {
            const double res = DF_S(m.rS) / n, res2 = DF_S(m.rlS) / n;
            const double Q = df_shape(res, res2);
            DF_S(m.Q) = Q;
            DF_S(m.R) = Q / res;
        }
        DF_S(m.aS) = 0.0; DF_S(m.aSS) = 0.0; DF_S(m.aN) = 0.0; DF_S(m.rS) = 0.0; DF_S(m.rlS) = 0.0;
        for (int a = 0; a < p.K; ++a) { DF_S(m.bS + a) = 0.0; DF_S(m.bSS + a) = 0.0; DF_S(m.bN + a) = 0.0; }
        for (int l = 0; l < m.L; ++l) { DF_S(m.eS + l) = 0.0; DF_S(m.eSS + l) = 0.0; DF_S(m.eN + l) = 0.0; DF_S(m.lS + l) = 0.0; DF_S(m.llS + l) = 0.0; }
        for (int c = 0; c < m.nc; ++c) { DF_S(m.sS + c) = 0.0; DF_S(m.slS + c) = 0.0; }
    }
    DF_S(p.gsum) = 0.0;
}

__global__ void k_df_pseudo(DiffParams p, double runlen)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < p.F) df_pseudo(p, f, runlen);
}

#undef DF_S

// ---- several comparisons against one model 0 in one launch (mmg_diff_poly_*) -----------------------------------------------
// ps[c] is comparison c's DiffParams: its own slot layout, state block, gam / tuned and class table; every one points at the same
// y / esq / M / P0.  blockIdx.y picks the comparison, so the parameters are read through a wave-uniform address (scalar loads, as
// the single-comparison kernels read theirs from the kernel arguments), and the grid is (blocks of F) x J.  The per-lane work is
// df_iteration / df_tune / df_pseudo / df_init unchanged, and the stream key has no comparison in it: comparison c's chain is the
// chain mmg_diff_* runs for the same inputs.
constexpr int DF_JMAX = 16;    // comparisons per handle

__global__ void k_dfp_init(const DiffParams *__restrict__ ps, double logitp0)
{
    const DiffParams &p = ps[blockIdx.y];
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < p.F) df_init(p, f, logitp0);
}

// as k_df_run; comparison c's stream index starts at off[c] + it0 (off: the iterations its own tuning took, 0 in burn-in)
__global__ void __launch_bounds__(DF_BLOCK) k_dfp_run(const DiffParams *__restrict__ ps, const uint32_t *__restrict__ off, uint32_t it0, int t0,
                                                      int n, int mode, int rec_from)
{
    const DiffParams &p = ps[blockIdx.y];
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= p.F) return;
    const uint32_t it = off[blockIdx.y] + it0;
    for (int j = 0; j < n; ++j) {
        const int t = t0 + j;
        df_iteration(p, f, it + (uint32_t)j, mode == 0, mode == 2 || t >= rec_from);
    }
}

// as k_df_tune, for the comparisons whose bit is set in `active` (the others have ended tuning: their blocks return at once).  Every
// active comparison is at batch b: all started together and an ended one never resumes.  untuned[c] counts comparison c's features.
__global__ void __launch_bounds__(DF_BLOCK) k_dfp_tune(const DiffParams *__restrict__ ps, uint32_t active, uint32_t it0, int b,
                                                       int *__restrict__ untuned)
{
    if (!((active >> blockIdx.y) & 1u)) return;
    const DiffParams &p = ps[blockIdx.y];
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= p.F) return;
    if (df_tune(p, f, it0, b)) atomicAdd(untuned + blockIdx.y, 1);
}

__global__ void k_dfp_pseudo(const DiffParams *__restrict__ ps, double runlen)
{
    const DiffParams &p = ps[blockIdx.y];
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < p.F) df_pseudo(p, f, runlen);
}

// ---- several chains of one comparison in one launch (mmg_diff_chains_*) ------------------------------------------------------
// ps[c] is chain c's DiffParams: the slot layout, y / esq / M / P0 / P1 and class table of every chain are the same; the state block,
// gam / tuned and `chain` are its own.  blockIdx.y picks the chain as it picks the comparison above, and the per-lane work is the same
// df_iteration / df_tune / df_pseudo / df_init: chain c is the chain of a single handle whose seed is seed ^ (c << 32).
// After the slots of df_layout every chain has DF_NB batch slots gb .. gb + DF_NB - 1: during sampling the lane adds its new gamma to
// slot t / blen, t the chain's sampling index and blen = (total sampling length) / DF_NB.  The sums are integers in doubles.
constexpr int DF_CHAINS_MAX = 16;   // chains per handle
constexpr int DF_NB = 16;           // batches of the sampling run (batch means for the Monte Carlo standard error)

__global__ void k_dfc_init(const DiffParams *__restrict__ ps, double logitp0, int gb)
{
    const DiffParams &p = ps[blockIdx.y];
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= p.F) return;
    df_init(p, f, logitp0);
    for (int b = 0; b < DF_NB; ++b) p.st[(size_t)(gb + b) * (size_t)p.F + (size_t)f] = 0.0;
}

// as k_dfp_run; in sampling (mode 2) t0 is the sampling index of the launch's first iteration, the same for every chain
__global__ void __launch_bounds__(DF_BLOCK) k_dfc_run(const DiffParams *__restrict__ ps, const uint32_t *__restrict__ off, uint32_t it0, int t0,
                                                      int n, int mode, int rec_from, int gb, int blen)
{
    const DiffParams &p = ps[blockIdx.y];
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= p.F) return;
    const uint32_t it = off[blockIdx.y] + it0;
    for (int j = 0; j < n; ++j) {
        const int t = t0 + j;
        df_iteration(p, f, it + (uint32_t)j, mode == 0, mode == 2 || t >= rec_from);
        if (mode == 2) p.st[(size_t)(gb + t / blen) * (size_t)p.F + (size_t)f] += (double)p.gam[f];
    }
}

// (tuning and the pseudopriors are k_dfp_tune and k_dfp_pseudo, `active` the chains still tuning)

MMG_HD double df_sigmoid(double x) { return x > 0 ? 1.0 / (1.0 + dexp(-x)) : dexp(x) / (1.0 + dexp(x)); }

// The chains' estimates pooled, one lane per feature, after T sampling iterations.  Every sum runs over the
// chains in ascending order.  out is SoA [DF_POOL_STATS + 2 Q][F], Q = 2 + 2 K + L0 + L1:
//   0 log_bf       the root b of sum_c sigmoid(b + logitp_c) = sum_c gsum_c / T by 64 halvings of [-1024, 1024]; -inf / +inf when no / every
//                  draw of any chain chose model 1
//   1 log_bf_sd    the sd (divisor n - 1, two passes) of logit(gsum_c / T) - logitp_c over the mixed chains (0 < gsum_c < T); NaN below two
//   2 log_bf_mcse  sqrt(sum_c v_c) / sum_c w_c, v_c the variance of chain c's mean gamma from its DF_NB batch means, w_c = s (1 - s) at
//                  s = sigmoid(log_bf + logitp_c); NaN when log_bf is infinite
//   3 chains_mixed
//   then for q = 0 .. Q - 1 (alpha of models 0, 1; beta [2][K]; eta [L0 + L1], the order of mmg_diff_get_results) the chains' summed
//   sums and summed counts: the host divides, as it does for a single handle.
// A chain whose logit p' is not finite (pdash 0 or 1 without tuning) makes 0 .. 2 NaN.
constexpr int DF_POOL_STATS = 4;

MMG_HD void df_pool(const DiffParams *__restrict__ ps, int C, int T, int gb, double *__restrict__ out, int f)
{
    const DiffParams &p = ps[0];
    const size_t F = (size_t)p.F;
#define DFC_S(c, o) ps[c].st[(size_t)(o) * F + (size_t)f]
    const double Td = (double)T, bl = (double)(T / DF_NB);
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    double sumG = 0.0;
    int mixed = 0;
    bool finite = true;
    for (int c = 0; c < C; ++c) {
        const double G = DFC_S(c, p.gsum), o = DFC_S(c, p.logitp);
        sumG += G;
        if (G > 0.0 && G < Td) ++mixed;
        if (!(o - o == 0.0)) finite = false;
    }
    double b = nan, sd = nan, mcse = nan;
    if (finite) {
        if (sumG == 0.0) b = -inf;
        else if (sumG == (double)C * Td) b = inf;
        else {
            const double target = sumG / Td;
            double lo = -1024.0, hi = 1024.0;
            for (int k = 0; k < 64; ++k) {
                const double mid = 0.5 * (lo + hi);
                double s = 0.0;
                for (int c = 0; c < C; ++c) s += df_sigmoid(mid + DFC_S(c, p.logitp));
                if (s - target < 0.0) lo = mid;
                else hi = mid;
            }
            b = 0.5 * (lo + hi);
        }
        if (mixed >= 2) {
            double sum = 0.0, ss = 0.0;
            for (int pass = 0; pass < 2; ++pass) {
                const double mean = sum / (double)mixed;
                for (int c = 0; c < C; ++c) {
                    const double G = DFC_S(c, p.gsum);
                    if (!(G > 0.0 && G < Td)) continue;
                    const double g = G / Td;
                    const double l = (dlog(g) - dlog(1.0 - g)) - DFC_S(c, p.logitp);
                    if (pass == 0) sum += l;
                    else ss += (l - mean) * (l - mean);
                }
            }
            sd = dsqrt(ss / (double)(mixed - 1));
        }
        if (b - b == 0.0) {
            double sv = 0.0, sw = 0.0;
            for (int c = 0; c < C; ++c) {
                const double g = DFC_S(c, p.gsum) / Td;
                double acc = 0.0;
                for (int k = 0; k < DF_NB; ++k) {
                    const double dv = DFC_S(c, gb + k) / bl - g;
                    acc += dv * dv;
                }
                sv += acc / (double)(DF_NB - 1) / (double)DF_NB;
                const double s = df_sigmoid(b + DFC_S(c, p.logitp));
                sw += s * (1.0 - s);
            }
            mcse = dsqrt(sv) / sw;
        }
    }
    out[0 * F + f] = b;
    out[1 * F + f] = sd;
    out[2 * F + f] = mcse;
    out[3 * F + f] = (double)mixed;
    int q = 0;
    auto pooled = [&](int oS, int oN) {
        double S = 0.0, N = 0.0;
        for (int c = 0; c < C; ++c) { S += DFC_S(c, oS); N += DFC_S(c, oN); }
        out[(size_t)(DF_POOL_STATS + 2 * q) * F + f] = S;
        out[(size_t)(DF_POOL_STATS + 2 * q + 1) * F + f] = N;
        ++q;
    };
    for (int mi = 0; mi < 2; ++mi) pooled(p.m[mi].aS, p.m[mi].aN);
    for (int mi = 0; mi < 2; ++mi)
        for (int k = 0; k < p.K; ++k) pooled(p.m[mi].bS + k, p.m[mi].bN + k);
    for (int mi = 0; mi < 2; ++mi)
        for (int l = 0; l < p.m[mi].L; ++l) pooled(p.m[mi].eS + l, p.m[mi].eN + l);
#undef DFC_S
}

__global__ void k_dfc_pool(const DiffParams *__restrict__ ps, int C, int T, int gb, double *__restrict__ out)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f < ps[0].F) df_pool(ps, C, T, gb, out, f);
}

} // namespace mmg
