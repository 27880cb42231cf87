// lrt_stats.hpp -- the statistics mmdiff -lrt derives on the host from the device's log likelihoods: the
// chi-squared upper tail as the regularised upper incomplete gamma function Q(a, x), and Benjamini-Hochberg q-values.  Plain C++ on
// dlog / dexp / dlgamma of mmg_math.h (compile with the library's rounding rules, -ffp-contract=off), so tests/mmdiff_lrt_ref.py
// restates it operation for operation.  host/lrt_stats_test.cpp drives it on a file; tests/test_lrt_stats.py compares with scipy.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>
#include "../mmg_math.h"

namespace lrt {

constexpr int GAMMA_ITMAX = 100000;       // both loops below end by their own test long before (a <= 20.5 here: df <= 41)
constexpr double GAMMA_EPS = 1e-16;
constexpr double GAMMA_FPMIN = 1e-300;

// Q(a, x) = Gamma(a, x) / Gamma(a), a > 0, x >= 0: the series of P below a + 1 (Q = 1 - P, P < about 0.6 there), the continued
// fraction of Q (modified Lentz) above.  NaN outside the domain.
inline double gamma_q(double a, double x)
{
    if (!(a > 0.0) || !(x >= 0.0) || !(a < __builtin_huge_val())) return __builtin_nan("");
    if (x == 0.0) return 1.0;
    if (x == __builtin_huge_val()) return 0.0;
    const double pre = mmg::dexp((-x + a * mmg::dlog(x)) - mmg::dlgamma(a));
    if (x < a + 1.0) {
        double ap = a, del = 1.0 / a, sum = del;
        for (int n = 0; n < GAMMA_ITMAX; ++n) {
            ap = ap + 1.0;
            del = del * x / ap;
            sum = sum + del;
            if (mmg::dabs(del) < mmg::dabs(sum) * GAMMA_EPS) break;
        }
        return 1.0 - sum * pre;
    }
    double b = (x + 1.0) - a, c = 1.0 / GAMMA_FPMIN, d = 1.0 / b, h = d;
    for (int i = 1; i <= GAMMA_ITMAX; ++i) {
        const double an = -(double)i * ((double)i - a);
        b = b + 2.0;
        d = an * d + b;
        if (mmg::dabs(d) < GAMMA_FPMIN) d = GAMMA_FPMIN;
        c = b + an / c;
        if (mmg::dabs(c) < GAMMA_FPMIN) c = GAMMA_FPMIN;
        d = 1.0 / d;
        const double del = d * c;
        h = h * del;
        if (mmg::dabs(del - 1.0) < GAMMA_EPS) break;
    }
    return pre * h;
}

// the upper tail of chi-squared with df degrees of freedom at max(stat, 0); NaN for df <= 0 or a NaN stat
inline double chi2_sf(int32_t df, double stat)
{
    if (df <= 0 || stat != stat) return __builtin_nan("");
    return gamma_q(0.5 * (double)df, 0.5 * (stat > 0.0 ? stat : 0.0));
}

// Benjamini-Hochberg over the p that are not NaN (q = NaN for the others): ascending p, ties in input order; from the largest p
// down, q = min(q of the next larger p, p m / rank).
inline void bh_qvalues(size_t n, const double *p, double *q)
{
    std::vector<size_t> idx;
    idx.reserve(n);
    for (size_t i = 0; i < n; ++i) {
        if (p[i] == p[i]) idx.push_back(i);
        else q[i] = __builtin_nan("");
    }
    std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return p[a] < p[b]; });
    const double m = (double)idx.size();
    double run = 1.0;
    for (size_t r = idx.size(); r-- > 0;) {
        const double v = p[idx[r]] * m / (double)(r + 1);
        if (v < run) run = v;
        q[idx[r]] = run;
    }
}

} // namespace lrt
