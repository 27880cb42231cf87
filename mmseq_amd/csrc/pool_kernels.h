// pool_kernels.h -- the posterior summary of the draws of ALL chains of a series (mmg_pooled_*; DESIGN.md section 14 states the
// definitions, tests/pooled_ref.py restates them in numpy).
//
// Input as for the convergence diagnostics: series-major slabs X[series][chain][sample] of C chains x S draws, N = C S pooled draws.
// The per-chain columns of the logged draws (mean, Sokal's var / tau / rc) are NOT computed here: a slab is count * C series of
// length S to k_series_summary<., true> (post_kernels.h, unchanged), whose results this kernel combines.  What is new here are the
// order statistics of the N pooled draws (block_sort of their order_key, padded to a power of two: mmg_series.h), the
// combination rule of the log columns, and the pooled proportion summaries (per chain the three sequential sums of
// k_series_summary<., false>, then summed over the chains in ascending order).  Every sum runs in a fixed order: reruns are bit-identical.
#pragma once
#include "post_kernels.h"

namespace mmg {

struct PoolOut {
    double *a, *b, *c;   // [count]  log mode: log_mean, var, tau;  proportion mode: mean, probit_mean, probit_sd
    double *mcse2;       // [count]  log mode
    int32_t *rc;         // [count]  log mode
    double *pct;         // [count][np]  order statistics of the pooled draws (both modes)
};

// One workgroup per series at a time (workgroup b takes the series b, b + gridDim.x, ...).
//   LOG_MODE:  cm / cv / ct / crc [count][C] hold the per-chain columns (read); one lane combines them.
//   otherwise: cm / cv / ct [count][C] are scratch: lanes strided over the chains store a chain's sums of x, probit(clamp(x)) and its
//              square there (sample order, as k_series_summary), one lane adds them over the chains; multi[series] as k_series_summary.
// PMAX > 0: the keys live in LDS (PP <= PMAX, PP = N rounded up to a power of two); PMAX == 0: in the workgroup's PP words of ws.
template <int PMAX, bool LOG_MODE>
__global__ __launch_bounds__(256) void k_pooled_summary(uint32_t count, uint32_t C, uint32_t S, const double *__restrict__ X, uint32_t np,
                                                        const int32_t *__restrict__ pind, double *cm, double *cv, double *ct,
                                                        const int32_t *__restrict__ crc, const uint8_t *__restrict__ multi, PoolOut o,
                                                        uint64_t *__restrict__ ws)
{
    constexpr bool IN_LDS = PMAX > 0;
    __shared__ uint64_t l_key[IN_LDS ? PMAX : 1];
    const uint32_t tid = threadIdx.x, N = C * S;
    const uint32_t PP = next_pow2(N);
    uint64_t *key;
    if constexpr (IN_LDS) key = l_key;
    else key = ws + (uint64_t)blockIdx.x * PP;
    const double dS = (double)S, dC = (double)C, dN = (double)N;
    for (uint32_t ser = blockIdx.x; ser < count; ser += gridDim.x) {
        __syncthreads();   // the previous series of this workgroup is done with the keys
        const double *x = X + (uint64_t)ser * N;
        for (uint32_t i = tid; i < PP; i += 256) key[i] = i < N ? order_key(x[i]) : ~0ull;   // padding sorts last
        __syncthreads();
        block_sort<256>(key, PP);
        for (uint32_t q = tid; q < np; q += 256) {
            const int32_t idx = pind[q];
            o.pct[(uint64_t)ser * np + q] = (idx >= 0 && (uint32_t)idx < N) ? order_unkey(key[idx]) : __builtin_nan("");
        }
        const uint64_t c0 = (uint64_t)ser * C;
        if constexpr (LOG_MODE) {
            if (tid == 0) {
                if (C == 1) {   // the chain's own values, copied
                    const int32_t rc = crc[c0];
                    o.a[ser] = cm[c0]; o.b[ser] = cv[c0]; o.rc[ser] = rc;
                    o.c[ser] = rc != 0 ? 0.0 : ct[c0];
                    o.mcse2[ser] = rc != 0 ? 0.0 : ct[c0] * cv[c0] / dS;
                } else {
                    double sm = 0.0, sv = 0.0, stv = 0.0;
                    int32_t rc = 0;
                    for (uint32_t c = 0; c < C; ++c) {
                        sm += cm[c0 + c];
                        sv += cv[c0 + c];
                        stv += ct[c0 + c] * cv[c0 + c];
                        if (rc == 0) rc = crc[c0 + c];
                    }
                    const double mean = sm / dC;
                    double sb = 0.0;
                    for (uint32_t c = 0; c < C; ++c) { const double e = cm[c0 + c] - mean; sb += e * e; }
                    o.a[ser] = mean;
                    o.b[ser] = ((dS - 1.0) * sv + dS * sb) / (dN - 1.0);
                    o.c[ser] = rc != 0 ? 0.0 : stv / sv;
                    o.mcse2[ser] = rc != 0 ? 0.0 : stv / dS / (dC * dC);
                    o.rc[ser] = rc;
                }
            }
        } else {
            const bool mm = multi[ser] != 0;
            for (uint32_t c = tid; c < C; c += 256) {
                const double *xc = x + (uint64_t)c * S;
                double sp = 0.0, s1 = 0.0, s2 = 0.0;
                for (uint32_t i = 0; i < S; ++i) {
                    sp += xc[i];
                    double z = __builtin_huge_val();
                    if (mm) {
                        double p = xc[i];
                        p = p < 0.000000001 ? 0.000000001 : p;   // as k_series_summary: a NaN stays a NaN
                        p = 0.999999999 < p ? 0.999999999 : p;
                        z = dprobit(p);
                    }
                    s1 += z;
                    s2 += z * z;
                }
                cm[c0 + c] = sp; cv[c0 + c] = s1; ct[c0 + c] = s2;
            }
            __syncthreads();   // (the chains' sums, written by other lanes of this workgroup, are visible)
            if (tid == 0) {
                double tp = 0.0, t1 = 0.0, t2 = 0.0;
                for (uint32_t c = 0; c < C; ++c) { tp += cm[c0 + c]; t1 += cv[c0 + c]; t2 += ct[c0 + c]; }
                o.a[ser] = tp / dN;
                o.b[ser] = t1 / dN;
                o.c[ser] = dsqrt((t2 - t1 * t1 / dN) / (dN - 1.0));
            }
        }
    }
}

} // namespace mmg
