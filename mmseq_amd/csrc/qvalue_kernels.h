// qvalue_kernels.h -- device side of mmg_qvalues and mmg_diff_perm_qvalues: the log Bayes factor of every
// (replica, feature) of a permutation handle, and the q-values of observed statistics against null statistics.
//
// A statistic is compared through a key: the bits of the double with -0.0 made 0.0, flipped so that unsigned order is numeric order
// (-inf lowest, +inf highest).  No value that is not NaN has the key 0 or 2^64 - 1: an observed NaN takes 0 and sorts behind -inf in
// the descending sort, a null NaN takes 2^64 - 1 and sorts behind +inf in the ascending one, so the m observed and m0 null values
// that count are the heads of the two sorted arrays.
#pragma once
#include <hip/hip_runtime.h>
#include "mmg_series.h"

namespace mmg {

constexpr int QV_BLOCK = 256;

__device__ inline uint64_t qv_key(double x, uint64_t nan_key)
{
    if (x != x) return nan_key;
    return order_key(x == 0.0 ? 0.0 : x);
}

// T = log(g) - log(1 - g) - logit p' per (replica, feature): g = (sum of gamma) / sampled as mmg_diff_*_get_results forms it.  st: the
// replicas' state blocks one after the other (stride doubles each), gsum / logitp the slots of the two quantities.
__global__ void __launch_bounds__(QV_BLOCK) k_qv_stat(const double *__restrict__ st, size_t stride, int gsum, int logitp, uint32_t F, double sampled,
                                                      double *__restrict__ stat)
{
    const size_t f = (size_t)blockIdx.x * QV_BLOCK + threadIdx.x;
    if (f >= F) return;
    const double *s = st + stride * blockIdx.y;
    const double g = s[(size_t)gsum * F + f] / sampled, o = s[(size_t)logitp * F + f];
    double t = dlog(g) - dlog(1.0 - g) - o;
    if (!(o - o == 0.0)) t = __builtin_nan("");   // (a logit p' that is not finite: no Bayes factor)
    stat[(size_t)blockIdx.y * F + f] = t;
}

// keys of the observed values with their feature indices, and of the nulls
__global__ void __launch_bounds__(QV_BLOCK) k_qv_keys(const double *__restrict__ obs, uint32_t F, const double *__restrict__ null, uint64_t n_null,
                                                      uint64_t *__restrict__ okey, uint32_t *__restrict__ oidx, uint64_t *__restrict__ nkey)
{
    const uint64_t i = (uint64_t)blockIdx.x * QV_BLOCK + threadIdx.x;
    if (i < F) { okey[i] = qv_key(obs[i], 0); oidx[i] = (uint32_t)i; }
    if (i < n_null) nkey[i] = qv_key(null[i], ~0ull);
}

// the number of entries of the ascending a[0 .. n) below k / of the descending a[0 .. n) not below k.  The trip count depends on n
// alone, so the lanes of a wave stay together; they hold neighbouring sorted values and so probe the same or neighbouring entries.
__device__ inline uint64_t qv_count_below(const uint64_t *__restrict__ a, uint64_t n, uint64_t k)
{
    uint64_t lo = 0;
    for (uint64_t step = n ? 1ull << (63 - __builtin_clzll(n)) : 0; step; step >>= 1)
        if (lo + step <= n && a[lo + step - 1] < k) lo += step;
    return lo;
}
__device__ inline uint64_t qv_count_not_below_desc(const uint64_t *__restrict__ a, uint64_t n, uint64_t k)
{
    uint64_t lo = 0;
    for (uint64_t step = n ? 1ull << (63 - __builtin_clzll(n)) : 0; step; step >>= 1)
        if (lo + step <= n && a[lo + step - 1] >= k) lo += step;
    return lo;
}

// sizes[0] = m, sizes[1] = m0: the sorted keys that belong to no NaN
__global__ void k_qv_sizes(const uint64_t *__restrict__ okey, uint32_t F, const uint64_t *__restrict__ nkey, uint64_t n_null, uint64_t *__restrict__ sizes)
{
    if (threadIdx.x == 0) sizes[0] = qv_count_not_below_desc(okey, F, 1);
    if (threadIdx.x == 1) sizes[1] = qv_count_below(nkey, n_null, ~0ull);
}

// per sorted observed value i < m: V = the nulls not below it, R = the observed values not below it (the rank of the last equal one),
// fdr = min(1, V m / (m0 R)) -- stored at m - 1 - i, so that the running minimum from the least significant end is a forward scan
__global__ void __launch_bounds__(QV_BLOCK) k_qv_estimate(const uint64_t *__restrict__ okey, const uint64_t *__restrict__ nkey,
                                                          const uint64_t *__restrict__ sizes, uint64_t *__restrict__ V, double *__restrict__ fdr_rev)
{
    const uint64_t m = sizes[0], m0 = sizes[1];
    const uint64_t i = (uint64_t)blockIdx.x * QV_BLOCK + threadIdx.x;
    if (i >= m) return;
    const uint64_t k = okey[i];
    const uint64_t v = m0 - qv_count_below(nkey, m0, k);
    const uint64_t r = qv_count_not_below_desc(okey, m, k);
    V[i] = v;
    double x = __builtin_nan("");
    if (m0) {
        x = ((double)v * (double)m) / ((double)m0 * (double)r);
        x = x < 1.0 ? x : 1.0;
    }
    fdr_rev[m - 1 - i] = x;
}

// to feature order: q of the sorted value i is the scanned minimum at m - 1 - i; the observed NaNs (i >= m) get NaN and 0
__global__ void __launch_bounds__(QV_BLOCK) k_qv_scatter(const uint32_t *__restrict__ oidx, uint32_t F, const uint64_t *__restrict__ sizes,
                                                         const uint64_t *__restrict__ V, const double *__restrict__ qmin_rev,
                                                         uint64_t *__restrict__ null_ge, double *__restrict__ q)
{
    const uint64_t m = sizes[0];
    const uint64_t i = (uint64_t)blockIdx.x * QV_BLOCK + threadIdx.x;
    if (i >= F) return;
    const uint32_t f = oidx[i];
    null_ge[f] = i < m ? V[i] : 0;
    q[f] = i < m ? qmin_rev[m - 1 - i] : __builtin_nan("");
}

struct QvMin {
    __device__ double operator()(double a, double b) const { return b < a ? b : a; }
};

} // namespace mmg
