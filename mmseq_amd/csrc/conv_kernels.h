// conv_kernels.h -- between-chain convergence diagnostics of the resident traces on the device: the rank-normalized split R-hat and the
// bulk and tail effective sample sizes of Vehtari, Gelman, Simpson, Carpenter and Buerkner (2021), as Stan and ArviZ report them.
// DESIGN.md section 11 states the definitions; tests/convergence_ref.py restates them in numpy.
//
// One workgroup per series of C chains x S draws (series-major input X[series][C][S]).  N = S / 2 draws per split chain (for odd S the
// middle draw is dropped), M = 2C split chains, P = M N pooled draws; split chain j = 2c + h is chain c's first (h = 0) or last half.
// Per series the workgroup sorts the pooled draws (block_sort on order_key: mmg_series.h), reads the median and the 5 % / 95 %
// quantiles off the sorted keys, ranks every draw by a lower / upper-bound search of its own key (ties get their average rank) and
// maps the rank to a normal score with dprobit; then the same for the draws folded about the median.  Sums over a split chain and over
// the lags of the autocovariances run in a fixed order (lanes strided, then a butterfly over the wave), so reruns are bit-identical.
// The autocovariances are computed directly, lag by lag, in chunks of doubling size: Geyer's truncation usually needs few of them.
#pragma once
#include "post_kernels.h"

namespace mmg {

// the sum of v over the 64 lanes; every lane holds the same bits (each step adds two partial sums, a + b == b + a).  An xor butterfly,
// not the halving order of lane_sum (mmg_series.h): it associates the 64 values differently, and its bits are R-hat's and ESS's contract
__device__ __forceinline__ double conv_wave_sum(double v)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// pooled draw i of a series: split chain j = i / N, draw n = i % N of it
__device__ __forceinline__ double conv_draw(const double *__restrict__ x, uint32_t i, uint32_t N, uint32_t S)
{
    const uint32_t j = i / N, n = i - j * N;
    return x[(uint64_t)(j >> 1) * S + ((j & 1) ? S - N + n : n)];
}

// normal score of the draw with key `key` among the P sorted keys: z = probit((r - 3/8) / (P + 1/4)), r its average 1-based rank
__device__ __forceinline__ double conv_z(const uint64_t *k, uint32_t P, uint64_t key)
{
    uint32_t lo = 0, hi = P;
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (k[mid] < key) lo = mid + 1; else hi = mid; }
    uint32_t up = lo;
    hi = P;
    while (up < hi) { const uint32_t mid = (up + hi) >> 1; if (k[mid] <= key) up = mid + 1; else hi = mid; }
    const double r = 0.5 * ((double)lo + (double)up + 1.0);   // positions lo .. up - 1: ranks lo + 1 .. up
    return dprobit((r - 0.375) / ((double)P + 0.25));
}

// numpy's default quantile (method "linear": h = (P - 1) p, its two-sided lerp) of the P sorted keys
__device__ __forceinline__ double conv_quantile(const uint64_t *k, uint32_t P, double p)
{
    const double vi = (double)(P - 1) * p;
    if (vi >= (double)(P - 1)) return order_unkey(k[P - 1]);
    const double fl = __builtin_floor(vi);
    const uint32_t lo = (uint32_t)fl;
    const double g = vi - fl, a = order_unkey(k[lo]), b = order_unkey(k[lo + 1]);
    const double d = b - a;
    return g >= 0.5 ? b - d * (1.0 - g) : a + d * g;
}

// R-hat and (want_ess) the effective sample size of the M split chains y[j * N + n], by the whole workgroup.  y is centred in place;
// wk holds N + M doubles of scratch (the autocovariances, turned into the autocorrelations rho in place, and the chain means);
// sh: 9 doubles, flag: 1 int of shared memory.  The results are valid in thread 0.  Ends synchronised.
__device__ void conv_split_stats(double *y, double *wk, uint32_t N, uint32_t M, bool want_ess, double inv_log10_p, double *sh, int *flag,
                                 double &rhat, double &ess)
{
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    double *ac = wk, *mj = wk + N;
    const double dn = (double)N, dm = (double)M;
    double sm = 0.0, ss = 0.0;   // this wave's sums of chain means and of squared deviations, its chains in ascending order
    for (uint32_t j = w; j < M; j += 4) {
        double *yj = y + (uint64_t)j * N;
        double s = 0.0;
        for (uint32_t n = lane; n < N; n += 64) s += yj[n];
        const double m = conv_wave_sum(s) / dn;
        double s2 = 0.0;
        for (uint32_t n = lane; n < N; n += 64) { const double d = yj[n] - m; yj[n] = d; s2 += d * d; }
        s2 = conv_wave_sum(s2);
        if (lane == 0) mj[j] = m;
        sm += m;
        ss += s2;
    }
    if (lane == 0) { sh[2 * w] = sm; sh[2 * w + 1] = ss; }
    __syncthreads();
    const double mbar = (((sh[0] + sh[2]) + sh[4]) + sh[6]) / dm;
    const double sum_s2 = ((sh[1] + sh[3]) + sh[5]) + sh[7];
    if (w == 0) {
        double b = 0.0;
        for (uint32_t j = lane; j < M; j += 64) { const double e = mj[j] - mbar; b += e * e; }
        b = conv_wave_sum(b);
        if (lane == 0) sh[8] = b;
    }
    __syncthreads();
    const double var_m = sh[8] / (dm - 1.0);          // var_j(m_j), divisor M - 1
    const double W = sum_s2 / (dn - 1.0) / dm;          // mean_j v_j, v_j with divisor N - 1
    const double B = dn * var_m;
    rhat = dsqrt(((dn - 1.0) / dn * W + B / dn) / W); // IEEE as written: W = 0 < B gives +inf, W = B = 0 NaN
    if (!want_ess) { __syncthreads(); return; }

    // Geyer's initial positive and monotone sequences over the mean autocovariance of the split chains; thread 0 walks them while
    // the workgroup supplies the lags [have, want) the walk needs next
    const uint32_t P = N * M;
    uint32_t have = 0, t = 1;
    double even = 1.0, odd = 0.0, mean_var = 0.0, var_plus = 0.0;
    bool nan_rho = false;
    for (;;) {
        const uint32_t want = have + (have > 16 ? have : 16) < N ? have + (have > 16 ? have : 16) : N;
        for (uint32_t lag = have + w; lag < want; lag += 4) {
            double s = 0.0;
            for (uint32_t i = lane; i < P; i += 64) {
                const uint32_t n = i % N;
                if (n + lag < N) s += y[i] * y[i + lag];
            }
            s = conv_wave_sum(s);
            if (lane == 0) ac[lag] = s / dn / dm;     // mean_j acov[j][lag], acov with divisor N
        }
        __syncthreads();
        const bool first = have == 0;
        have = want;
        if (tid == 0) {
            int more = 0;
            if (first) {
                mean_var = ac[0] * dn / (dn - 1.0);
                var_plus = mean_var * (dn - 1.0) / dn + var_m;
                odd = 1.0 - (mean_var - ac[1]) / var_plus;
                nan_rho = __builtin_isnan(odd);
                ac[0] = 1.0;
                ac[1] = odd;
            }
            while ((int)t < (int)N - 3 && even + odd > 0.0) {
                if (t + 2 >= have) { more = 1; break; }
                even = 1.0 - (mean_var - ac[t + 1]) / var_plus;
                odd = 1.0 - (mean_var - ac[t + 2]) / var_plus;
                const bool keep = even + odd >= 0.0;
                ac[t + 1] = keep ? even : 0.0;   // (rho starts as zeros: a pair that is not kept stays 0)
                ac[t + 2] = keep ? odd : 0.0;
                t += 2;
            }
            *flag = more;
        }
        __syncthreads();
        if (!*flag) break;
    }
    if (tid == 0) {
        const int max_t = (int)t - 2;
        if (even > 0.0) ac[max_t + 1] = even;
        for (int u = 1; u <= max_t - 2; u += 2)
            if (ac[u + 1] + ac[u + 2] > ac[u - 1] + ac[u]) { const double a = (ac[u - 1] + ac[u]) / 2.0; ac[u + 1] = a; ac[u + 2] = a; }
        double sum = 0.0;
        for (int u = 0; u <= max_t; ++u) sum += ac[u];
        double tau = -1.0 + 2.0 * sum + ac[max_t + 1];
        tau = tau < inv_log10_p ? inv_log10_p : tau;
        ess = nan_rho ? __builtin_nan("") : (double)P / tau;
    }
    __syncthreads();
}

// One workgroup per series (workgroup b takes the series b, b + gridDim.x, ...): rhat = fmax(R-hat of the ranks, R-hat of the ranks
// of the draws folded about the median), ess_bulk = ESS of the ranks, ess_tail = fmin(ESS(I[x <= q05]), ESS(I[x <= q95])); NaN x 3
// for a series whose draws are all equal.  SMAX > 0: the sort keys and the transformed draws live in LDS (C S <= SMAX, 16 SMAX bytes);
// SMAX == 0: any C S, in the workgroup's slice of ws (2 PP words, PP = P rounded up to a power of two).  The draws themselves are
// read from X whenever they are needed (they are not kept in LDS).
template <int SMAX>
__global__ __launch_bounds__(256) void k_convergence(uint32_t count, uint32_t C, uint32_t S, const double *__restrict__ X, double inv_log10_p,
                                                     double *__restrict__ rhat_o, double *__restrict__ ess_bulk_o, double *__restrict__ ess_tail_o,
                                                     uint64_t *__restrict__ ws)
{
    constexpr bool IN_LDS = SMAX > 0;
    __shared__ uint64_t l_key[IN_LDS ? SMAX : 1];
    __shared__ double l_y[IN_LDS ? SMAX : 1];
    __shared__ double sh[9];
    __shared__ int flag;
    const uint32_t tid = threadIdx.x, N = S / 2, M = 2 * C, P = M * N;
    const uint32_t PP = next_pow2(P);
    uint64_t *key;
    double *y;
    if constexpr (IN_LDS) {
        key = l_key; y = l_y;
    } else {
        key = ws + (uint64_t)blockIdx.x * 2 * PP; y = reinterpret_cast<double *>(key + PP);
    }
    double *wk = reinterpret_cast<double *>(key);   // scratch of conv_split_stats while the keys are not needed (N + M <= P words)
    for (uint32_t ser = blockIdx.x; ser < count; ser += gridDim.x) {
        __syncthreads();   // the previous series of this workgroup is done with the buffers
        const double *x = X + (uint64_t)ser * C * S;
        for (uint32_t i = tid; i < PP; i += 256) key[i] = i < P ? order_key(conv_draw(x, i, N, S) + 0.0) : ~0ull; // (+ 0.0: -0 ties +0)
        __syncthreads();
        block_sort<256>(key, PP);
        if (key[0] == key[P - 1]) {   // a constant series (the same answer in every thread: the keys are sorted and synchronised)
            if (tid == 0) { rhat_o[ser] = __builtin_nan(""); ess_bulk_o[ser] = __builtin_nan(""); ess_tail_o[ser] = __builtin_nan(""); }
            continue;
        }
        const double med = (order_unkey(key[P / 2 - 1]) + order_unkey(key[P / 2])) / 2.0;
        const double q05 = conv_quantile(key, P, 0.05), q95 = conv_quantile(key, P, 0.95);
        // bulk: normal scores of the ranks
        for (uint32_t i = tid; i < P; i += 256) y[i] = conv_z(key, P, order_key(conv_draw(x, i, N, S) + 0.0));
        __syncthreads();
        double rhat_bulk = 0.0, ess_bulk = 0.0, rhat_tail = 0.0, ess_lo = 0.0, ess_hi = 0.0, unused = 0.0;
        conv_split_stats(y, wk, N, M, true, inv_log10_p, sh, &flag, rhat_bulk, ess_bulk);
        // folded about the median
        for (uint32_t i = tid; i < PP; i += 256) key[i] = i < P ? order_key(dabs(conv_draw(x, i, N, S) - med)) : ~0ull;
        __syncthreads();
        block_sort<256>(key, PP);
        for (uint32_t i = tid; i < P; i += 256) y[i] = conv_z(key, P, order_key(dabs(conv_draw(x, i, N, S) - med)));
        __syncthreads();
        conv_split_stats(y, wk, N, M, false, inv_log10_p, sh, &flag, rhat_tail, unused);
        // tails: indicators of the 5 % and 95 % quantiles
        for (uint32_t i = tid; i < P; i += 256) y[i] = conv_draw(x, i, N, S) <= q05 ? 1.0 : 0.0;
        __syncthreads();
        conv_split_stats(y, wk, N, M, true, inv_log10_p, sh, &flag, unused, ess_lo);
        for (uint32_t i = tid; i < P; i += 256) y[i] = conv_draw(x, i, N, S) <= q95 ? 1.0 : 0.0;
        __syncthreads();
        conv_split_stats(y, wk, N, M, true, inv_log10_p, sh, &flag, unused, ess_hi);
        if (tid == 0) {
            rhat_o[ser] = __builtin_fmax(rhat_bulk, rhat_tail);
            ess_bulk_o[ser] = ess_bulk;
            ess_tail_o[ser] = __builtin_fmin(ess_lo, ess_hi);
        }
    }
}

// out[(t * C + c) * S + s] = in[s * ld + col(t0 + t)] for t < cnt, s < S: chain c of a slab of series, series-major (col: int_of_ext, or
// the identity when null)
__global__ __launch_bounds__(256) void k_conv_slab(const double *__restrict__ in, uint64_t ld, uint32_t t0, uint32_t cnt, uint32_t S, uint32_t C,
                                                   uint32_t c, const uint32_t *__restrict__ col, double *__restrict__ out)
{
    __shared__ double tile[32][33];
    const uint32_t tb = blockIdx.x * 32, s0 = blockIdx.y * 32;
    const uint32_t tx = threadIdx.x & 31, ty = threadIdx.x >> 5; // 32 x 8
    const uint32_t tt = tb + tx;
    const uint64_t src = tt < cnt ? (col ? col[t0 + tt] : t0 + tt) : 0;
    for (uint32_t i = ty; i < 32; i += 8) {
        const uint32_t s = s0 + i;
        if (s < S && tt < cnt) tile[i][tx] = in[(uint64_t)s * ld + src];
    }
    __syncthreads();
    for (uint32_t i = ty; i < 32; i += 8) {
        const uint32_t t = tb + i, s = s0 + tx;
        if (s < S && t < cnt) out[((uint64_t)t * C + c) * S + s] = tile[tx][i];
    }
}

} // namespace mmg
