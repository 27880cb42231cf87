// post_kernels.h -- the posterior summary of the Gibbs trace on the device (src/mmseq.cpp:927-1008 trace aggregation,
// :1110-1192 percentiles, :1195-1227 log means, :1235-1305 proportion summaries, :1307-1363 Sokal per feature; src/sokal.cc:33-87).
//
// The trace stays where K2 wrote it (sample-major [S][n] in device numbering).  Derived traces (simulated isoforms, sums over
// identical sets and genes, proportions) are built sample-major as well -- the layout the trace writers print, row by row -- and
// transposed once to series-major for the per-series summary kernel: one workgroup per series sorts the S samples (percentiles),
// logs them, and runs Sokal's estimator with two radix-2 FFTs in LDS.  Sums run in the reference's order (members of a group in
// the given order, samples ascending), the FFT uses the butterfly order and twiddle factors of the host implementation
// (mmseq_amd/csrc/host/numerics.hpp; the table is computed on the host and uploaded), so device and host agree to the rounding of
// log() alone.
#pragma once
#include "mmg_types.h"
#include "mmg_series.h"

namespace mmg {

// simulated traces of isoforms without hits (:971-978): V[s * nv + v] = Gamma(alpha) * scale[v], keyed (seed, chain, tag, id[v], s)
// (the summary: chain 0, TAG_SIMU; mmcollapse: chain = the sample, TAG_COLLAPSE_SIMU)
__global__ __launch_bounds__(256) void k_virtual_traces(uint64_t seed, uint32_t chain, uint32_t tag, double alpha, uint32_t nv, uint32_t S,
                                                        const uint64_t *__restrict__ id, const double *__restrict__ scale, double *__restrict__ V)
{
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (uint64_t)nv * S) return;
    const uint32_t s = (uint32_t)(gid / nv), v = (uint32_t)(gid % nv);
    Stream st(seed, chain, tag, id[v], s);
    V[gid] = gamma_unit(st, alpha) * scale[v];
}

// G[s * ng + g] = sum over the members of group g, in the given order, of their trace at sample s (:927-1008).
// member < n: the caller's transcript (device column int_of_ext[member]); member >= n: virtual transcript member - n.
__global__ __launch_bounds__(256) void k_group_sums(uint32_t ng, uint32_t S, uint32_t n, uint32_t nv, const uint64_t *__restrict__ ptr,
                                                    const uint32_t *__restrict__ member, const uint32_t *__restrict__ int_of_ext,
                                                    const double *__restrict__ trace, const double *__restrict__ V, double *__restrict__ G)
{
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (uint64_t)ng * S) return;
    const uint32_t s = (uint32_t)(gid / ng), g = (uint32_t)(gid % ng);
    double acc = 0.0;
    for (uint64_t j = ptr[g]; j < ptr[g + 1]; ++j) {
        const uint32_t m = member[j];
        acc += m < n ? trace[(uint64_t)s * n + (int_of_ext ? int_of_ext[m] : m)] : V[(uint64_t)s * nv + (m - n)];
    }
    G[gid] = acc;
}

// proportions of gene expression (:1014-1031): P[s * cnt + i] = x_i(s) / G[s * ng + gene_of[i]], i over the caller's transcripts
// (x from the trace) or over the virtual ones (x from V); gene_of == 0xffffffff: NaN (a transcript outside every gene)
__global__ __launch_bounds__(256) void k_proportions(uint32_t cnt, uint32_t S, uint32_t stride, const double *__restrict__ X,
                                                     const uint32_t *__restrict__ col_of, const uint32_t *__restrict__ gene_of, uint32_t ng,
                                                     const double *__restrict__ G, double *__restrict__ P)
{
    const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (uint64_t)cnt * S) return;
    const uint32_t s = (uint32_t)(gid / cnt), i = (uint32_t)(gid % cnt);
    const uint32_t g = gene_of[i];
    const double x = X[(uint64_t)s * stride + (col_of ? col_of[i] : i)];
    P[gid] = g == 0xffffffffu ? __builtin_nan("") : x / G[(uint64_t)s * ng + g];
}

// (dprobit, the inverse standard normal CDF of the proportion summaries: mmg_math.h)

struct SeriesOut {
    double *log_mean, *var, *tau;   // [count]      (log mode)
    int32_t *rc;                    // [count]      Sokal return code (src/sokal.cc:36-39)
    double *pct;                    // [count][np]  percentiles of the series itself (both modes)
    double *mean, *probit_mean, *probit_sd; // [count]  (proportion mode)
};

// The order statistics of the series x[0 .. S) by the whole workgroup of BLOCK threads: pct[q] = the pind[q]-th smallest value (NaNs
// sort last; NaN for a position outside [0, S)).  s_key: cap >= SP words, SP = next_pow2(S); the words [SP, cap) are padded as well.
// The caller synchronises before (the buffer is free) and, when it reuses the keys' storage, after (the picks are out).
template <uint32_t BLOCK>
__device__ __forceinline__ void series_order_stats(const double *x, uint32_t S, uint32_t SP, uint32_t cap, uint64_t *s_key, uint32_t np,
                                                   const int32_t *__restrict__ pind, double *pct)
{
    const uint32_t tid = threadIdx.x;
    for (uint32_t i = tid; i < S; i += BLOCK) s_key[i] = order_key(x[i]);
    for (uint32_t i = S + tid; i < cap; i += BLOCK) s_key[i] = ~0ull; // padding sorts last
    __syncthreads();
    block_sort<BLOCK>(s_key, SP);
    for (uint32_t q = tid; q < np; q += BLOCK) {
        const int32_t idx = pind[q];
        pct[q] = (idx >= 0 && (uint32_t)idx < S) ? order_unkey(s_key[idx]) : __builtin_nan("");
    }
}

// The mean and Sokal's var / tau of y = log x (TAKE_LOG) or y = x (:1195-1227, :1307-1363; src/sokal.cc:33-87) by a workgroup of 256
// threads: the return code, y in natural order into s_im, its sequential mean, the bit-reversed radix-2 transform of y, the power
// spectrum with the mean removed, its transform, and the window loop.  Thread 0 stores the results of series `ser` at mean[ser],
// var[ser], tau[ser] and rc_out[ser] (the arrays and the index, not four addresses: those would each hold a pair of scalar registers
// across the whole body).  s_re / s_im: S words each; s_pw: S words when SMAX == 0 (they may be the caller's sort keys), unused otherwise (the
// spectrum waits in registers).  Returns where there is nothing more to do for this series: rc != 0 after the mean, or the end.
// Every floating-point expression and its order is the contract here: k_series_summary, k_contrast_summary and the host
// implementation (host/numerics.hpp) give the same bits because they run the same operations in the same order.
template <int SMAX, bool TAKE_LOG>
__device__ __forceinline__ void series_sokal(const double *x, uint32_t S, uint32_t lg, double *s_re, double *s_im, double *s_pw,
                                             const double *__restrict__ tw, uint32_t ser, double *mean, double *var, double *tau, int32_t *rc_out)
{
    const uint32_t tid = threadIdx.x;
    __syncthreads();   // the order statistics are out: the keys' storage becomes the real parts
    int rc = 0;
    if (S > (2u << 20)) rc = 100;
    else if (S < 4) rc = 200;
    else if (S & (S - 1)) rc = 201;
    for (uint32_t i = tid; i < S; i += 256) { // natural order, for the mean
        if constexpr (TAKE_LOG) s_im[i] = dlog(x[i]);
        else s_im[i] = x[i];
    }
    __syncthreads();
    if (tid == 0) {
        double acc = 0.0;
        for (uint32_t i = 0; i < S; ++i) acc += s_im[i];
        mean[ser] = acc / (double)S;
    }
    if (rc != 0) {
        if (tid == 0) { rc_out[ser] = rc; var[ser] = 0.0; tau[ser] = 0.0; }
        return;
    }
    // y into the transform buffers in bit-reversed order (the host permutes after loading; same values)
    for (uint32_t i = tid; i < S; i += 256) s_re[__brev(i) >> (32 - lg)] = s_im[i];
    __syncthreads();
    for (uint32_t i = tid; i < S; i += 256) s_im[i] = 0.0;
    __syncthreads();
    auto fft = [&]() { // in-place radix-2 DIT on bit-reversed input: the butterflies of host/numerics.hpp:fft_pow2
        for (uint32_t len = 2; len <= S; len <<= 1) {
            const uint32_t half = len >> 1;
            for (uint32_t b = tid; b < (S >> 1); b += 256) {
                const uint32_t j = b & (half - 1), i = ((b / half) * len) + j, q = i + half;
                const double wr = tw[2 * (half + j)], wi = tw[2 * (half + j) + 1];
                const double xr = s_re[q] * wr - s_im[q] * wi, xi = s_re[q] * wi + s_im[q] * wr;
                const double ar = s_re[i], ai = s_im[i];
                s_re[q] = ar - xr; s_im[q] = ai - xi;
                s_re[i] = ar + xr; s_im[i] = ai + xi;
            }
            __syncthreads();
        }
    };
    fft();
    // power spectrum, mean removed, back into bit-reversed order for the second transform
    if constexpr (SMAX > 0) {
        double pw[(SMAX + 255) / 256];
        for (uint32_t i = tid, c = 0; i < S; i += 256, ++c) pw[c] = i == 0 ? 0.0 : s_re[i] * s_re[i] + s_im[i] * s_im[i];
        __syncthreads();
        for (uint32_t i = tid, c = 0; i < S; i += 256, ++c) { s_re[__brev(i) >> (32 - lg)] = pw[c]; s_im[i] = 0.0; }
    } else {
        for (uint32_t i = tid; i < S; i += 256) s_pw[i] = i == 0 ? 0.0 : s_re[i] * s_re[i] + s_im[i] * s_im[i];
        __syncthreads();
        for (uint32_t i = tid; i < S; i += 256) { s_re[__brev(i) >> (32 - lg)] = s_pw[i]; s_im[i] = 0.0; }
    }
    __syncthreads();
    fft();
    if (tid == 0) {
        const double n = (double)S;
        const double r0 = s_re[0];
        var[ser] = r0 / (n * (n - 1.0));
        const double c = 1.0 / r0;
        double sum = -0.333333333333333333333;
        int m = (int)S + 1;
        for (uint32_t i = 0; i < S; ++i) {
            sum += s_re[i] * c - 0.166666666666666666666;
            if (sum < 0) { m = (int)i + 1; break; }
        }
        tau[ser] = 2 * (sum + ((double)m - 1.0) / 6.0);
        rc_out[ser] = 0;
    }
}

// One workgroup per series of S samples at a time (series-major input X[series * S + s]); workgroup b takes the series b, b + gridDim.x, ...
//   LOG_MODE:  percentiles of x (:1110-1192); y = log x; mean of y (:1195-1227); Sokal var / tau of y (:1307-1363)
//   otherwise: percentiles of x; mean of x; mean and sd of probit(clamp(x)) when multi[series] (:1235-1305)
// SMAX > 0: the series is sorted and transformed in LDS (S <= SMAX; the sort keys and the real parts share their storage: the sort
// is over before the transform starts).  SMAX == 0: any S, in the workgroup's slice of ws (3 * SP * 8 bytes per workgroup, SP = S
// rounded up to a power of two) -- the same steps on global memory, for traces longer than LDS holds.
// S a power of two in [4, 2^21] for the Sokal part, else rc = 201 / 200 / 100 (src/sokal.cc:36-39).
template <int SMAX, bool LOG_MODE>
__global__ __launch_bounds__(256) void k_series_summary(uint32_t count, uint32_t S, const double *__restrict__ X, uint32_t np,
                                                        const int32_t *__restrict__ pind, const uint8_t *__restrict__ multi,
                                                        const double *__restrict__ tw /* [S] (cos, sin) pairs at tw[2 * (half + j)] */,
                                                        SeriesOut o, uint64_t *__restrict__ ws)
{
    constexpr bool IN_LDS = SMAX > 0;
    __shared__ uint64_t l_key[IN_LDS ? SMAX : 1];
    __shared__ double l_im[(IN_LDS && LOG_MODE) ? SMAX : 1];
    const uint32_t tid = threadIdx.x;
    const uint32_t SP = next_pow2(S);
    uint64_t *s_key;
    double *s_re, *s_im, *s_pw;
    uint32_t cap;
    if constexpr (IN_LDS) {
        s_key = l_key; s_re = reinterpret_cast<double *>(l_key); s_im = l_im; s_pw = nullptr; cap = SMAX;
    } else {
        s_key = ws + (uint64_t)blockIdx.x * 3 * SP; s_re = reinterpret_cast<double *>(s_key + SP); s_im = s_re + SP;
        s_pw = reinterpret_cast<double *>(s_key); cap = SP;
    }
    uint32_t lg = 0;
    while ((1u << lg) < S) ++lg;
    for (uint32_t ser = blockIdx.x; ser < count; ser += gridDim.x) {
        __syncthreads();   // the previous series of this workgroup is done with the buffers
        const double *x = X + (uint64_t)ser * S;
        series_order_stats<256>(x, S, SP, cap, s_key, np, pind, o.pct + (uint64_t)ser * np);
        if constexpr (LOG_MODE) {
            series_sokal<SMAX, true>(x, S, lg, s_re, s_im, s_pw, tw, ser, o.log_mean, o.var, o.tau, o.rc);
        } else {
            // sequential sums in sample order, as the reference (:1237-1262)
            if (tid == 0) {
                double sp = 0.0;
                for (uint32_t i = 0; i < S; ++i) sp += x[i];
                o.mean[ser] = sp / (double)S;
            }
            if (tid == 64) {
                const bool mm = multi[ser] != 0;
                double s1 = 0.0, s2 = 0.0;
                for (uint32_t i = 0; i < S; ++i) {
                    double z = __builtin_huge_val();
                    if (mm) {
                        double p = x[i];
                        p = p < 0.000000001 ? 0.000000001 : p;   // std::min(std::max(p, 1e-9), 1 - 1e-9) (:1250); a NaN stays a NaN
                        p = 0.999999999 < p ? 0.999999999 : p;
                        z = dprobit(p);
                    }
                    s1 += z;
                    s2 += z * z;
                }
                o.probit_mean[ser] = s1 / (double)S;
                o.probit_sd[ser] = dsqrt((s2 - s1 * s1 / (double)S) / ((double)S - 1.0));
            }
        }
    }
}

} // namespace mmg
