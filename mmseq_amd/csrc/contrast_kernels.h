// contrast_kernels.h -- posterior log-ratios between sets of transcripts of one sample, from the kept samples of a chain
// (mmg_contrast_*; specification in tests/contrast_ref.py).
//
// A contrast has a numerator and a denominator list of members (member < n: the caller's transcript, n + v: isoform without hits v).
// Per kept sample s: N_s and D_s the sums of the members' traces in list order (the sequential sums of k_group_sums),
// r_s = dlog(N_s) - dlog(D_s), gt_s = N_s > D_s.  Per contrast: the mean of r, Sokal's var / tau of r, order statistics of r, the
// share of samples with gt_s.  Three kernels:
//   k_contrast_gather   the distinct members of a slab of contrasts, out of the chain's sample-major trace (device numbering) and
//                       the simulated traces, into a series-major matrix M[slot][S]
//   k_contrast_series   one wave per contrast, lane = sample: walks the two slot lists over M, writes R[contrast][S] and the count of gt_s
//   k_contrast_summary  one workgroup per series of R at a time: the steps of k_series_summary<SMAX, true> (post_kernels.h) on y = R
//                       itself instead of on log x -- the same two device functions, so the same operations in the same order: that
//                       order is the contract behind both kernels' output bits
// No floating-point atomics; every sum runs in a fixed order: reruns are bit-identical.
#pragma once
#include "post_kernels.h"

namespace mmg {

// M[j * S + s] = the trace of member col[j] at sample s, j < nm:
//   col[j] <  n: trace[s * n + int_of_ext[col[j]]]  (int_of_ext null: the identity)
//   col[j] >= n: the simulated trace of isoform v = col[j] - n, Gamma(alpha) * scale[v] keyed (seed, chain 0, TAG_SIMU, id[v], s) --
//                the expression of k_virtual_traces, so the same bits
// 32 x 32 tiles through LDS, as k_transpose: the reads run along the trace's rows, the writes along M's.
__global__ __launch_bounds__(256) void k_contrast_gather(uint32_t nm, uint32_t S, uint32_t n, const uint32_t *__restrict__ col,
                                                         const uint32_t *__restrict__ int_of_ext, const double *__restrict__ trace,
                                                         uint64_t seed, double alpha, const uint64_t *__restrict__ vid,
                                                         const double *__restrict__ vscale, double *__restrict__ M)
{
    __shared__ double tile[32][33];
    const uint32_t j0 = blockIdx.x * 32, s0 = blockIdx.y * 32;
    const uint32_t tx = threadIdx.x & 31, ty = threadIdx.x >> 5; // 32 x 8
    const uint32_t jj = j0 + tx;
    const uint32_t m = jj < nm ? col[jj] : 0;
    const bool real = m < n;
    const uint32_t src = real ? (int_of_ext ? int_of_ext[m] : m) : m - n;
    for (uint32_t i = ty; i < 32; i += 8) {
        const uint32_t s = s0 + i;
        if (s < S && jj < nm) {
            if (real) tile[i][tx] = trace[(uint64_t)s * n + src];
            else {
                Stream st(seed, 0u, (uint32_t)TAG_SIMU, vid[src], s);
                tile[i][tx] = gamma_unit(st, alpha) * vscale[src];
            }
        }
    }
    __syncthreads();
    for (uint32_t i = ty; i < 32; i += 8) {
        const uint32_t j = j0 + i, s = s0 + tx;
        if (s < S && j < nm) M[(uint64_t)j * S + s] = tile[tx][i];
    }
}

constexpr uint32_t CTR_BLOCK = 256, CTR_LANES = 64;   // four waves, a contrast each

// Contrast c0 + w of wave w < cnt: R[w * S + s] = dlog(N_s) - dlog(D_s) with N_s = sum_j M[num_slot[j] * S + s] over
// j in [num_ptr[c], num_ptr[c + 1]) ascending from 0.0, D_s alike; gt[w] = the number of samples with N_s > D_s (gt null: not wanted).
// Every lane of a wave follows the same two lists: the walk does not diverge, and a member's S values are read along its row.
__global__ __launch_bounds__(CTR_BLOCK) void k_contrast_series(uint32_t c0, uint32_t cnt, uint32_t S, const uint64_t *__restrict__ num_ptr,
                                                              const uint32_t *__restrict__ num_slot, const uint64_t *__restrict__ den_ptr,
                                                              const uint32_t *__restrict__ den_slot, const double *__restrict__ M,
                                                              double *__restrict__ R, uint32_t *__restrict__ gt)
{
    const uint32_t w = blockIdx.x * (CTR_BLOCK / CTR_LANES) + threadIdx.x / CTR_LANES, lane = threadIdx.x % CTR_LANES;
    if (w >= cnt) return;
    const uint64_t nb = num_ptr[c0 + w], ne = num_ptr[c0 + w + 1], db = den_ptr[c0 + w], de = den_ptr[c0 + w + 1];
    uint32_t count = 0;
    for (uint32_t sb = 0; sb < S; sb += CTR_LANES) {   // (sb is uniform over the wave: the ballot below sees every lane)
        const uint32_t s = sb + lane;
        const bool in = s < S;
        double N = 0.0, D = 0.0;
        if (in) {
            for (uint64_t j = nb; j < ne; ++j) N += M[(uint64_t)num_slot[j] * S + s];
            for (uint64_t j = db; j < de; ++j) D += M[(uint64_t)den_slot[j] * S + s];
            R[(uint64_t)w * S + s] = dlog(N) - dlog(D);
        }
        count += (uint32_t)__popcll(__ballot(in && N > D));
    }
    if (gt && lane == 0) gt[w] = count;
}

struct ContrastOut {
    double *log_ratio, *var, *tau;  // [count]
    int32_t *rc;                    // [count]      Sokal return code (src/sokal.cc:36-39)
    double *pct;                    // [count][np]  order statistics of the series
};

// One workgroup per series of S samples at a time (series-major input R[series * S + s]); workgroup b takes the series b, b + gridDim.x, ...
// k_series_summary<SMAX, true> (post_kernels.h) on y = R itself instead of on log x: the same buffers, series_order_stats for the order
// statistics at pind, series_sokal<SMAX, false> for the mean and Sokal's var / tau.
// SMAX > 0: in LDS (S <= SMAX).  SMAX == 0: any S, in the workgroup's slice of ws (3 * SP * 8 bytes, SP = S rounded up to a power of two).
// S a power of two in [4, 2^21] for the Sokal part, else rc = 201 / 200 / 100.
template <int SMAX>
__global__ __launch_bounds__(256) void k_contrast_summary(uint32_t count, uint32_t S, const double *__restrict__ X, uint32_t np,
                                                          const int32_t *__restrict__ pind,
                                                          const double *__restrict__ tw /* [S] (cos, sin) pairs at tw[2 * (half + j)] */,
                                                          ContrastOut o, uint64_t *__restrict__ ws)
{
    constexpr bool IN_LDS = SMAX > 0;
    __shared__ uint64_t l_key[IN_LDS ? SMAX : 1];
    __shared__ double l_im[IN_LDS ? SMAX : 1];
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
        series_sokal<SMAX, false>(x, S, lg, s_re, s_im, s_pw, tw, ser, o.log_ratio, o.var, o.tau, o.rc);
    }
}

} // namespace mmg
