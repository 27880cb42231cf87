// fold_kernels.h -- the posterior log fold change of a feature between two samples from all pairs of their draws (mmg_fold_*).
// Feature f has the draws a[0 .. Sa) of sample A and b[0 .. Sb) of sample B, on the mu scale; x_i = dlog(a_i), y_j = dlog(b_j) + off,
// d_ij = x_i - y_j, each rounded once.  Specification: tests/fold_ref.py, DESIGN.md section 16.
//
// One workgroup of four waves per feature; the two series live in LDS as 64-bit words, PA + PB of them (Sa, Sb rounded up to powers of
// two), sized by the launch.  The steps:
//   load      every draw is checked (finite and > 0) before anything else: a feature with a bad draw gets its status bits, NaN and
//             zero counts, and the workgroup leaves -- no logarithm, no sort and no search ever sees such a series
//   moments   wave 0 takes x, wave 1 takes y, in the caller's sample order: lane l adds its samples l, l + 64, ... ascending from 0.0,
//             the 64 partial sums are folded by halving; mean = sum / S, then ss = the same sum over (v - mean) * (v - mean)
//   sort      the words become order-preserving keys (order_key), padded with ~0 above every finite key, and are sorted (bitonic, the
//             whole workgroup); then they are turned back into doubles in place
//   counts    per x_i a lower- and an upper-bound search in y: n_gt += #{y_j < x_i}, n_eq += #{y_j == x_i}; x and y are compared, never d
//   ranks     per requested rank k a bisection over the key space of d for the smallest key c with #{d_ij <= c} >= k + 1, at most 64
//             rounds; a round counts per row i the j with x_i - y_j <= c by a binary search (rounded subtraction is monotone: the row
//             is sorted), summed with integer adds.  The smallest such c is one of the d_ij: the k-th smallest, exactly.
// -0.0 is stored as +0.0 (x + 0.0), so keys order as the values compare.  No private memory, no floating-point atomics: reruns are
// bit-identical.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mmg_series.h"

namespace mmg {

constexpr uint32_t FOLD_BLOCK = 256;
constexpr uint32_t FOLD_MAX_S = 4096;      // draws per side at most: 2 x 4096 words = 64 KiB of LDS
constexpr uint32_t FOLD_MAX_RANKS = 64;
enum : uint8_t { FOLD_BAD_A = 1, FOLD_BAD_B = 2 };

// the sum of v over the workgroup, in every thread; sh: 4 words that no thread is still reading (the callers alternate two sets)
__device__ __forceinline__ uint32_t fold_block_add(uint32_t v, uint32_t *sh)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return sh[0] + sh[1] + sh[2] + sh[3];
}

struct FoldOut {
    double *mean_a, *mean_b, *ss_a, *ss_b;   // [count]
    uint32_t *n_gt, *n_eq;                   // [count]
    double *q;                               // [count][nr]
    uint8_t *status;                         // [count]
};

// Feature f = blockIdx.x < gridDim.x: a = A[f * Sa ..], b = B[f * Sb ..]; PA >= Sa and PB >= Sb powers of two, 8 (PA + PB) bytes of
// dynamic LDS; ranks[nr] zero-based, a rank >= Sa Sb gives NaN.
__global__ __launch_bounds__(FOLD_BLOCK) void k_fold(uint32_t Sa, uint32_t Sb, uint32_t PA, uint32_t PB, const double *__restrict__ A,
                                                     const double *__restrict__ B, double off, uint32_t nr, const uint32_t *__restrict__ ranks,
                                                     FoldOut o)
{
    extern __shared__ uint64_t fold_lds[];
    __shared__ uint32_t sh_cnt[2][4];
    __shared__ uint32_t sh_bad;
    uint64_t *const kx = fold_lds, *const ky = fold_lds + PA;
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t f = blockIdx.x;
    const double *const a = A + (uint64_t)f * Sa;
    const double *const b = B + (uint64_t)f * Sb;
    const double nan = __builtin_nan("");

    // ---- load: every draw finite and > 0, or the feature is left alone
    if (tid == 0) sh_bad = 0;
    __syncthreads();
    uint32_t bad = 0;
    for (uint32_t i = tid; i < Sa; i += FOLD_BLOCK) {
        const double v = a[i];
        if (v > 0.0 && v <= 0x1.fffffffffffffp+1023) kx[i] = bits_of(dlog(v) + 0.0);
        else bad |= FOLD_BAD_A;
    }
    for (uint32_t j = tid; j < Sb; j += FOLD_BLOCK) {
        const double v = b[j];
        if (v > 0.0 && v <= 0x1.fffffffffffffp+1023) ky[j] = bits_of((dlog(v) + off) + 0.0);
        else bad |= FOLD_BAD_B;
    }
    if (bad) atomicOr(&sh_bad, bad);
    __syncthreads();
    bad = sh_bad;   // (the same in every thread)
    if (bad) {
        if (tid == 0) {
            o.status[f] = (uint8_t)bad;
            o.mean_a[f] = nan; o.mean_b[f] = nan; o.ss_a[f] = nan; o.ss_b[f] = nan;
            o.n_gt[f] = 0; o.n_eq[f] = 0;
        }
        for (uint32_t r = tid; r < nr; r += FOLD_BLOCK) o.q[(uint64_t)f * nr + r] = nan;
        return;
    }

    // ---- moments, in the caller's sample order: wave 0 the side A, wave 1 the side B
    if (w < 2) {
        const uint64_t *const z = w ? ky : kx;
        const uint32_t S = w ? Sb : Sa;
        double s = 0.0;
        for (uint32_t i = lane; i < S; i += 64) s = s + double_of(z[i]);
        const double m = lane_sum(s) / (double)S;
        double q = 0.0;
        for (uint32_t i = lane; i < S; i += 64) { const double d = double_of(z[i]) - m; q = q + d * d; }
        q = lane_sum(q);
        if (lane == 0) {
            if (w) { o.mean_b[f] = m; o.ss_b[f] = q; }
            else { o.mean_a[f] = m; o.ss_a[f] = q; o.status[f] = 0; }
        }
    }
    __syncthreads();

    // ---- sort both sides by key; the padding sorts above every finite key
    for (uint32_t i = tid; i < PA; i += FOLD_BLOCK) kx[i] = i < Sa ? order_key(double_of(kx[i])) : ~0ull;
    for (uint32_t j = tid; j < PB; j += FOLD_BLOCK) ky[j] = j < Sb ? order_key(double_of(ky[j])) : ~0ull;
    __syncthreads();
    block_sort<FOLD_BLOCK>(kx, PA);
    block_sort<FOLD_BLOCK>(ky, PB);
    for (uint32_t i = tid; i < Sa; i += FOLD_BLOCK) kx[i] = bits_of(order_unkey(kx[i]));
    for (uint32_t j = tid; j < Sb; j += FOLD_BLOCK) ky[j] = bits_of(order_unkey(ky[j]));
    __syncthreads();

    // ---- counts: x against y
    uint32_t gt = 0, eq = 0;
    for (uint32_t i = tid; i < Sa; i += FOLD_BLOCK) {
        const double xi = double_of(kx[i]);
        uint32_t lo = 0, hi = Sb;
        while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (double_of(ky[mid]) < xi) lo = mid + 1; else hi = mid; }
        uint32_t up = lo;
        hi = Sb;
        while (up < hi) { const uint32_t mid = (up + hi) >> 1; if (double_of(ky[mid]) <= xi) up = mid + 1; else hi = mid; }
        gt += lo;
        eq += up - lo;
    }
    gt = fold_block_add(gt, sh_cnt[0]);
    eq = fold_block_add(eq, sh_cnt[1]);
    if (tid == 0) { o.n_gt[f] = gt; o.n_eq[f] = eq; }

    // ---- order statistics of d: bisection over its key space
    const uint64_t key_min = order_key((double_of(kx[0]) - double_of(ky[Sb - 1])) + 0.0);
    const uint64_t key_max = order_key((double_of(kx[Sa - 1]) - double_of(ky[0])) + 0.0);
    const uint32_t pairs = Sa * Sb;   // at most 2^24
    uint32_t par = 0;
    for (uint32_t r = 0; r < nr; ++r) {
        const uint32_t k = ranks[r];
        if (k >= pairs) {
            if (tid == 0) o.q[(uint64_t)f * nr + r] = nan;
            continue;
        }
        uint64_t lo = key_min, hi = key_max;   // the same in every thread: the counts are
        while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo) >> 1);
            const double c = order_unkey(mid);
            uint32_t cnt = 0;
            for (uint32_t i = tid; i < Sa; i += FOLD_BLOCK) {
                const double xi = double_of(kx[i]);
                uint32_t l = 0, h = Sb;   // x_i - y_j falls as j grows: the first j with x_i - y_j <= c
                while (l < h) { const uint32_t m = (l + h) >> 1; if (xi - double_of(ky[m]) <= c) h = m; else l = m + 1; }
                cnt += Sb - l;
            }
            cnt = fold_block_add(cnt, sh_cnt[par]);
            par ^= 1;
            if (cnt >= k + 1) hi = mid; else lo = mid + 1;
        }
        if (tid == 0) o.q[(uint64_t)f * nr + r] = order_unkey(lo) + 0.0;
    }
}

} // namespace mmg
