// iso_kernels.h -- posterior isoform usage within groups of transcripts of one sample (mmg_isoform_*): which member of a group is
// the major one and with what probability, the entropy of the usage and the share of the top member, from the joint draws of the
// group's members in the kept samples of a chain.  Specification: tests/isoforms_ref.py, DESIGN.md section 18.
//
// The members' traces are rows of a series-major matrix M[slot][S] (gathered by k_contrast_gather, or the caller's host traces).
//   k_iso_series   one wave per group, lane = sample, in blocks of 64 samples.  Every lane walks the same member list, so the walk does
//                  not diverge and a member's samples are read along its row, 512 bytes per step.  The first walk takes the check,
//                  T_s, the top and the second (strict comparisons: the first of equals wins); the second walk takes the entropy and,
//                  per member, the ballots of top == j, second == j and x_j > theta_q T.  Lane k < 2 + nq adds the population count of
//                  ballot k to counter k of the member: always the same lane for the same word, a plain load and store (the counters
//                  are zeroed before the launch; one wave owns a group's counters).  A group with a sample that is not valid does no
//                  logarithm from that block on, and ends with NaN rows, 0xffffffff tops and zero counters.
//   k_iso_summary  one workgroup of four waves per group: the H and P series as 64-bit words in LDS, the moments in the fixed lane
//                  order of lane_sum (pairs_ref.lsum) by waves 0 and 1, major and n_distinct from the counters by wave 2, then
//                  both series as order-preserving keys, sorted bitonically and picked at the ranks: the shape of k_sim_pair.
// No floating-point atomics, no atomics at all; every sum runs in a fixed order: reruns and any slab cut give the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mmg_series.h"

namespace mmg {

constexpr uint32_t ISO_MAX_S = 4096;        // samples at most: 2 x 4096 words = 64 KiB of LDS in k_iso_summary
constexpr uint32_t ISO_MAX_THRESHOLDS = 8;
constexpr uint32_t ISO_MAX_RANKS = 64;
constexpr uint32_t ISO_BLOCK = 256, ISO_LANES = 64;   // four waves: a group each (series), or one group together (summary)
constexpr uint32_t ISO_NONE = 0xffffffffu;

struct IsoTheta { double v[ISO_MAX_THRESHOLDS]; };

// Group g = g0 + w of wave w < cnt, its members the slots slot[ptr[g] .. ptr[g + 1]) of M[slot][S] (ptr and slot are the whole
// description's: flat positions).  Rows w of top / second / H / P [cnt][S] (top and second may be null: not wanted), bad[w] = 1 when a
// sample is not valid.  cnt_words null: rows only.  Otherwise counter k of the member at flat position f is cnt_words[f * (2 + nq) + k],
// k = 0: n_top, 1: n_second, 2 + q: n_above[q]; zero before the launch.
__global__ __launch_bounds__(ISO_BLOCK) void k_iso_series(uint32_t g0, uint32_t cnt, uint32_t S, uint32_t nq, IsoTheta theta,
                                                         const uint64_t *__restrict__ ptr, const uint32_t *__restrict__ slot,
                                                         const double *__restrict__ M, uint32_t *__restrict__ top_row,
                                                         uint32_t *__restrict__ second_row, double *__restrict__ H_row, double *__restrict__ P_row,
                                                         uint8_t *__restrict__ bad_out, uint32_t *__restrict__ cnt_words)
{
    const uint32_t lane = threadIdx.x & (ISO_LANES - 1);
    const uint32_t w = __builtin_amdgcn_readfirstlane(blockIdx.x * (ISO_BLOCK / ISO_LANES) + (threadIdx.x >> 6));
    if (w >= cnt) return;
    const uint64_t jb = ptr[g0 + w], je = ptr[g0 + w + 1];
    const uint32_t stride = 2 + nq;
    const double nan = __builtin_nan("");
    const double dmax = 0x1.fffffffffffffp+1023;
    bool bad = false;   // (uniform over the wave: it comes from ballots)
    for (uint32_t sb = 0; sb < S; sb += ISO_LANES) {   // (sb is uniform over the wave: the ballots see every lane)
        const uint32_t s = sb + lane;
        const bool in = s < S;
        const double *const col = M + (in ? s : 0);   // (a lane past S reads sample 0 and is masked out of everything)
        // ---- the first walk: the check, T, the top and the second
        double T = 0.0, xt = 0.0, x2 = 0.0;
        uint32_t top = 0, second = ISO_NONE;
        bool ok = true;
        for (uint64_t j = jb; j < je; ++j) {
            const double x = col[(uint64_t)slot[j] * S];
            const uint32_t pos = (uint32_t)(j - jb);
            ok = ok && x >= 0.0 && x <= dmax;
            T = T + x;
            if (pos == 0) xt = x;
            else if (x > xt) { second = top; x2 = xt; top = pos; xt = x; }
            else if (second == ISO_NONE || x > x2) { second = pos; x2 = x; }
        }
        ok = ok && T > 0.0 && T <= dmax;
        if (__ballot(in && !ok)) bad = true;
        if (bad) break;   // (uniform) the group is not valid: nothing more is computed, the rows are overwritten below
        // ---- the second walk: the entropy, and the counters from ballots
        double th[ISO_MAX_THRESHOLDS];
#pragma unroll
        for (uint32_t q = 0; q < ISO_MAX_THRESHOLDS; ++q) th[q] = q < nq ? theta.v[q] * T : 0.0;
        double a = 0.0;
        for (uint64_t j = jb; j < je; ++j) {
            const double x = col[(uint64_t)slot[j] * S];
            const uint32_t pos = (uint32_t)(j - jb);
            const double p = x / T;
            if (p > 0.0) a = a + p * dlog(p);
            if (cnt_words) {
                uint32_t mine = 0;   // lane k < 2 + nq: the population count of ballot k
                const uint32_t ct = (uint32_t)__popcll(__ballot(in && top == pos));
                const uint32_t cs = (uint32_t)__popcll(__ballot(in && second == pos));
                if (lane == 0) mine = ct;
                if (lane == 1) mine = cs;
#pragma unroll
                for (uint32_t q = 0; q < ISO_MAX_THRESHOLDS; ++q) {
                    if (q < nq) {   // (uniform)
                        const uint32_t ca = (uint32_t)__popcll(__ballot(in && x > th[q]));
                        if (lane == 2 + q) mine = ca;
                    }
                }
                if (lane < stride) {
                    uint32_t *const c = cnt_words + j * stride + lane;
                    *c = *c + mine;
                }
            }
        }
        if (in) {
            const uint64_t o = (uint64_t)w * S + s;
            H_row[o] = (-a) + 0.0;
            P_row[o] = xt / T;
            if (top_row) top_row[o] = top;
            if (second_row) second_row[o] = second;
        }
    }
    if (bad) {
        for (uint32_t s = lane; s < S; s += ISO_LANES) {
            const uint64_t o = (uint64_t)w * S + s;
            H_row[o] = nan;
            P_row[o] = nan;
            if (top_row) top_row[o] = ISO_NONE;
            if (second_row) second_row[o] = ISO_NONE;
        }
        if (cnt_words && lane < stride)   // (the lane that added to a word is the one that clears it)
            for (uint64_t j = jb; j < je; ++j) cnt_words[j * stride + lane] = 0;
    }
    if (bad_out && lane == 0) bad_out[w] = bad ? 1 : 0;
}

struct IsoOut {
    double *mean_H, *ss_H, *mean_P, *ss_P;   // [cnt]
    double *q_H, *q_P;                       // [cnt][nr]
    uint32_t *major, *n_distinct;            // [cnt]
};

// Group g0 + blockIdx.x, blockIdx.x < cnt: rows blockIdx.x of H / P [cnt][S], its counters as k_iso_series left them.  PP >= S a power
// of two, 16 PP bytes of dynamic LDS; ranks[nr] zero-based, a rank >= S gives NaN.
__global__ __launch_bounds__(ISO_BLOCK) void k_iso_summary(uint32_t g0, uint32_t S, uint32_t PP, uint32_t nq, const uint64_t *__restrict__ ptr,
                                                          const double *__restrict__ H_row, const double *__restrict__ P_row,
                                                          const uint8_t *__restrict__ bad_in, const uint32_t *__restrict__ cnt_words, uint32_t nr,
                                                          const uint32_t *__restrict__ ranks, IsoOut o)
{
    extern __shared__ uint64_t iso_lds[];
    uint64_t *const kh = iso_lds, *const kp = iso_lds + PP;
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t b = blockIdx.x;
    const bool bad = bad_in[b] != 0;
    const double nan = __builtin_nan("");
    const double *const h = H_row + (uint64_t)b * S, *const p = P_row + (uint64_t)b * S;
    for (uint32_t s = tid; s < S; s += ISO_BLOCK) { kh[s] = bits_of(h[s]); kp[s] = bits_of(p[s]); }
    __syncthreads();

    if (w < 2) {   // ---- moments over the samples in their order: wave 0 the entropy, wave 1 the top proportion
        const uint64_t *const x = w ? kp : kh;
        double mean = nan, ss = nan;
        if (!bad) {
            double a = 0.0;
            for (uint32_t s = lane; s < S; s += 64) a = a + double_of(x[s]);
            mean = lane_sum(a) / (double)S;
            double q = 0.0;
            for (uint32_t s = lane; s < S; s += 64) { const double d = double_of(x[s]) - mean; q = q + d * d; }
            ss = lane_sum(q);
        }
        if (lane == 0) {
            if (w) { o.mean_P[b] = mean; o.ss_P[b] = ss; }
            else { o.mean_H[b] = mean; o.ss_H[b] = ss; }
        }
    } else if (w == 2) {   // ---- major = the smallest position with the largest n_top; n_distinct = positions with n_top > 0
        const uint64_t jb = ptr[g0 + b], K = ptr[g0 + b + 1] - jb;
        const uint32_t stride = 2 + nq;
        uint32_t best = 0, at = ISO_NONE, distinct = 0;
        for (uint64_t j0 = 0; j0 < K; j0 += 64) {   // (uniform: the ballot sees every lane)
            const uint64_t j = j0 + lane;
            const uint32_t c = j < K ? cnt_words[(jb + j) * stride] : 0;
            if (j < K && (at == ISO_NONE || c > best)) { best = c; at = (uint32_t)j; }   // (ascending j per lane: the first of equals stays)
            distinct += (uint32_t)__popcll(__ballot(c > 0));
        }
        for (uint32_t d = 32; d > 0; d >>= 1) {
            const uint32_t ob = __shfl_down(best, d, 64), oa = __shfl_down(at, d, 64);
            if (oa != ISO_NONE && (at == ISO_NONE || ob > best || (ob == best && oa < at))) { best = ob; at = oa; }
        }
        if (lane == 0) { o.major[b] = at; o.n_distinct[b] = distinct; }
    }
    __syncthreads();

    // ---- order statistics: both series sorted by key, the padding above every key
    if (!bad) {   // (uniform over the workgroup)
        for (uint32_t s = tid; s < PP; s += ISO_BLOCK) {
            kh[s] = s < S ? order_key(double_of(kh[s])) : ~0ull;
            kp[s] = s < S ? order_key(double_of(kp[s])) : ~0ull;
        }
        __syncthreads();
        block_sort<ISO_BLOCK>(kh, PP);
        block_sort<ISO_BLOCK>(kp, PP);
    }
    for (uint32_t k = tid; k < nr; k += ISO_BLOCK) {
        const uint32_t rk = ranks[k];
        o.q_H[(uint64_t)b * nr + k] = rk < S && !bad ? order_unkey(kh[rk]) : nan;
        o.q_P[(uint64_t)b * nr + k] = rk < S && !bad ? order_unkey(kp[rk]) : nan;
    }
}

} // namespace mmg
