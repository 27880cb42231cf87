// pair_kernels.h -- the posterior correlation of transcripts that share reads (mmg_pairs_*): for ordered pairs (a, b) of transcripts
// of one sample, from the kept samples of a chain, the two-pass second moments of log x_a, log x_b and log(x_a + x_b) and the
// number of samples with x_a > x_b.  Specification: tests/pairs_ref.py, DESIGN.md section 15.
//
// One wave per unit of work, lane = sample, four independent waves per workgroup.  Every series is a contiguous row of S doubles: the
// 64 lanes of a wave read 512 contiguous bytes per step.  A lane adds its samples lane, lane + 64, ... in ascending order from 0.0;
// the 64 partial sums are folded by halving (32, 16, 8, 4, 2, 1) and lane 0 stores.  Two kernels:
//   k_pair_members  a wave per distinct member of a slab of pairs: u = dlog(x), its mean, the centred series du = u - mean stored as
//                   a row of Cn, saa = sum du * du.  dlog of a member's sample is evaluated here once, however many pairs the member is in.
//   k_pair_stats    a wave per pair: w = dlog(x_a + x_b) from the members' rows of X, its mean and sss = sum dw * dw, sab = sum du * dv
//                   from the members' rows of Cn, the ballot count of x_a > x_b; the members' mean and saa copied beside them.
// Up to PAIR_REG_SAMPLES samples the logarithms of a lane's samples stay in registers between the two passes; beyond that they are
// evaluated again (dlog is deterministic: the same bits).  No atomics; products are rounded before they are added (-ffp-contract=off).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mmg_series.h"

namespace mmg {

constexpr uint32_t PAIR_LANES = 64;
constexpr uint32_t PAIR_BLOCK = 256;                              // four waves per workgroup, a member or a pair each
constexpr uint32_t PAIR_REG_BLOCKS = 16;                          // sample blocks of 64 a lane keeps in registers
constexpr uint32_t PAIR_REG_SAMPLES = PAIR_REG_BLOCKS * PAIR_LANES;   // 1024

// Member j < nm of wave j: x = X[(row ? row[j] : j) * S + s]; mean[j] = lsum(dlog x) / S, Cn[j * S + s] = dlog(x) - mean[j],
// saa[j] = lsum of the squares of that row.  REG: S <= PAIR_REG_SAMPLES.
template <bool REG>
__global__ __launch_bounds__(PAIR_BLOCK) void k_pair_members(uint32_t nm, uint32_t S, const uint32_t *__restrict__ row, const double *__restrict__ X,
                                                            double *__restrict__ Cn, double *__restrict__ mean, double *__restrict__ saa)
{
    const uint32_t lane = threadIdx.x & (PAIR_LANES - 1);
    const uint32_t j = __builtin_amdgcn_readfirstlane(blockIdx.x * (PAIR_BLOCK / PAIR_LANES) + (threadIdx.x >> 6));
    if (j >= nm) return;
    const double *const x = X + (uint64_t)(row ? row[j] : j) * S;
    double *const c = Cn + (uint64_t)j * S;
    const double div = (double)S;
    double A = 0.0, Q = 0.0;
    if constexpr (REG) {
        double u[PAIR_REG_BLOCKS];
#pragma unroll
        for (uint32_t b = 0; b < PAIR_REG_BLOCKS; ++b) {
            const uint32_t s = b * PAIR_LANES + lane;
            u[b] = 0.0;
            if (s < S) { u[b] = dlog(x[s]); A = A + u[b]; }
        }
        const double m = lane_sum(A) / div;
#pragma unroll
        for (uint32_t b = 0; b < PAIR_REG_BLOCKS; ++b) {
            const uint32_t s = b * PAIR_LANES + lane;
            if (s < S) {
                const double d = u[b] - m;
                c[s] = d;
                Q = Q + d * d;
            }
        }
        const double q = lane_sum(Q);
        if (lane == 0) { mean[j] = m; saa[j] = q; }
    } else {
        for (uint32_t s = lane; s < S; s += PAIR_LANES) A = A + dlog(x[s]);
        const double m = lane_sum(A) / div;
        for (uint32_t s = lane; s < S; s += PAIR_LANES) {
            const double d = dlog(x[s]) - m;
            c[s] = d;
            Q = Q + d * d;
        }
        const double q = lane_sum(Q);
        if (lane == 0) { mean[j] = m; saa[j] = q; }
    }
}

struct PairOut {
    double *mean_a, *mean_b, *mean_sum, *saa, *sbb, *sab, *sss;   // [np]
    uint32_t *n_gt;                                               // [np]
};

// Pair p < np of wave p, its members the slots sa[p], sb[p] < nm of the slab: x rows X[(row ? row[slot] : slot) * S ..], centred rows
// Cn[slot * S ..], mean / saa of the member pass.  REG: S <= PAIR_REG_SAMPLES.
template <bool REG>
__global__ __launch_bounds__(PAIR_BLOCK) void k_pair_stats(uint32_t np, uint32_t S, const uint32_t *__restrict__ sa, const uint32_t *__restrict__ sb,
                                                          const uint32_t *__restrict__ row, const double *__restrict__ X, const double *__restrict__ Cn,
                                                          const double *__restrict__ mean, const double *__restrict__ saa, PairOut o)
{
    const uint32_t lane = threadIdx.x & (PAIR_LANES - 1);
    const uint32_t p = __builtin_amdgcn_readfirstlane(blockIdx.x * (PAIR_BLOCK / PAIR_LANES) + (threadIdx.x >> 6));
    if (p >= np) return;
    const uint32_t ja = sa[p], jb = sb[p];
    const double *const xa = X + (uint64_t)(row ? row[ja] : ja) * S;
    const double *const xb = X + (uint64_t)(row ? row[jb] : jb) * S;
    const double *const ca = Cn + (uint64_t)ja * S;
    const double *const cb = Cn + (uint64_t)jb * S;
    const double div = (double)S;
    double A = 0.0, Q = 0.0, AB = 0.0;
    uint32_t count = 0;
    if constexpr (REG) {
        double w[PAIR_REG_BLOCKS];
#pragma unroll
        for (uint32_t b = 0; b < PAIR_REG_BLOCKS; ++b) {   // (b is uniform over the wave: the ballot sees every lane)
            const uint32_t s = b * PAIR_LANES + lane;
            const bool in = s < S;
            double va = 0.0, vb = 0.0;
            w[b] = 0.0;
            if (in) { va = xa[s]; vb = xb[s]; w[b] = dlog(va + vb); A = A + w[b]; }
            count += (uint32_t)__popcll(__ballot(in && va > vb));
        }
        const double m = lane_sum(A) / div;
#pragma unroll
        for (uint32_t b = 0; b < PAIR_REG_BLOCKS; ++b) {
            const uint32_t s = b * PAIR_LANES + lane;
            if (s < S) {
                const double d = w[b] - m;
                Q = Q + d * d;
                AB = AB + ca[s] * cb[s];
            }
        }
        const double q = lane_sum(Q), ab = lane_sum(AB);
        if (lane == 0) {
            o.mean_a[p] = mean[ja]; o.mean_b[p] = mean[jb]; o.mean_sum[p] = m;
            o.saa[p] = saa[ja]; o.sbb[p] = saa[jb]; o.sab[p] = ab; o.sss[p] = q; o.n_gt[p] = count;
        }
    } else {
        for (uint32_t sb0 = 0; sb0 < S; sb0 += PAIR_LANES) {   // (sb0 is uniform over the wave: the ballot sees every lane)
            const uint32_t s = sb0 + lane;
            const bool in = s < S;
            double va = 0.0, vb = 0.0;
            if (in) { va = xa[s]; vb = xb[s]; A = A + dlog(va + vb); }
            count += (uint32_t)__popcll(__ballot(in && va > vb));
        }
        const double m = lane_sum(A) / div;
        for (uint32_t s = lane; s < S; s += PAIR_LANES) {
            const double d = dlog(xa[s] + xb[s]) - m;
            Q = Q + d * d;
            AB = AB + ca[s] * cb[s];
        }
        const double q = lane_sum(Q), ab = lane_sum(AB);
        if (lane == 0) {
            o.mean_a[p] = mean[ja]; o.mean_b[p] = mean[jb]; o.mean_sum[p] = m;
            o.saa[p] = saa[ja]; o.sbb[p] = saa[jb]; o.sab[p] = ab; o.sss[p] = q; o.n_gt[p] = count;
        }
    }
}

} // namespace mmg
