// assign_kernels.h -- the posterior assignment probability of every hit (mmg_assign_*): for a hit (i, t) the mean over the kept
// samples s of mu_s[t] / sum_{t' in row i} mu_s[t'], the Rao-Blackwellised estimate of what the sample kernel draws and discards.
// Specification: tests/assign_ref.py, DESIGN.md section 12.
//
// One wave per run of rows, lane = sample.  The trace is transcript-major (tr[t * stride + s]): the 64 lanes of a wave read 512
// contiguous bytes per hit, all lanes walk the same row (no divergence on its length), and the sequential sum D of the specification
// is each lane's own loop.  A lane adds its samples s = lane, lane + 64, ... in ascending order; the 64 partial sums are folded by
// halving (32, 16, 8, 4, 2, 1) and lane 0 stores P.  No floating-point atomics: a rerun gives the same bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mmg_series.h"   // lane_fold

namespace mmg {

constexpr uint32_t ASG_LANES = 64;
constexpr uint32_t ASG_BLOCK = 256;            // four waves per workgroup, each on rows of its own
constexpr uint32_t ASG_REG_HITS = 8;           // rows up to this length keep their hits' partial sums in registers
constexpr uint32_t ASG_HITS_PER_WAVE = 256;    // wave g owns the rows that start at hit offsets [g, g + 1) * ASG_HITS_PER_WAVE
constexpr uint64_t ASG_SCRATCH_BYTES = 64ull << 20;

// samples padded to whole blocks of 64
__host__ __device__ inline uint32_t asg_pad(uint32_t count) { return (count + ASG_LANES - 1) / ASG_LANES * ASG_LANES; }
// Waves of one launch.  A wave keeps one double per padded sample (the reciprocal sums of the row it is on) in a slice of the
// scratch buffer; a launch covers as many waves as ASG_SCRATCH_BYTES hold slices for (one at least), `max_waves` if that is less
// and not 0, and never more than there are.
__host__ __device__ inline uint64_t asg_chunk_waves(uint64_t n_waves, uint32_t count, uint32_t max_waves)
{
    uint64_t w = ASG_SCRATCH_BYTES / ((uint64_t)asg_pad(count) * 8);
    if (w == 0) w = 1;
    if (max_waves && w > max_waves) w = max_waves;
    if (w > n_waves) w = n_waves;
    return w ? w : 1;
}

struct AsgArgs {
    const uint64_t *row_ptr;   // n_rows + 1
    const uint32_t *col;
    uint64_t n_rows;
    const double *tr;          // tr[t * stride + s]
    uint64_t stride;
    uint32_t first, count;     // the samples [first, first + count)
    uint64_t wave0;            // global index of the launch's first wave
    uint32_t n_waves;          // waves of this launch
    double *scratch;           // n_waves slices of asg_pad(count) doubles
    double *P;                 // one per hit
};

// first row r < n_rows with row_ptr[r] >= x, n_rows if none
__device__ inline uint64_t asg_first_row_at(const uint64_t *row_ptr, uint64_t n_rows, uint64_t x)
{
    uint64_t lo = 0, hi = n_rows;
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (row_ptr[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(ASG_BLOCK) void k_assign(AsgArgs a)
{
    const uint32_t lane = threadIdx.x & (ASG_LANES - 1);
    const uint32_t wl = __builtin_amdgcn_readfirstlane(blockIdx.x * (ASG_BLOCK / ASG_LANES) + (threadIdx.x >> 6));
    if (wl >= a.n_waves) return;
    // rows dealt by hit count: this wave owns the rows whose first hit lies in its interval of ASG_HITS_PER_WAVE hit offsets, so a
    // row of thousands of hits has a wave to itself (the waves whose intervals it covers own nothing) and short rows come 256 hits
    // at a time.  Empty rows produce nothing, whoever owns them.
    const uint64_t g = a.wave0 + wl;
    uint64_t r = asg_first_row_at(a.row_ptr, a.n_rows, g * ASG_HITS_PER_WAVE);
    const uint64_t r_end = asg_first_row_at(a.row_ptr, a.n_rows, (g + 1) * ASG_HITS_PER_WAVE);
    const uint32_t nb = asg_pad(a.count) / ASG_LANES;
    double *const rs = a.scratch + (uint64_t)wl * asg_pad(a.count);
    const double *const tr = a.tr + a.first;
    const double div = (double)a.count;
    for (; r < r_end; ++r) {
        const uint64_t b = a.row_ptr[r], e = a.row_ptr[r + 1];
        const uint32_t L = (uint32_t)(e - b);
        if (L == 0) continue;
        if (L == 1) {                              // nothing to divide: 1 whatever the trace holds (v * (1 / v) is not always 1)
            if (lane == 0) a.P[b] = 1.0;
            continue;
        }
        const double flat = 1.0 / (double)L;
        if (L <= ASG_REG_HITS) {
            // one walk: the row's trace values of a sample block stay in registers between the sum and the products
            const double *src[ASG_REG_HITS];
            double A[ASG_REG_HITS];
#pragma unroll
            for (uint32_t j = 0; j < ASG_REG_HITS; ++j) {
                src[j] = tr + (uint64_t)a.col[b + (j < L ? j : 0)] * a.stride;
                A[j] = 0.0;
            }
            for (uint32_t blk = 0; blk < nb; ++blk) {
                const uint32_t s = blk * ASG_LANES + lane;
                if (s < a.count) {
                    double v[ASG_REG_HITS];
#pragma unroll
                    for (uint32_t j = 0; j < ASG_REG_HITS; ++j) v[j] = j < L ? src[j][s] : 0.0;
                    double D = 0.0;
#pragma unroll
                    for (uint32_t j = 0; j < ASG_REG_HITS; ++j) if (j < L) D = D + v[j];
                    const bool ok = D > 0.0 && D < __builtin_inf();
                    const double rr = 1.0 / (ok ? D : 1.0);
#pragma unroll
                    for (uint32_t j = 0; j < ASG_REG_HITS; ++j) A[j] = A[j] + (ok ? v[j] * rr : flat);
                }
            }
#pragma unroll
            for (uint32_t j = 0; j < ASG_REG_HITS; ++j) {
                if (j < L) {                       // (L is the wave's: every lane takes part in the fold)
                    const double sum = lane_fold(A[j]);
                    if (lane == 0) a.P[b + j] = sum / div;
                }
            }
        } else {
            // first walk: per sample the reciprocal of the row's sum into the wave's slice (-1: the degenerate case)
            for (uint32_t blk = 0; blk < nb; ++blk) {
                const uint32_t s = blk * ASG_LANES + lane;
                if (s < a.count) {
                    double D = 0.0;
                    for (uint64_t j = b; j < e; ++j) D = D + tr[(uint64_t)a.col[j] * a.stride + s];
                    const bool ok = D > 0.0 && D < __builtin_inf();
                    rs[s] = ok ? 1.0 / D : -1.0;
                }
            }
            // second walk, hit by hit: its trace row streamed once, a lane's samples added in ascending order.  A lane reads back
            // only what it wrote itself.
            for (uint64_t j = b; j < e; ++j) {
                const double *const src = tr + (uint64_t)a.col[j] * a.stride;
                double A = 0.0;
                for (uint32_t blk = 0; blk < nb; ++blk) {
                    const uint32_t s = blk * ASG_LANES + lane;
                    if (s < a.count) {
                        const double rr = rs[s];
                        A = A + (rr < 0.0 ? flat : src[s] * rr);
                    }
                }
                const double sum = lane_fold(A);
                if (lane == 0) a.P[j] = sum / div;
            }
        }
    }
}

} // namespace mmg
