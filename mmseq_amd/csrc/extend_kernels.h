// extend_kernels.h -- the two kernels of mmg_sampler_extend: a finished run of length L becomes the first half of a run
// of length 2 L.  The samples a run of 2 L keeps are every second one of the run of L, so the even rows of the resident trace move to
// its front and the two moment sums are added up again from them, in sample order, as k_update (misc_kernels.h) would have.
#pragma once
#include "mmg_types.h"
#include "mmg_math.h"

namespace mmg {

// dst row j = src row j * src_step for j < rows_copy, +0.0 for rows_copy <= j < rows_total; rows of n doubles, densely packed on both
// sides, dst and src distinct buffers.  mmg_sampler_extend moves a chain in two launches through a scratch buffer: the even rows into
// the scratch (src_step 2, rows_copy == rows_total == S / 2), then the scratch back to the front of the trace with zeros behind it
// (src_step 1, rows_copy S / 2, rows_total S) -- no launch reads a row that it or a concurrent workgroup writes.
// A row starts at 8 n j bytes: for odd n only every other row is 16-byte aligned.  A lane moves the 16-byte-aligned pair of the
// DESTINATION row it owns (one 16-byte store; one 16-byte load when the source pair is aligned too, which it is in the second launch
// and in every launch for even n, two 8-byte loads otherwise); the lane behind the last pair moves the row's unaligned first and
// last element.  grid.x covers the pairs of a row plus that lane, grid.y strides over the rows.
__global__ __launch_bounds__(256) void k_trace_halve(double *__restrict__ dst, const double *__restrict__ src, uint32_t n, uint32_t rows_copy,
                                                     uint32_t rows_total, uint32_t src_step)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    for (uint32_t row = blockIdx.y; row < rows_total; row += gridDim.y) { // (uniform)
        double *d = dst + (uint64_t)row * n;
        const uint32_t head = (uint32_t)(((uintptr_t)d >> 3) & 1u);      // elements in front of the first aligned pair
        const uint32_t pairs = (n - head) >> 1, tail = (n - head) & 1u;  // n >= 1 >= head
        if (row < rows_copy) {
            const double *s = src + (uint64_t)row * src_step * n;
            if (i < pairs) {
                const uint32_t e = head + 2u * i;                        // e + 1 <= head + 2 pairs - 1 <= n - 1
                double2 v;
                if ((((uintptr_t)(s + e)) & 15u) == 0) v = *reinterpret_cast<const double2 *>(s + e); // (uniform over a row)
                else { v.x = s[e]; v.y = s[e + 1]; }
                *reinterpret_cast<double2 *>(d + e) = v;
            } else if (i == pairs) {
                if (head) d[0] = s[0];
                if (tail) d[n - 1] = s[n - 1];
            }
        } else {
            if (i < pairs) *reinterpret_cast<double2 *>(d + head + 2u * i) = double2{0.0, 0.0};
            else if (i == pairs) {
                if (head) d[0] = 0.0;
                if (tail) d[n - 1] = 0.0;
            }
        }
    }
}

// One lane per (chain, device transcript): the moment sums of the first `rows` rows of the chain's trace [S][n], added in ascending
// sample order exactly as k_update adds them (sum = sum + lg, sum2 = sum2 + lg * lg from +0.0, every operation rounded once), into
// k_update's places: sum_log[c n + t], sum_log2[c n + t].  Lanes read adjacent words of a row; no atomics.
__global__ __launch_bounds__(256) void k_moments_rebuild(const double *__restrict__ trace, double *__restrict__ sum_log, double *__restrict__ sum_log2,
                                                         uint32_t n, uint32_t S, uint32_t rows)
{
    const uint32_t c = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    const double *x = trace + (uint64_t)c * S * n + t;
    double sl = 0.0, sl2 = 0.0;
    uint32_t s = 0;
    for (; s + 4 <= rows; s += 4) { // four loads in flight per lane: the sums are one dependent chain
        const double m0 = x[(uint64_t)s * n], m1 = x[(uint64_t)(s + 1) * n], m2 = x[(uint64_t)(s + 2) * n], m3 = x[(uint64_t)(s + 3) * n];
        const double l0 = dlog(m0), l1 = dlog(m1), l2 = dlog(m2), l3 = dlog(m3);
        sl = sl + l0; sl2 = sl2 + l0 * l0;
        sl = sl + l1; sl2 = sl2 + l1 * l1;
        sl = sl + l2; sl2 = sl2 + l2 * l2;
        sl = sl + l3; sl2 = sl2 + l3 * l3;
    }
    for (; s < rows; ++s) {
        const double lg = dlog(x[(uint64_t)s * n]);
        sl = sl + lg;
        sl2 = sl2 + lg * lg;
    }
    const uint64_t gid = (uint64_t)c * n + t;
    sum_log[gid] = sl;
    sum_log2[gid] = sl2;
}

} // namespace mmg
