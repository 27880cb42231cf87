// diff_effects_kernels.h -- mmdiff's effect summaries (mmg_diff_effects_summarize, mmg_effects_of_rows): from the thinned rows that
// k_df_run_traced records, rows[S][P][F] with gamma as parameter P - 1, per parameter and feature the mean, the standard deviation,
// the number of positive draws and order statistics of the draws under the parameter's own model.  Specification:
// tests/mmdiff_effects_ref.py, DESIGN.md section 10.3.
//
// The draws of parameter s (of model m = model_of[s]) for feature f are the rows whose own gamma equals m, in row order.  A series is
// strided by P F 8 bytes, so a workgroup does not take one series: it takes one parameter and a tile of FX_TILE = 8 consecutive
// features, and the eight lanes that read a row of the tile read one 64-byte piece of it (aligned when F is a multiple of 8).
//   1. load      FX_CHUNK rows of the tile and of its gamma tile go to LDS (lane = (row, feature): a wave reads 8 rows x 64 bytes)
//   2. compact   a wave per series, lane = row: ballot of "gamma == m", the prefix count below the lane is the draw's place behind the
//                series' count so far (a register of the wave: no atomics, row order kept).  The draw is stored as its sort key, which
//                is a bijection of the bits.  The same ballots count the draws > 0 and (parameter 0's workgroups) the rows of model 1.
//   3. moments   one lane per series walks its draws in row order: sum / n, then the squared deviations from that mean (two passes)
//   4. sort      the keys are padded with ~0 to a power of two and sorted by the whole workgroup: the bitonic network and the keys
//                of mmg_series.h (block_sort, order_key), all series of the workgroup side by side
//   5. pick      q[j] = the sorted draw at floor(percentiles[j] / 100 * (n - 1) + 0.5)
// KEYS is the power of two of keys a series has room for in LDS (S <= KEYS), NSER the series a workgroup sorts: 8 up to 2048 keys.  At
// 4096 keys eight series would take 256 KiB, more than a CU has, so NSER = 4 and the tile is shared by two workgroups (blockIdx.z),
// each still loading whole 64-byte pieces.  Sums are sequential, there is no floating-point atomic: reruns are bit-identical.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mmg_series.h"

namespace mmg {

constexpr uint32_t FX_TILE = 8;        // features per tile: 64 bytes of a row
constexpr uint32_t FX_BLOCK = 256;
constexpr uint32_t FX_CHUNK = 128;     // rows staged at a time (with 1024 keys a series, two workgroups fit a CU)
constexpr uint32_t FX_SMAX = 4096;     // keys per series at most
constexpr uint32_t FX_NPMAX = 32;

struct EffectsOut {
    uint32_t *n;       // [2][F]
    double *mean, *sd; // [P - 1][F]
    uint32_t *n_gt;    // [P - 1][F]
    double *q;         // [P - 1][np][F]
};

// grid (ceil(F / 8), P - 1, 8 / NSER), FX_BLOCK threads
template <uint32_t KEYS, uint32_t NSER>
__global__ __launch_bounds__(FX_BLOCK) void k_df_effects(uint32_t S, uint32_t P, uint32_t F, const double *__restrict__ rows,
                                                         const uint8_t *__restrict__ model_of, uint32_t np,
                                                         const double *__restrict__ pct, EffectsOut o)
{
    static_assert(NSER == 4 || NSER == 8, "a wave compacts NSER / 4 series");
    constexpr uint32_t PER_WAVE = NSER / 4;
    __shared__ uint64_t s_key[NSER][KEYS];
    __shared__ double s_x[FX_TILE][FX_CHUNK];
    __shared__ uint8_t s_g[FX_TILE][FX_CHUNK];
    __shared__ uint32_t s_n[NSER];

    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t s = blockIdx.y, f0 = blockIdx.x * FX_TILE, j0 = blockIdx.z * NSER;   // series j0 .. j0 + NSER - 1 of the tile
    const uint32_t m = model_of[s];
    const size_t PF = (size_t)P * F;
    const uint64_t below = (1ull << lane) - 1;

    uint32_t cnt[PER_WAVE], gt[PER_WAVE], ones[PER_WAVE];
    for (uint32_t u = 0; u < PER_WAVE; ++u) cnt[u] = gt[u] = ones[u] = 0;

    for (uint32_t c0 = 0; c0 < S; c0 += FX_CHUNK) {
        // 1. load: thread = (row rr of 32, feature j of 8)
        {
            const uint32_t j = tid & 7, rr = tid >> 3, f = f0 + j;
            for (uint32_t it = 0; it < FX_CHUNK / 32; ++it) {
                const uint32_t i = it * 32 + rr, r = c0 + i;
                double x = 0.0, g = 0.0;
                if (r < S && f < F) {
                    const double *row = rows + (size_t)r * PF + f;
                    x = row[(size_t)s * F];
                    g = row[(size_t)(P - 1) * F];
                }
                s_x[j][i] = x;
                s_g[j][i] = g == 1.0 ? 1 : 0;
            }
        }
        __syncthreads();
        // 2. compact: wave = series, lane = row
        for (uint32_t u = 0; u < PER_WAVE; ++u) {
            const uint32_t jl = wave + 4 * u, j = j0 + jl;
            for (uint32_t i0 = 0; i0 < FX_CHUNK; i0 += 64) {
                const uint32_t i = i0 + lane;
                const bool live = c0 + i < S && f0 + j < F;
                const double x = s_x[j][i];
                const uint32_t g = s_g[j][i];
                const bool keep = live && g == m;
                const uint64_t mask = __ballot(keep);
                if (keep) s_key[jl][cnt[u] + (uint32_t)__popcll(mask & below)] = order_key(x);   // cnt + prefix < n <= S <= KEYS
                cnt[u] += (uint32_t)__popcll(mask);
                gt[u] += (uint32_t)__popcll(__ballot(keep && x > 0.0));
                ones[u] += (uint32_t)__popcll(__ballot(live && g == 1));
            }
        }
        __syncthreads();   // the stage is free for the next chunk; after the last one, every key is in place
    }

    // 3. moments: lane u of a wave walks series wave + 4 u in row order
    if (lane < PER_WAVE) {
        uint32_t n = 0, ng = 0, n1 = 0;
        for (uint32_t u = 0; u < PER_WAVE; ++u)
            if (u == lane) { n = cnt[u]; ng = gt[u]; n1 = ones[u]; }
        const uint32_t jl = wave + 4 * lane, f = f0 + j0 + jl;
        s_n[jl] = n;
        if (f < F) {
            const uint64_t *k = s_key[jl];
            double sum = 0.0;
            for (uint32_t i = 0; i < n; ++i) sum += order_unkey(k[i]);
            const double mean = sum / (double)n;   // 0 / 0 for n = 0: NaN
            double ss = 0.0;
            for (uint32_t i = 0; i < n; ++i) {
                const double dx = order_unkey(k[i]) - mean;
                ss += dx * dx;
            }
            const size_t at = (size_t)s * F + f;
            o.mean[at] = n ? mean : __builtin_nan("");
            o.sd[at] = n > 1 ? dsqrt(ss / (double)(n - 1)) : __builtin_nan("");
            o.n_gt[at] = ng;
            if (s == 0) { o.n[f] = S - n1; o.n[(size_t)F + f] = n1; }
        }
    }
    __syncthreads();

    // 4. sort NSER series of SP keys each, SP the power of two that holds the longest of them
    uint32_t nmax = 0;
    for (uint32_t jl = 0; jl < NSER; ++jl) nmax = s_n[jl] > nmax ? s_n[jl] : nmax;
    uint32_t lg = 0;
    while ((1u << lg) < nmax) ++lg;
    const uint32_t SP = 1u << lg;   // <= KEYS
    for (uint32_t e = tid; e < NSER * SP; e += FX_BLOCK) {
        const uint32_t jl = e >> lg, i = e & (SP - 1);
        if (i >= s_n[jl]) s_key[jl][i] = ~0ull;   // padding sorts last
    }
    __syncthreads();
    for (uint32_t k = 2; k <= SP; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t e = tid; e < NSER * SP; e += FX_BLOCK) {
                const uint32_t jl = e >> lg, i = e & (SP - 1), l = i ^ j;
                if (l > i) {
                    const uint64_t a = s_key[jl][i], b = s_key[jl][l];
                    const bool up = (i & k) == 0;
                    if ((a > b) == up) { s_key[jl][i] = b; s_key[jl][l] = a; }
                }
            }
            __syncthreads();
        }

    // 5. pick
    for (uint32_t e = tid; e < NSER * np; e += FX_BLOCK) {
        const uint32_t jq = e / NSER, jl = e - jq * NSER, f = f0 + j0 + jl, n = s_n[jl];
        if (f >= F) continue;
        double v = __builtin_nan("");
        if (n) {
            uint32_t idx = (uint32_t)__builtin_floor(pct[jq] / 100.0 * (double)(n - 1) + 0.5);
            idx = idx < n ? idx : n - 1;
            v = order_unkey(s_key[jl][idx]);
        }
        o.q[((size_t)s * np + jq) * F + f] = v;
    }
}

} // namespace mmg
