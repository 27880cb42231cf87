// sim_kernels.h -- posterior distances and correlations between S samples from their joint draws (mmg_sim_*).  Draw t of every sample
// together is one draw of all S expression profiles; per draw the Gram matrix of the S profiles over the used features gives every
// pairwise distance and correlation.  Specification: tests/sim_ref.py, DESIGN.md section 17.
//
// The values live as z[s][t][f] (the trace files' layout per sample), so the feature axis is contiguous in every row of every draw.
//   k_sim_prepare  one sample in place: the check (before the logarithm), x = dlog(v) or v, z = ((x + off) - c[f]) + 0.0; an invalid
//                  value stores 0.0 and marks bad[s][f] (plain byte stores of the one value 1)
//   k_sim_used     used[f] = mask[f] && no sample marked f; the row of ones (1.0 used, 0.0 not); the count of used features (integer add)
//   k_sim_zero     z = 0.0 at the unused features, so that they contribute nothing anywhere
//   k_sim_gram     the hot path, on the matrix cores: per (draw, chunk of features, 64 x 64 block of the upper triangle) the partial
//                  Gram tiles of the S + 1 rows (the ones appended as row S: the products with it are m, its own is n), rows padded
//                  with zeros to a multiple of 16.  A wave owns one row of 16 x 16 tiles of the block; v_mfma_f64_16x16x4_f64 takes
//                  A[i = lane & 15][k = lane >> 4] and B[k = lane >> 4][j = lane & 15], one double per lane each.  A Gram matrix sums
//                  over k in any order as long as both operands agree on it, so lane (i, h) streams the contiguous run
//                  [c0 + h L, c0 + (h + 1) L) of its own row straight from global memory and feeds element j at step j (L = a
//                  quarter of the chunk, rounded up; past the chunk's end a lane feeds 0.0): no LDS, no transpose.  On a diagonal
//                  tile A and B are the same registers.  D[row = (lane >> 4) + 4 reg][col = lane & 15] is stored as it lies in the
//                  registers, 256 doubles per tile
//   k_sim_reduce   adds the chunks of a tile in ascending order from 0.0 and writes G (both triangles), m and n
//   k_sim_pair     one workgroup per pair r < s: D[t] and R[t] of the T draws in LDS, the moments in the fixed lane order of
//                  lane_sum (pairs_ref.lsum), a bitonic sort of each, the order statistics at the ranks
//   k_sim_nn       one thread per (a, t): the nearest other sample by the D^2 numerator, ties to the smallest index; integer adds
// No floating-point atomics, no private memory: reruns are bit-identical.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "mmg_series.h"

namespace mmg {

constexpr uint32_t SIM_MAX_S = 256;
constexpr uint32_t SIM_MAX_T = 4096;       // draws at most: 2 x 4096 words = 64 KiB of LDS in k_sim_pair
constexpr uint32_t SIM_MAX_RANKS = 64;
constexpr uint32_t SIM_TILE = 16;          // the MFMA's tile
constexpr uint32_t SIM_BT = 4;             // tiles per side of a workgroup's block: 64 x 64, one wave per tile row
constexpr uint32_t SIM_TILE_WORDS = SIM_TILE * SIM_TILE;
enum : uint8_t { SIM_FEW_FEATURES = 1, SIM_PAIR_NO_R = 2 };

constexpr uint32_t SIM_PAIR_BLOCK = 256;

typedef double sim_acc __attribute__((ext_vector_type(4)));

// tiles (ti <= tj) of an NT x NT upper triangle in row-major order: the index of (ti, tj), and back
__host__ __device__ __forceinline__ uint32_t sim_ut_index(uint32_t NT, uint32_t ti, uint32_t tj)
{
    return ti * NT - ti * (ti - 1) / 2 + (tj - ti);
}
__host__ __device__ __forceinline__ void sim_ut_decode(uint32_t NT, uint32_t idx, uint32_t &ti, uint32_t &tj)
{
    ti = 0;
    while (idx >= NT - ti) { idx -= NT - ti; ++ti; }
    tj = ti + idx;
}

// Sample s, draw t = blockIdx.y < T, feature f < F: z = the sample's [T][F] block, bad = the sample's [F] bytes (zeroed before).
__global__ __launch_bounds__(256) void k_sim_prepare(uint32_t F, double *__restrict__ z, double off, const double *__restrict__ centre, uint32_t logged,
                                                     uint8_t *__restrict__ bad)
{
    const uint64_t f = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= F) return;
    double *const p = z + (uint64_t)blockIdx.y * F + f;
    const double v = *p;
    const bool ok = logged ? dabs(v) <= 0x1.fffffffffffffp+1023 : (v > 0.0 && v <= 0x1.fffffffffffffp+1023);
    if (!ok) {
        *p = 0.0;
        bad[f] = 1;
        return;
    }
    const double x = logged ? v : dlog(v);
    *p = ((x + off) - centre[f]) + 0.0;
}

__global__ __launch_bounds__(256) void k_sim_used(uint32_t F, uint32_t S, const uint8_t *__restrict__ mask, const uint8_t *__restrict__ bad,
                                                  uint8_t *__restrict__ used, double *__restrict__ ones, unsigned long long *__restrict__ count)
{
    const uint64_t f = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t u = 0;
    if (f < F) {
        u = mask[f] != 0;
        for (uint32_t s = 0; s < S && u; ++s) u = bad[(uint64_t)s * F + f] == 0;
        used[f] = (uint8_t)u;
        ones[f] = u ? 1.0 : 0.0;
    }
    const unsigned long long b = __ballot(u != 0);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(count, (unsigned long long)__popcll(b));
}

// rows [64 blockIdx.y, ...) of the S T rows of z, feature f: zero where f is not used
__global__ __launch_bounds__(256) void k_sim_zero(uint32_t F, uint32_t rows, const uint8_t *__restrict__ used, double *__restrict__ z)
{
    const uint64_t f = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (f >= F || used[f]) return;
    const uint32_t r0 = blockIdx.y * 64, r1 = r0 + 64 < rows ? r0 + 64 : rows;
    for (uint32_t r = r0; r < r1; ++r) z[(uint64_t)r * F + f] = 0.0;
}

// grid (blocks of the upper triangle, chunks, T) x 256 threads.  NT = ceil((S + 1) / 16) tiles per side, NB = ceil(NT / 4) blocks per
// side, CH features per chunk; part[((t * chunks + c) * NT (NT + 1) / 2 + sim_ut_index(ti, tj)) * 256 + reg * 64 + lane].
__global__ __launch_bounds__(256) void k_sim_gram(uint32_t S, uint32_t T, uint32_t F, uint32_t NT, uint32_t NB, uint32_t CH, const double *__restrict__ z,
                                                  const double *__restrict__ ones, double *__restrict__ part)
{
    const uint32_t lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // (w in a scalar: the tile tests below branch)
    uint32_t bi, bj;
    sim_ut_decode(NB, blockIdx.x, bi, bj);
    const uint32_t ti = SIM_BT * bi + w;
    if (ti >= NT) return;   // (the whole wave)
    const uint32_t t = blockIdx.z, c = blockIdx.y;
    const uint32_t c0 = c * CH, c1 = F - c0 < CH ? F : c0 + CH;   // c0 < F: the launch has ceil(F / CH) chunks
    const uint32_t L = (c1 - c0 + 3) / 4;
    const uint32_t i = lane & 15, h = lane >> 4;
    const uint64_t start = (uint64_t)c0 + (uint64_t)h * L;
    const uint32_t own = start < c1 ? (c1 - (uint32_t)start < L ? c1 - (uint32_t)start : L) : 0;   // this lane's run, cut at the chunk's end

    // row r of the S + 1: sample r's draw t, the ones, or a padding row of zeros (no run)
    const uint32_t ra = ti * SIM_TILE + i;
    const double *const pa = (ra < S ? z + ((uint64_t)ra * T + t) * F : ones) + start;
    const uint32_t own_a = ra <= S ? own : 0;
    const double *pb[SIM_BT];
    uint32_t own_b[SIM_BT];
    bool act[SIM_BT];
    sim_acc acc[SIM_BT];
#pragma unroll
    for (uint32_t q = 0; q < SIM_BT; ++q) {
        const uint32_t tj = SIM_BT * bj + q, rb = tj * SIM_TILE + i;
        act[q] = tj < NT && tj >= ti;   // (the same in every lane)
        pb[q] = (rb < S ? z + ((uint64_t)rb * T + t) * F : ones) + start;
        own_b[q] = act[q] && rb <= S ? own : 0;
        acc[q] = sim_acc{0.0, 0.0, 0.0, 0.0};
    }
    for (uint32_t j = 0; j < L; j += 4) {   // four steps' loads in flight; the steps past L feed zeros
        double a[4];
#pragma unroll
        for (uint32_t u = 0; u < 4; ++u) a[u] = j + u < own_a ? pa[j + u] : 0.0;
#pragma unroll
        for (uint32_t q = 0; q < SIM_BT; ++q) {
            if (!act[q]) continue;
            double b[4];
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u) b[u] = SIM_BT * bj + q == ti ? a[u] : (j + u < own_b[q] ? pb[q][j + u] : 0.0);
#pragma unroll
            for (uint32_t u = 0; u < 4; ++u) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[u], b[u], acc[q], 0, 0, 0);
        }
    }
    const uint32_t n_ut = NT * (NT + 1) / 2;
    double *const out = part + ((uint64_t)t * gridDim.y + c) * n_ut * SIM_TILE_WORDS;
#pragma unroll
    for (uint32_t q = 0; q < SIM_BT; ++q) {
        if (!act[q]) continue;
        double *const o = out + (uint64_t)sim_ut_index(NT, ti, SIM_BT * bj + q) * SIM_TILE_WORDS;
        o[lane] = acc[q][0]; o[64 + lane] = acc[q][1]; o[128 + lane] = acc[q][2]; o[192 + lane] = acc[q][3];
    }
}

// grid (tiles of the upper triangle, T) x 256 threads: thread e holds register e >> 6 of lane e & 63 of the tile
__global__ __launch_bounds__(256) void k_sim_reduce(uint32_t S, uint32_t NT, uint32_t chunks, const double *__restrict__ part, double *__restrict__ G,
                                                    double *__restrict__ m, double *__restrict__ n)
{
    const uint32_t e = threadIdx.x, lane = e & 63, reg = e >> 6, t = blockIdx.y;
    uint32_t ti, tj;
    sim_ut_decode(NT, blockIdx.x, ti, tj);
    const uint32_t n_ut = NT * (NT + 1) / 2;
    const double *p = part + ((uint64_t)t * chunks * n_ut + blockIdx.x) * SIM_TILE_WORDS + e;
    double v = 0.0;
    for (uint32_t c = 0; c < chunks; ++c) v = v + p[(uint64_t)c * n_ut * SIM_TILE_WORDS];
    const uint32_t r = ti * SIM_TILE + (lane >> 4) + 4 * reg, s = tj * SIM_TILE + (lane & 15);
    if (r < S && s < S) {
        G[((uint64_t)t * S + r) * S + s] = v;
        if (ti != tj) G[((uint64_t)t * S + s) * S + r] = v;
    } else if (r < S && s == S) m[(uint64_t)t * S + r] = v;
    else if (r == S && s == S) n[t] = v;
}

struct SimOut {
    double *mean_D, *ss_D, *mean_R, *ss_R;   // [pairs]
    double *q_D, *q_R;                       // [pairs][nr]
    uint8_t *pair_status;                    // [pairs]
};

// Pair p = blockIdx.x of the S (S - 1) / 2 pairs r < s, r-major; P >= T a power of two, 16 P bytes of dynamic LDS; n >= 2 the used
// features; ranks[nr] zero-based, a rank >= T gives NaN.
__global__ __launch_bounds__(SIM_PAIR_BLOCK) void k_sim_pair(uint32_t S, uint32_t T, uint32_t P, double n, const double *__restrict__ G,
                                                         const double *__restrict__ m, uint32_t nr, const uint32_t *__restrict__ ranks, SimOut o)
{
    extern __shared__ uint64_t sim_lds[];
    __shared__ uint32_t sh_bad;
    uint64_t *const kd = sim_lds, *const kr = sim_lds + P;
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t p = blockIdx.x;
    uint32_t r = 0, s = p;
    while (s >= S - 1 - r) { s -= S - 1 - r; ++r; }
    s += r + 1;
    const double nan = __builtin_nan("");

    if (tid == 0) sh_bad = 0;
    __syncthreads();
    uint32_t bad = 0;
    for (uint32_t t = tid; t < T; t += SIM_PAIR_BLOCK) {
        const double *const g = G + (uint64_t)t * S * S;
        const double grr = g[(uint64_t)r * S + r], gss = g[(uint64_t)s * S + s], grs = g[(uint64_t)r * S + s];
        const double mr = m[(uint64_t)t * S + r], ms = m[(uint64_t)t * S + s];
        const double num = (grr + gss) - 2.0 * grs;
        kd[t] = bits_of(dsqrt((num < 0.0 ? 0.0 : num) / n) + 0.0);
        const double va = grr - mr * mr / n, vb = gss - ms * ms / n;
        const double R = (grs - mr * ms / n) / dsqrt(va * vb);
        if (!(va > 0.0) || !(vb > 0.0) || !(dabs(R) <= 0x1.fffffffffffffp+1023)) bad = 1;
        kr[t] = bits_of(R + 0.0);
    }
    if (bad) atomicOr(&sh_bad, bad);
    __syncthreads();
    bad = sh_bad;   // (the same in every thread)

    // ---- moments over the draws in their order: wave 0 the distances, wave 1 the correlations
    if (w < 2) {
        const uint64_t *const x = w ? kr : kd;
        double mean = nan, ss = nan;
        if (!(w && bad)) {
            double a = 0.0;
            for (uint32_t t = lane; t < T; t += 64) a = a + double_of(x[t]);
            mean = lane_sum(a) / (double)T;
            double q = 0.0;
            for (uint32_t t = lane; t < T; t += 64) { const double d = double_of(x[t]) - mean; q = q + d * d; }
            ss = lane_sum(q);
        }
        if (lane == 0) {
            if (w) { o.mean_R[p] = mean; o.ss_R[p] = ss; }
            else { o.mean_D[p] = mean; o.ss_D[p] = ss; o.pair_status[p] = bad ? SIM_PAIR_NO_R : 0; }
        }
    }
    __syncthreads();

    // ---- order statistics: both series sorted by key, the padding above every key
    for (uint32_t t = tid; t < P; t += SIM_PAIR_BLOCK) {
        kd[t] = t < T ? order_key(double_of(kd[t])) : ~0ull;
        kr[t] = t < T ? order_key(double_of(kr[t])) : ~0ull;
    }
    __syncthreads();
    block_sort<SIM_PAIR_BLOCK>(kd, P);
    if (!bad) block_sort<SIM_PAIR_BLOCK>(kr, P);
    for (uint32_t k = tid; k < nr; k += SIM_PAIR_BLOCK) {
        const uint32_t rk = ranks[k];
        o.q_D[(uint64_t)p * nr + k] = rk < T ? order_unkey(kd[rk]) : nan;
        o.q_R[(uint64_t)p * nr + k] = rk < T && !bad ? order_unkey(kr[rk]) : nan;
    }
}

// thread a * T + t: the b != a with the smallest (G_aa + G_bb) - 2 G_ab of draw t, the first of equals; nn[a * S + b] counts the draws
__global__ __launch_bounds__(256) void k_sim_nn(uint32_t S, uint32_t T, const double *__restrict__ G, uint32_t *__restrict__ nn)
{
    const uint32_t idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= S * T) return;
    const uint32_t a = idx / T, t = idx - a * T;
    const double *const g = G + (uint64_t)t * S * S;
    const double gaa = g[(uint64_t)a * S + a];
    uint32_t best = a ? 0 : 1;
    double dbest = (gaa + g[(uint64_t)best * S + best]) - 2.0 * g[(uint64_t)a * S + best];
    for (uint32_t b = best + 1; b < S; ++b) {
        if (b == a) continue;
        const double d = (gaa + g[(uint64_t)b * S + b]) - 2.0 * g[(uint64_t)a * S + b];
        if (d < dbest) { dbest = d; best = b; }
    }
    atomicAdd(&nn[a * S + best], 1u);
}

} // namespace mmg
