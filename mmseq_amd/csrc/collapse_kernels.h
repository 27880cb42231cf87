// collapse_kernels.h -- mmcollapse on the device (src/mmcollapse.cpp:483-561 covariances and mean correlations, :713-747 the
// threshold's row maxima, :758-819 with collapse() at :398-441 the greedy loop).
//
// Storage, per handle: the centred candidate traces X[s][k][Cp] of every sample s (k over the N trace rows, the candidate index
// contiguous, C rounded up to Cp = a multiple of CT with zero columns), the column variances var[s][Cp], the observed mask
// obs[s][Cp], and the mean-correlation matrix V[Cp][Cp] -- O(Cp^2 + S N Cp) doubles, where the reference keeps the C x C x S cube
// of covariances.  A merged candidate's trace is the sum of its members' centred traces, so its covariances are what collapse()'s
// additions compute; they are recomputed from the summed trace rather than kept per sample.
//
// Every sum runs in a fixed order (k ascending with fma, samples ascending) and nothing uses floating-point atomics: reruns are
// bit-identical.  V is symmetric by construction: both entries of a pair are written with one value.
//
// The greedy loop keeps, per column j, the minimum of V(:, j) skipping NaNs and the first row that attains it (Armadillo's
// column-major min: over the columns, the smallest value, ties to the lower column, then the lower row).  After a merge of b into
// a < b only column a, the columns whose minimum sat in row a or b, and nothing else need a rescan; the others compare one new
// entry, V(a, j).
#pragma once
#include "mmg_types.h"
#include "mmg_math.h"

namespace mmg {

constexpr uint32_t CL_CT = 64;        // edge of a V tile; Cp is a multiple of it
constexpr uint32_t CL_KT = 16;        // trace rows per LDS step of the tile product; N is a multiple of it
constexpr uint32_t CL_NONE = 0xffffffffu;

// column means removed, column by column: mean = (sum over k ascending) / N (one thread per column of one sample)
__global__ __launch_bounds__(256) void k_cl_center(uint32_t N, uint32_t Cp, uint32_t C, double *__restrict__ X)
{
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= C) return;
    double s = 0.0;
    for (uint32_t k = 0; k < N; ++k) s += X[(uint64_t)k * Cp + j];
    const double m = s / (double)N;
    for (uint32_t k = 0; k < N; ++k) X[(uint64_t)k * Cp + j] -= m;
}

// var[j] = sum_k x_kj^2 / (N - 1), fma in k order (the diagonal of the tile product, bit for bit); non-finite -> 0 (:556-559)
__global__ __launch_bounds__(256) void k_cl_var(uint32_t N, uint32_t Cp, const double *__restrict__ X, double *__restrict__ var)
{
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= Cp) return;
    double acc = 0.0;
    for (uint32_t k = 0; k < N; ++k) { const double x = X[(uint64_t)k * Cp + j]; acc = __builtin_fma(x, x, acc); }
    double v = acc / (double)(N - 1);
    if (!__builtin_isfinite(v)) v = 0.0;
    var[j] = v;
}

// The mean correlations of one CT x CT tile of V, for every sample in turn (:514-561 then :483-512 with SDPENALTY = 0):
//   cov = X_i . X_j / (N - 1) (non-finite -> 0), r = cov / sqrt(var_hi) / sqrt(var_lo) (hi / lo: the larger / smaller of i, j --
//   the order of the reference's last write to the pair), r = 0 where the pair is not observed in both, V = sum_s r / sum_s u.
// Only tiles with bj >= bi run; each writes its block and the mirror block.  256 threads, 4 x 4 entries each (rows ty + 16 r,
// columns tx + 16 c), the two KT x CT panels of the trace in LDS.
__global__ __launch_bounds__(256) void k_cl_corr_tiles(uint32_t N, uint32_t Cp, uint32_t S, const double *__restrict__ X,
                                                       const double *__restrict__ var, const uint8_t *__restrict__ obs,
                                                       double *__restrict__ V)
{
    const uint32_t bi = blockIdx.y, bj = blockIdx.x;
    if (bj < bi) return;
    __shared__ double As[CL_KT][CL_CT], Bs[CL_KT][CL_CT];
    const uint32_t tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const uint32_t i0 = bi * CL_CT, j0 = bj * CL_CT;
    double vs[4][4];
    uint32_t cnt[4][4];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) { vs[r][c] = 0.0; cnt[r][c] = 0; }
    for (uint32_t s = 0; s < S; ++s) {
        const double *Xs = X + (uint64_t)s * N * Cp;
        double acc[4][4];
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) acc[r][c] = 0.0;
        for (uint32_t k0 = 0; k0 < N; k0 += CL_KT) {
            for (uint32_t q = 0; q < 4; ++q) {
                const uint32_t e = tid + 256 * q, kk = e >> 6, c = e & 63;
                As[kk][c] = Xs[(uint64_t)(k0 + kk) * Cp + i0 + c];
                Bs[kk][c] = Xs[(uint64_t)(k0 + kk) * Cp + j0 + c];
            }
            __syncthreads();
#pragma unroll 4
            for (uint32_t kk = 0; kk < CL_KT; ++kk) {
                double a[4], b[4];
                for (int r = 0; r < 4; ++r) a[r] = As[kk][ty + 16 * r];
                for (int c = 0; c < 4; ++c) b[c] = Bs[kk][tx + 16 * c];
                for (int r = 0; r < 4; ++r)
                    for (int c = 0; c < 4; ++c) acc[r][c] = __builtin_fma(a[r], b[c], acc[r][c]);
            }
            __syncthreads();
        }
        const double *vr = var + (uint64_t)s * Cp;
        const uint8_t *ob = obs + (uint64_t)s * Cp;
        for (int r = 0; r < 4; ++r)
            for (int c = 0; c < 4; ++c) {
                const uint32_t i = i0 + ty + 16 * r, j = j0 + tx + 16 * c;
                const uint32_t lo = i < j ? i : j, hi = i < j ? j : i;
                double cv = acc[r][c] / (double)(N - 1);
                if (!__builtin_isfinite(cv)) cv = 0.0;
                double rr = cv / __builtin_sqrt(vr[hi]) / __builtin_sqrt(vr[lo]);
                const uint32_t u = (ob[i] & ob[j]) ? 1u : 0u;
                if (!u) rr = 0.0;
                vs[r][c] += rr;
                cnt[r][c] += u;
            }
    }
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) {
            const uint32_t i = i0 + ty + 16 * r, j = j0 + tx + 16 * c;
            const double v = vs[r][c] / (double)cnt[r][c];
            V[(uint64_t)i * Cp + j] = v;
            V[(uint64_t)j * Cp + i] = v;
        }
}

// lexicographic (value, index) minimum, NaN values and CL_NONE indices never win
__device__ __forceinline__ void cl_min_into(double &bv, uint32_t &bi, double v, uint32_t i)
{
    if (i == CL_NONE || !(v == v)) return;
    if (bi == CL_NONE || v < bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

// one workgroup per row j < C (= column j, V is symmetric): the minimum of the column and its first row (flagged columns only when
// flag != nullptr), and with rowmax != nullptr the off-diagonal maximum of the row starting from -1, NaN skipped (:719-730)
__global__ __launch_bounds__(256) void k_cl_scan(uint32_t C, uint32_t Cp, const double *__restrict__ V, uint8_t *__restrict__ flag,
                                                 double *__restrict__ cmin, uint32_t *__restrict__ carg, double *__restrict__ rowmax)
{
    const uint32_t j = blockIdx.x, tid = threadIdx.x;
    if (j >= C) return;
    if (flag && !flag[j]) return;
    __shared__ double s_v[256], s_m[256];
    __shared__ uint32_t s_i[256];
    const double *row = V + (uint64_t)j * Cp;
    double bv = 0.0, mx = -1.0;
    uint32_t bi = CL_NONE;
    for (uint32_t i = tid; i < C; i += 256) {
        const double v = row[i];
        cl_min_into(bv, bi, v, i);
        if (i != j && v > mx) mx = v;
    }
    s_v[tid] = bv; s_i[tid] = bi; s_m[tid] = mx;
    __syncthreads();
    for (uint32_t w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            double v = s_v[tid];
            uint32_t i = s_i[tid];
            cl_min_into(v, i, s_v[tid + w], s_i[tid + w]);
            s_v[tid] = v; s_i[tid] = i;
            if (s_m[tid + w] > s_m[tid]) s_m[tid] = s_m[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        cmin[j] = s_v[0];
        carg[j] = s_i[0];
        if (rowmax) rowmax[j] = s_m[0];
        if (flag) flag[j] = 0;
    }
}

struct ClPick {
    double value;
    uint32_t row, col;
};

// the minimum of V: over the columns j < C the smallest column minimum, ties to the lower column (one workgroup of 1024)
__global__ __launch_bounds__(1024) void k_cl_global_min(uint32_t C, const double *__restrict__ cmin, const uint32_t *__restrict__ carg,
                                                        ClPick *__restrict__ out)
{
    const uint32_t tid = threadIdx.x;
    __shared__ double s_v[1024];
    __shared__ uint32_t s_j[1024];
    double bv = 0.0;
    uint32_t bj = CL_NONE;
    for (uint32_t j = tid; j < C; j += 1024)
        if (carg[j] != CL_NONE) cl_min_into(bv, bj, cmin[j], j);
    s_v[tid] = bv; s_j[tid] = bj;
    __syncthreads();
    for (uint32_t w = 512; w > 0; w >>= 1) {
        if (tid < w) {
            double v = s_v[tid];
            uint32_t i = s_j[tid];
            cl_min_into(v, i, s_v[tid + w], s_j[tid + w]);
            s_v[tid] = v; s_j[tid] = i;
        }
        __syncthreads();
    }
    if (tid == 0) {
        const uint32_t j = s_j[0];
        out->value = j == CL_NONE ? __builtin_nan("") : s_v[0];
        out->col = j;
        out->row = j == CL_NONE ? CL_NONE : carg[j];
    }
}

// merge b into a: X[s][k][a] += X[s][k][b] for every sample and trace row; b is dead from here on
__global__ __launch_bounds__(256) void k_cl_merge(uint32_t N, uint32_t Cp, uint32_t S, uint32_t a, uint32_t b, double *__restrict__ X,
                                                  uint8_t *__restrict__ dead)
{
    const uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid == 0) dead[b] = 1;
    if (gid >= (uint64_t)S * N) return;
    double *x = X + gid * Cp;   // (s, k) = (gid / N, gid % N): row gid of the [S * N][Cp] array
    x[a] += x[b];
}

// cov[s][j] = X_a . X_j / (N - 1) of one sample (fma in k order; non-finite -> 0); j = a gives the merged variance
__global__ __launch_bounds__(256) void k_cl_row_cov(uint32_t N, uint32_t Cp, uint32_t a, const double *__restrict__ X, double *__restrict__ cov)
{
    const uint32_t j = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
    if (j >= Cp) return;
    const double *Xs = X + (uint64_t)s * N * Cp;
    double acc = 0.0;
    for (uint32_t k = 0; k < N; ++k) acc = __builtin_fma(Xs[(uint64_t)k * Cp + a], Xs[(uint64_t)k * Cp + j], acc);
    double v = acc / (double)(N - 1);
    if (!__builtin_isfinite(v)) v = 0.0;
    cov[(uint64_t)s * Cp + j] = v;
}

// Row and column a of V from the merged covariances (mean_corrs over ts = {a, b}, :483-512: r = cov / sqrt(var_a) / sqrt(var_j),
// the merged row keeps a's observed mask), row and column b NaN, dead candidates NaN; then the column minima: a column whose minimum
// sat in row a or b, and column a itself, is flagged for a rescan, any other takes V(a, j) when it undercuts (ties: a < its row).
__global__ __launch_bounds__(256) void k_cl_row_update(uint32_t C, uint32_t Cp, uint32_t S, uint32_t a, uint32_t b,
                                                       const double *__restrict__ cov, double *__restrict__ var,
                                                       const uint8_t *__restrict__ obs, const uint8_t *__restrict__ dead,
                                                       double *__restrict__ V, double *__restrict__ cmin, uint32_t *__restrict__ carg,
                                                       uint8_t *__restrict__ flag)
{
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= C) return;
    double v = __builtin_nan("");
    if (!dead[j]) {
        double vs = 0.0;
        uint32_t cnt = 0;
        for (uint32_t s = 0; s < S; ++s) {
            const double va = cov[(uint64_t)s * Cp + a];
            const double vj = j == a ? va : var[(uint64_t)s * Cp + j];
            double rr = cov[(uint64_t)s * Cp + j] / __builtin_sqrt(va) / __builtin_sqrt(vj);
            const uint32_t u = (obs[(uint64_t)s * Cp + a] & obs[(uint64_t)s * Cp + j]) ? 1u : 0u;
            if (!u) rr = 0.0;
            vs += rr;
            cnt += u;
        }
        v = vs / (double)cnt;
    }
    V[(uint64_t)a * Cp + j] = v;
    V[(uint64_t)j * Cp + a] = v;
    V[(uint64_t)b * Cp + j] = __builtin_nan("");
    V[(uint64_t)j * Cp + b] = __builtin_nan("");
    if (j == a) {
        for (uint32_t s = 0; s < S; ++s) var[(uint64_t)s * Cp + a] = cov[(uint64_t)s * Cp + a];
        flag[j] = 1;
    } else if (j == b || dead[j]) {
        cmin[j] = __builtin_nan("");
        carg[j] = CL_NONE;
    } else if (carg[j] == a || carg[j] == b) {
        flag[j] = 1;
    } else {
        double bv = cmin[j];
        uint32_t bi = carg[j];
        cl_min_into(bv, bi, v, a);
        cmin[j] = bv;
        carg[j] = bi;
    }
}

} // namespace mmg
