// diff_perm_kernels.h -- the shuffle of mmg_diff_perm_*: replica b >= 1 of a permutation handle is the data with every feature's
// samples shuffled.  The chain itself runs in diff_kernels.h's k_dfp_* kernels, blockIdx.y the replica.
#pragma once
#include "diff_kernels.h"

namespace mmg {

// One lane per (replica b = blockIdx.y + 1, feature f): a Fisher-Yates on the replica's own column of y and esq ([R][N][F], replica 0
// untouched), drawn from SeqStream(Stream(seed, b, TAG_DIFF_PERM, f, 0)).  Swapping the data in place is the permutation that
// mmdiff -permute (apply_permutation) forms by shuffling an index array and gathering through it: data[j] = old[idx[j]] holds before
// and after every swap.  No per-lane array, so nothing goes to scratch at N = 512; lane f touches words f of rows j and k, so a
// wave's accesses stay within two rows of F doubles.
__global__ void __launch_bounds__(DF_BLOCK) k_dfq_shuffle(double *__restrict__ y, double *__restrict__ esq, int F, int N, uint64_t seed)
{
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const uint32_t b = blockIdx.y + 1;
    const size_t base = (size_t)b * (size_t)N * (size_t)F + (size_t)f;
    double *yb = y + base, *eb = esq + base;
    SeqStream q(Stream(seed, b, TAG_DIFF_PERM, (uint64_t)f, 0));
    for (size_t j = (size_t)N - 1; j > 0; --j) {
        size_t k = (size_t)(q.next() * (double)(j + 1));
        if (k > j) k = j;
        const double ty = yb[j * F], te = eb[j * F];
        yb[j * F] = yb[k * F]; eb[j * F] = eb[k * F];
        yb[k * F] = ty; eb[k * F] = te;
    }
}

} // namespace mmg
