// extend.hip -- device TU of mmg_sampler_extend (sampler.hip): the kernels of extend_kernels.h and their launchers
#include "extend_kernels.h"
#include "mmg_launch.h"

namespace mmg {

static dim3 halve_grid(uint32_t n, uint32_t rows)
{
    // the pairs of a row and the lane behind them (n / 2 + 1 lanes at most); rows beyond grid.y's limit are strided over
    return dim3((n / 2u + 1u + 255u) / 256u, rows < 65535u ? rows : 65535u);
}

void launch_trace_halve(double *trace, double *scratch, uint32_t n, uint32_t S, hipStream_t s)
{
    const uint32_t half = S / 2u;
    if (!n || !half) return;
    hipLaunchKernelGGL(k_trace_halve, halve_grid(n, half), dim3(256), 0, s, scratch, (const double *)trace, n, half, half, 2u);
    hipLaunchKernelGGL(k_trace_halve, halve_grid(n, S), dim3(256), 0, s, trace, (const double *)scratch, n, half, S, 1u);
}

void launch_moments_rebuild(const double *trace, double *sum_log, double *sum_log2, uint32_t n, uint32_t n_chains, uint32_t S, uint32_t rows, hipStream_t s)
{
    if (!n || !n_chains) return;
    hipLaunchKernelGGL(k_moments_rebuild, dim3((n + 255u) / 256u, n_chains), dim3(256), 0, s, trace, sum_log, sum_log2, n, S, rows);
}

} // namespace mmg
