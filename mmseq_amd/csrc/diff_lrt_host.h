// diff_lrt_host.h -- what diff_lrt.hip and diff_lrt_perm.hip share on the host: the handle of mmg_diff_lrt_*, and the observed test as
// one function that leaves its device arrays alive for a caller that goes on with them (DESIGN.md sections 10.5 and 10.6).
#pragma once
#include "diff_lrt_kernels.h"
#include "mmg_host.h"

#include <vector>

// Creation computes everything; the handle keeps the results on the host and no device memory.
struct mmg_diff_lrt {
    uint32_t F = 0;
    int32_t flags[3] = {0, 0, 0};
    uint32_t nc[2] = {0, 0}, p[2] = {0, 0};
    int32_t df = 0;
    uint64_t device_bytes = 0;
    std::vector<double> ll, stat, pv, qv, theta[2], sig[2];
    std::vector<uint32_t> iters, status;
};

namespace mmg {

// The device side of one observed test.  Members are released in reverse order, the stream last.
struct LrtDevice {
    DevStream st;
    DevBuf<double> d_y, d_esq, d_X[2], d_theta[2], d_sig[2], d_ll, d_ws;
    DevBuf<int> d_cls;
    DevBuf<uint32_t> d_iters, d_status;
    LrtParams q{};
    bool small = false;   // both models have p <= LRT_PSMALL: the register instantiation
    uint32_t pm = 0;      // max(p_0, p_1)
};

// the checks of mmg_diff_lrt_create that come before any device work, require_device last
int lrt_check_args(int device, uint32_t F, uint32_t N, const double *y, const double *e, uint32_t K, const double *M, uint32_t L0, const double *P0,
                   uint32_t L1, const double *P1, const int32_t *C, int nc[2]);
// mmg_diff_lrt_create after its checks: fills h (every result of the observed test) and leaves D's arrays as the k_lrt launch read
// and wrote them; D.st has been waited for when it returns, with an error too.
int lrt_observed(int device, uint32_t F, uint32_t N, const double *y, const double *e, uint32_t K, const double *M, uint32_t L0, const double *P0,
                 uint32_t L1, const double *P1, const int32_t *C, const int nc[2], int fixalpha, uint32_t max_iters, mmg_diff_lrt *h, LrtDevice &D);

} // namespace mmg
