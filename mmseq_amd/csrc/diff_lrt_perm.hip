// diff_lrt_perm.hip -- device TU + host side of the mmg_diff_lrt_perm_* entry points: the permutation null of mmdiff's likelihood-ratio
// test.  Kernels in diff_lrt_perm_kernels.h; the observed test is diff_lrt.hip's, the q-values qvalue.hip's.
#include "diff_lrt_perm_kernels.h"
#include "diff_lrt_host.h"

#include <cstring>
#include <memory>
#include <vector>

using namespace mmg;

constexpr uint32_t LRT_PERM_MAX = 65535;            // grid.y holds a slab of that many copies
constexpr uint64_t LRT_PERM_SLAB_BYTES = 1ull << 30;   // the default slab and its workspace stay under this

// Creation computes everything; the handle keeps the results on the host and no device memory.
struct mmg_diff_lrt_perm {
    uint32_t F = 0, B = 0;
    uint64_t device_bytes = 0;
    mmg_diff_lrt obs;
    std::vector<double> null_stat, perm_p, q;
    std::vector<uint8_t> null_status;
    std::vector<uint64_t> perm_ge, perm_n, null_ge;
};

extern "C" int mmg_diff_lrt_perm_create(int device, uint32_t F, uint32_t N, const double *y, const double *e, uint32_t K, const double *M,
                                        uint32_t L0, const double *P0, uint32_t L1, const double *P1, const int32_t *C, int fixalpha,
                                        uint32_t max_iters, uint32_t n_perm, uint64_t seed, uint32_t slab_copies, mmg_diff_lrt_perm **out)
{
    if (!out || !y || !e || !M || !P0 || !P1 || !C) return fail(MMG_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (n_perm < 1 || n_perm > LRT_PERM_MAX) return fail(MMG_ERR_ARG, "the number of permutations must be between 1 and 65535");
    if ((uint64_t)n_perm * F > 0x7fffffffull)
        return fail(MMG_ERR_ARG, "the number of permutations times the number of features must be at most 2147483647");
    int nc[2] = {0, 0};
    int rc = lrt_check_args(device, F, N, y, e, K, M, L0, P0, L1, P1, C, nc);
    if (rc) return rc;

    std::unique_ptr<mmg_diff_lrt_perm> h(new mmg_diff_lrt_perm());
    h->F = F; h->B = n_perm;
    // everything on the device is released when this function returns; `drain`, the last local, waits for the stream first
    LrtDevice D;
    rc = lrt_observed(device, F, N, y, e, K, M, L0, P0, L1, P1, C, nc, fixalpha, max_iters, &h->obs, D);
    if (rc) return rc;
    h->device_bytes = h->obs.device_bytes;
    hipStream_t st = D.st.get();

    const uint64_t B = n_perm, BF = B * F, NF = (uint64_t)N * F;
    const uint64_t wslots = lrt_perm_wslots((uint32_t)D.q.ncmax, D.pm);
    const uint64_t per_copy = 8 * (uint64_t)F * (2ull * N + wslots);
    uint64_t Sc = slab_copies ? slab_copies : LRT_PERM_SLAB_BYTES / per_copy;
    if (Sc < 1) Sc = 1;
    if (Sc > B) Sc = B;   // (B <= LRT_PERM_MAX, the bound of grid.y)

    DevBuf<double> d_T, d_obs, d_p, d_q, d_slab_y, d_slab_e, d_ws;
    DevBuf<uint8_t> d_status;
    DevBuf<uint64_t> d_ge, d_n, d_null_ge;
    struct Drain { hipStream_t s; ~Drain() { (void)hipStreamSynchronize(s); } } drain{st};
    HIP_TRY(d_T.alloc(BF));
    HIP_TRY(d_status.alloc(BF));
    HIP_TRY(d_obs.alloc(F));
    HIP_TRY(d_p.alloc(F));
    HIP_TRY(d_q.alloc(F));
    HIP_TRY(d_ge.alloc(F));
    HIP_TRY(d_n.alloc(F));
    HIP_TRY(d_null_ge.alloc(F));
    HIP_TRY(d_slab_y.alloc(Sc * NF));
    HIP_TRY(d_slab_e.alloc(Sc * NF));
    HIP_TRY(d_ws.alloc(Sc * wslots * F));
    h->device_bytes += 9 * BF + 48ull * F + Sc * per_copy;

    const uint32_t blocks = (F + LRT_BLOCK - 1) / LRT_BLOCK;
    for (uint64_t b0 = 0; b0 < B; b0 += Sc) {
        const uint32_t copies = (uint32_t)(B - b0 < Sc ? B - b0 : Sc);
        const dim3 grid(blocks, copies), block(LRT_BLOCK);
        if (D.small)
            hipLaunchKernelGGL(k_lrt_perm<LRT_PSMALL>, grid, block, 0, st, D.q, (uint32_t)wslots, (uint32_t)b0, seed, D.d_X[0].get(), D.d_X[1].get(),
                               D.d_cls.get(), D.d_y.get(), D.d_esq.get(), d_slab_y.get(), d_slab_e.get(), d_ws.get(), d_T.get(), d_status.get());
        else
            hipLaunchKernelGGL(k_lrt_perm<0>, grid, block, 0, st, D.q, (uint32_t)wslots, (uint32_t)b0, seed, D.d_X[0].get(), D.d_X[1].get(),
                               D.d_cls.get(), D.d_y.get(), D.d_esq.get(), d_slab_y.get(), d_slab_e.get(), d_ws.get(), d_T.get(), d_status.get());
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_lrt_perm_count, dim3(blocks), dim3(LRT_BLOCK), 0, st, (int)F, n_perm, D.d_ll.get(), d_T.get(), d_obs.get(), d_ge.get(),
                       d_n.get(), d_p.get());
    HIP_TRY(hipGetLastError());
    // the slab has done its work: it goes before the q-values take their working memory
    HIP_TRY(hipStreamSynchronize(st));
    d_slab_y.reset(); d_slab_e.reset(); d_ws.reset();
    rc = qvalues_on_device(st, F, d_obs.get(), BF, d_T.get(), d_null_ge.get(), d_q.get());
    if (rc) return rc;

    h->null_stat.resize(BF); h->null_status.resize(BF);
    h->perm_ge.resize(F); h->perm_n.resize(F); h->perm_p.resize(F); h->null_ge.resize(F); h->q.resize(F);
    HIP_TRY(hipMemcpyAsync(h->null_stat.data(), d_T.get(), BF * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h->null_status.data(), d_status.get(), BF, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h->perm_ge.data(), d_ge.get(), (size_t)F * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h->perm_n.data(), d_n.get(), (size_t)F * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h->perm_p.data(), d_p.get(), (size_t)F * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h->null_ge.data(), d_null_ge.get(), (size_t)F * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h->q.data(), d_q.get(), (size_t)F * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *out = h.release();
    return MMG_OK;
}

extern "C" mmg_diff_lrt *mmg_diff_lrt_perm_observed(mmg_diff_lrt_perm *h) { return h ? &h->obs : nullptr; }

extern "C" int mmg_diff_lrt_perm_get(mmg_diff_lrt_perm *h, uint64_t *perm_ge, uint64_t *perm_n, double *perm_p, uint64_t *null_ge, double *q_perm)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL argument");
    auto put = [](auto *dst, const auto &v) { if (dst) std::memcpy(dst, v.data(), v.size() * sizeof(v[0])); };
    put(perm_ge, h->perm_ge); put(perm_n, h->perm_n); put(perm_p, h->perm_p); put(null_ge, h->null_ge); put(q_perm, h->q);
    return MMG_OK;
}

extern "C" int mmg_diff_lrt_perm_get_null(mmg_diff_lrt_perm *h, uint32_t b0, uint32_t nb, double *stat, uint8_t *status)
{
    if (!h) return fail(MMG_ERR_ARG, "NULL argument");
    if ((uint64_t)b0 + nb > h->B) return fail(MMG_ERR_ARG, "the copies asked for go past the last one");
    const size_t o = (size_t)b0 * h->F, n = (size_t)nb * h->F;
    if (stat && n) std::memcpy(stat, h->null_stat.data() + o, n * 8);
    if (status && n) std::memcpy(status, h->null_status.data() + o, n);
    return MMG_OK;
}

extern "C" int mmg_diff_lrt_perm_device_bytes(mmg_diff_lrt_perm *h, uint64_t *bytes)
{
    if (!h || !bytes) return fail(MMG_ERR_ARG, "NULL argument");
    *bytes = h->device_bytes;
    return MMG_OK;
}

extern "C" void mmg_diff_lrt_perm_destroy(mmg_diff_lrt_perm *h) { delete h; }
