// diff_effects.hip -- device TU + host side of the mmg_effects_* entry points: mmdiff's effect summaries from recorded rows.  Kernel in
// diff_effects_kernels.h; specification in tests/mmdiff_effects_ref.py and DESIGN.md section 10.3.  mmg_diff_effects_summarize
// (diff.hip) hands the rows of its handle, which stay where they are, to effects_of_device_rows below.
#include "diff_effects_kernels.h"
#include "mmg_host.h"

#include <cmath>
#include <memory>
#include <vector>

using namespace mmg;

// The results stay on the device until mmg_effects_get.  Members are destroyed in reverse declaration order: the destructor waits
// for `st`, then the buffers go, and the stream last.
struct mmg_effects {
    DevStream st;
    int device = 0;
    uint32_t P = 0, F = 0, np = 0;
    DevBuf<uint32_t> d_n, d_ngt;
    DevBuf<double> d_mean, d_sd, d_q, d_pct;
    DevBuf<uint8_t> d_model;
    uint64_t device_bytes = 0;
    ~mmg_effects() { if (st) (void)hipStreamSynchronize(st.get()); }
};

int mmg::effects_check(uint32_t S, uint32_t P, uint32_t np, const double *percentiles)
{
    if (S == 0 || S > FX_SMAX) return fail(MMG_ERR_ARG, "the number of rows must be between 1 and 4096");
    if (P < 2 || P > 65536) return fail(MMG_ERR_ARG, "rows hold at least one parameter and gamma, 65536 in all at most");
    if (np > FX_NPMAX) return fail(MMG_ERR_ARG, "at most 32 percentiles");
    if (np && !percentiles) return fail(MMG_ERR_ARG, "NULL percentile array");
    for (uint32_t j = 0; j < np; ++j)
        if (!(percentiles[j] >= 0.0 && percentiles[j] <= 100.0)) return fail(MMG_ERR_ARG, "percentiles must be between 0 and 100");
    return MMG_OK;
}

int mmg::effects_of_device_rows(int device, uint32_t S, uint32_t P, uint32_t F, const double *d_rows, const uint8_t *model_of, uint32_t np,
                                const double *percentiles, mmg_effects **out)
{
    std::unique_ptr<mmg_effects> e(new mmg_effects());
    e->device = device; e->P = P; e->F = F; e->np = np;
    const uint64_t PF = (uint64_t)(P - 1) * F;
    auto dalloc = [&](auto &buf, uint64_t count) {
        HIPE_TRY(buf.alloc(count ? count : 1));
        e->device_bytes += count * sizeof(*buf.get());
        return hipSuccess;
    };
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(e->st.create(hipStreamNonBlocking));
    hipStream_t st = e->st.get();
    HIP_TRY(dalloc(e->d_n, 2 * (uint64_t)F));
    HIP_TRY(dalloc(e->d_ngt, PF));
    HIP_TRY(dalloc(e->d_mean, PF));
    HIP_TRY(dalloc(e->d_sd, PF));
    HIP_TRY(dalloc(e->d_q, PF * np));
    HIP_TRY(dalloc(e->d_pct, np));
    HIP_TRY(dalloc(e->d_model, P - 1));
    if (np) HIP_TRY(hipMemcpyAsync(e->d_pct.get(), percentiles, (size_t)np * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(e->d_model.get(), model_of, P - 1, hipMemcpyHostToDevice, st));
    const EffectsOut o{e->d_n.get(), e->d_mean.get(), e->d_sd.get(), e->d_ngt.get(), e->d_q.get()};
    const uint32_t tiles = (F + FX_TILE - 1) / FX_TILE;
#define FX_LAUNCH(KEYS, NSER)                                                                                                            \
    hipLaunchKernelGGL((k_df_effects<KEYS, NSER>), dim3(tiles, P - 1, FX_TILE / NSER), dim3(FX_BLOCK), 0, st, S, P, F, d_rows,            \
                       (const uint8_t *)e->d_model.get(), np, (const double *)e->d_pct.get(), o)
    // the keys a series has room for: the tile of eight within a CU's LDS up to 2048, half a tile per workgroup at 4096
    if (S <= 256) FX_LAUNCH(256, 8);
    else if (S <= 1024) FX_LAUNCH(1024, 8);
    else if (S <= 2048) FX_LAUNCH(2048, 8);
    else FX_LAUNCH(4096, 4);
#undef FX_LAUNCH
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));   // (the host arrays were the sources of asynchronous copies; the caller's rows are free again)
    *out = e.release();
    return MMG_OK;
}

extern "C" int mmg_effects_of_rows(int device, uint32_t S, uint32_t P, uint32_t F, const double *rows, const uint8_t *model_of, uint32_t np,
                                   const double *percentiles, mmg_effects **out)
{
    if (!out || !rows || !model_of) return fail(MMG_ERR_ARG, "NULL argument");
    *out = nullptr;
    int rc = effects_check(S, P, np, percentiles);
    if (rc) return rc;
    if (F == 0) return fail(MMG_ERR_ARG, "the number of features must be at least 1");
    for (uint32_t s = 0; s + 1 < P; ++s)
        if (model_of[s] > 1) return fail(MMG_ERR_ARG, "model_of must be 0 or 1");
    const size_t PF = (size_t)P * F;
    for (uint32_t r = 0; r < S; ++r) {
        const double *g = rows + (size_t)r * PF + (size_t)(P - 1) * F;
        for (uint32_t f = 0; f < F; ++f)
            if (!(g[f] == 0.0 || g[f] == 1.0))
                return fail(MMG_ERR_ARG, "gamma of row " + std::to_string(r) + ", feature " + std::to_string(f) + " is neither 0 nor 1");
    }
    rc = require_device(device);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> d_rows;
    HIP_TRY(d_rows.alloc((size_t)S * PF));
    HIP_TRY(hipMemcpy(d_rows.get(), rows, (size_t)S * PF * 8, hipMemcpyHostToDevice));
    return effects_of_device_rows(device, S, P, F, d_rows.get(), model_of, np, percentiles, out);
}

extern "C" int mmg_effects_get(mmg_effects *e, uint32_t *n, double *mean, double *sd, uint32_t *n_gt, double *q)
{
    if (!e) return fail(MMG_ERR_ARG, "NULL effects handle");
    HIP_TRY(hipSetDevice(e->device));
    const size_t F = e->F, PF = (size_t)(e->P - 1) * F;
    if (n) HIP_TRY(hipMemcpy(n, e->d_n.get(), 2 * F * 4, hipMemcpyDeviceToHost));
    if (mean) HIP_TRY(hipMemcpy(mean, e->d_mean.get(), PF * 8, hipMemcpyDeviceToHost));
    if (sd) HIP_TRY(hipMemcpy(sd, e->d_sd.get(), PF * 8, hipMemcpyDeviceToHost));
    if (n_gt) HIP_TRY(hipMemcpy(n_gt, e->d_ngt.get(), PF * 4, hipMemcpyDeviceToHost));
    if (q && e->np) HIP_TRY(hipMemcpy(q, e->d_q.get(), PF * e->np * 8, hipMemcpyDeviceToHost));
    return MMG_OK;
}

extern "C" int mmg_effects_device_bytes(mmg_effects *e, uint64_t *bytes)
{
    if (!e || !bytes) return fail(MMG_ERR_ARG, "NULL argument");
    *bytes = e->device_bytes;
    return MMG_OK;
}

extern "C" void mmg_effects_destroy(mmg_effects *e) { delete e; }
