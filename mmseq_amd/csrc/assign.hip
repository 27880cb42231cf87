// assign.hip -- device TU + host side of the mmg_assign_* entry points: the posterior assignment probability of every hit from a
// chain's trace.  Kernel in assign_kernels.h; specification in tests/assign_ref.py and DESIGN.md section 12.
#include "assign_kernels.h"
#include "mmg_host.h"
#include "mmg_launch.h"

#include <memory>
#include <vector>

using namespace mmg;

// Members are destroyed in reverse declaration order: the destructor waits for `st`, then the buffers go, and the stream last.
struct mmg_assign {
    DevStream st;
    int device = 0;
    uint64_t n_rows = 0, H = 0;
    uint32_t n_tx = 0;
    DevBuf<uint64_t> d_row_ptr;  // n_rows + 1, the caller's order
    DevBuf<uint32_t> d_col;      // the caller's numbering
    DevBuf<double> d_P;          // one per hit
    DevBuf<double> d_trace;      // [n_tx][trace_T] transcript-major, the caller's numbering: the trace of the last run
    DevBuf<double> d_scratch;    // scratch_waves slices of asg_pad(count) doubles
    uint64_t trace_T = 0, scratch_elems = 0;
    bool ran = false;
    uint64_t n_waves() const { return (H + ASG_HITS_PER_WAVE - 1) / ASG_HITS_PER_WAVE; }
    ~mmg_assign() { if (st) (void)hipStreamSynchronize(st.get()); }
};

extern "C" int mmg_assign_create(int device, uint64_t n_rows, uint32_t n_tx, const uint64_t *row_ptr, const uint32_t *col_idx, mmg_assign **out)
{
    if (!out || !row_ptr) return fail(MMG_ERR_ARG, "NULL argument");
    *out = nullptr;
    if (n_tx == 0) return fail(MMG_ERR_ARG, "n_tx must be at least 1");
    if (row_ptr[0] != 0) return fail(MMG_ERR_ARG, "row_ptr[0] must be 0");
    for (uint64_t i = 0; i < n_rows; ++i)
        if (row_ptr[i + 1] < row_ptr[i]) return fail(MMG_ERR_ARG, "row_ptr must not decrease");
    const uint64_t H = row_ptr[n_rows];
    if (H && !col_idx) return fail(MMG_ERR_ARG, "NULL argument");
    for (uint64_t j = 0; j < H; ++j)
        if (col_idx[j] >= n_tx) return fail(MMG_ERR_ARG, "column index out of range");
    int rc = require_device(device);
    if (rc) return rc;
    std::unique_ptr<mmg_assign> h(new mmg_assign());
    h->device = device; h->n_rows = n_rows; h->H = H; h->n_tx = n_tx;
    HIP_TRY(h->st.create(hipStreamNonBlocking));
    HIP_TRY(h->d_row_ptr.alloc(n_rows + 1));
    HIP_TRY(h->d_col.alloc(H ? H : 1));
    HIP_TRY(h->d_P.alloc(H ? H : 1));
    HIP_TRY(hipMemcpyAsync(h->d_row_ptr.get(), row_ptr, (n_rows + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, h->st.get()));
    if (H) HIP_TRY(hipMemcpyAsync(h->d_col.get(), col_idx, H * sizeof(uint32_t), hipMemcpyHostToDevice, h->st.get()));
    HIP_TRY(hipStreamSynchronize(h->st.get()));   // (the caller's arrays were the sources of asynchronous copies)
    *out = h.release();
    return MMG_OK;
}

// the trace copy and the scratch slices of a run over `count` samples of a trace of T samples; kept for the next run of the same shape
static int asg_reserve(mmg_assign *h, uint64_t T, uint32_t count)
{
    if (h->trace_T != T) {
        h->d_trace.reset();
        h->trace_T = 0;
        HIP_TRY(h->d_trace.alloc((uint64_t)h->n_tx * T));
        h->trace_T = T;
    }
    const uint64_t nw = h->n_waves();
    const int cap = opt(MMG_OPT_ASSIGN_WAVES);
    const uint64_t elems = asg_chunk_waves(nw, count, cap > 0 ? (uint32_t)cap : 0) * asg_pad(count);
    if (h->scratch_elems != elems) {
        h->d_scratch.reset();
        h->scratch_elems = 0;
        HIP_TRY(h->d_scratch.alloc(elems));
        h->scratch_elems = elems;
    }
    return MMG_OK;
}

// the launches over d_trace: the waves in chunks that share the scratch slices, in stream order
static int asg_launch(mmg_assign *h, uint32_t first, uint32_t count)
{
    const uint64_t nw = h->n_waves();
    const int cap = opt(MMG_OPT_ASSIGN_WAVES);
    const uint64_t per = asg_chunk_waves(nw, count, cap > 0 ? (uint32_t)cap : 0);
    AsgArgs a;
    a.row_ptr = h->d_row_ptr.get(); a.col = h->d_col.get(); a.n_rows = h->n_rows;
    a.tr = h->d_trace.get(); a.stride = h->trace_T; a.first = first; a.count = count;
    a.scratch = h->d_scratch.get(); a.P = h->d_P.get();
    for (uint64_t w0 = 0; w0 < nw; w0 += per) {
        a.wave0 = w0;
        a.n_waves = (uint32_t)(nw - w0 < per ? nw - w0 : per);
        const unsigned grid = (a.n_waves + ASG_BLOCK / ASG_LANES - 1) / (ASG_BLOCK / ASG_LANES);
        hipLaunchKernelGGL(k_assign, dim3(grid), dim3(ASG_BLOCK), 0, h->st.get(), a);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(h->st.get()));
    h->ran = true;
    return MMG_OK;
}

static int asg_check_range(int64_t T, int first, int count)
{
    if (first < 0 || count < 1 || (int64_t)first + count > T) return fail(MMG_ERR_ARG, "sample range outside the trace");
    return MMG_OK;
}

extern "C" int mmg_assign_run_sampler(mmg_assign *h, mmg_sampler *s, int chain, int first_sample, int n_samples)
{
    if (!h || !s) return fail(MMG_ERR_ARG, "NULL argument");
    SamplerView v;
    int rc = sampler_view(s, &v);
    if (rc) return rc;
    if (v.p->device != h->device) return fail(MMG_ERR_ARG, "the sampler lives on another device");
    if (v.p->n != h->n_tx) return fail(MMG_ERR_ARG, "the sampler's problem has another number of transcripts");
    if (chain < 0 || chain >= v.cfg.n_chains) return fail(MMG_ERR_ARG, "chain index out of range");
    if (!v.d_trace) return fail(MMG_ERR_STATE, "sampler was created with keep_trace == 0");
    rc = asg_check_range(v.cfg.trace_len, first_sample, n_samples);
    if (rc) return rc;
    if ((int64_t)first_sample + n_samples > v.n_kept) return fail(MMG_ERR_STATE, "the chain has not kept these samples yet");
    HIP_TRY(hipSetDevice(h->device));
    const uint64_t T = (uint64_t)v.cfg.trace_len;
    rc = asg_reserve(h, T, (uint32_t)n_samples);
    if (rc) return rc;
    // The sampler keeps its trace sample-major in the device's transcript numbering (one contiguous row per K2 launch).  The pass
    // needs it transcript-major in the caller's numbering, so it is transposed on the device, behind the chain on the sampler's
    // stream, exactly as mmg_sampler_get_trace does; nothing goes through the host.
    launch_transpose(v.d_trace + (uint64_t)chain * T * h->n_tx, h->d_trace.get(), h->n_tx, (uint32_t)T, v.p->d_int_of_ext.get(), v.stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(v.stream));
    return asg_launch(h, (uint32_t)first_sample, (uint32_t)n_samples);
}

extern "C" int mmg_assign_run_host(mmg_assign *h, const double *trace, int trace_len, int first_sample, int n_samples)
{
    if (!h || !trace) return fail(MMG_ERR_ARG, "NULL argument");
    if (trace_len < 1) return fail(MMG_ERR_ARG, "trace_len must be at least 1");
    int rc = asg_check_range(trace_len, first_sample, n_samples);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    rc = asg_reserve(h, (uint64_t)trace_len, (uint32_t)n_samples);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(h->d_trace.get(), trace, (uint64_t)h->n_tx * (uint64_t)trace_len * sizeof(double), hipMemcpyHostToDevice, h->st.get()));
    return asg_launch(h, (uint32_t)first_sample, (uint32_t)n_samples);
}

extern "C" int mmg_assign_get(mmg_assign *h, uint64_t first_hit, uint64_t n_hits, double *P)
{
    if (!h || (n_hits && !P)) return fail(MMG_ERR_ARG, "NULL argument");
    if (first_hit > h->H || n_hits > h->H - first_hit) return fail(MMG_ERR_ARG, "hit range out of bounds");
    if (!h->ran) return fail(MMG_ERR_STATE, "mmg_assign_get before a run");
    if (!n_hits) return MMG_OK;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpy(P, h->d_P.get() + first_hit, n_hits * sizeof(double), hipMemcpyDeviceToHost));
    return MMG_OK;
}

extern "C" int mmg_assign_device_bytes(mmg_assign *h, uint64_t *bytes)
{
    if (!h || !bytes) return fail(MMG_ERR_ARG, "NULL argument");
    const uint64_t Hs = h->H ? h->H : 1;
    *bytes = 8 * (h->n_rows + 1) + 4 * Hs + 8 * Hs + 8 * (uint64_t)h->n_tx * h->trace_T + 8 * h->scratch_elems;
    return MMG_OK;
}

extern "C" void mmg_assign_destroy(mmg_assign *h) { delete h; }
