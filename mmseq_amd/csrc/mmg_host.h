// mmg_host.h -- shared by the host translation units of libmmgibbs (mmgibbs.hip, sampler.hip, em_host.hip, post_host.hip):
// the problem handle, error plumbing, caller <-> device transcript numbering.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <atomic>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>
#include "../../include/mmgibbs.h"
#include "mmg_types.h"

namespace mmg {

int fail(int code, const std::string &msg);   // records the thread-local message behind mmg_last_error(), returns code
int opt(int option);                          // mmg_selftest_option value, -1 = default
bool fail_acquire();                          // MMG_OPT_FAIL_ALLOC: this acquisition of an owner below is the one that fails
enum { LIVE_BUFFERS = 0, LIVE_STREAMS = 1, LIVE_EVENTS = 2 };
void count_live(int kind, int delta);         // what the owners below hold, for mmg_selftest_live

// Owners of the library's device memory, streams and events.  Every acquisition goes through them (MMG_OPT_FAIL_ALLOC counts them);
// a handle's members are owners, so what a failed create built is released by the destructors, in reverse declaration order.
template <typename T> struct elem_size { static constexpr size_t value = sizeof(T); };
template <> struct elem_size<void> { static constexpr size_t value = 1; };

// A device buffer and the device it was allocated on: freed there, with the caller's current device restored.
template <typename T>
class DevBuf {
public:
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    DevBuf(DevBuf &&o) noexcept : p_(o.p_), dev_(o.dev_) { o.p_ = nullptr; }
    template <typename U, typename V = T, typename = std::enable_if_t<std::is_void<V>::value>>
    DevBuf(DevBuf<U> &&o) noexcept : p_(o.p_), dev_(o.dev_) { o.p_ = nullptr; } // (DevBuf<void>: a typed buffer seen as bytes)
    DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { reset(); p_ = o.p_; dev_ = o.dev_; o.p_ = nullptr; } return *this; }
    ~DevBuf() { reset(); }
    hipError_t alloc(size_t count)
    {
        reset();
        if (fail_acquire()) return hipErrorOutOfMemory;
        hipError_t e = hipGetDevice(&dev_);
        if (e == hipSuccess) e = hipMalloc((void **)&p_, count * elem_size<T>::value);
        if (e != hipSuccess) p_ = nullptr;
        else count_live(LIVE_BUFFERS, 1);
        return e;
    }
    T *get() const { return p_; }
    int device() const { return dev_; }
    explicit operator bool() const { return p_ != nullptr; }
    T *release() // (the caller frees it: no longer counted)
    {
        if (p_) count_live(LIVE_BUFFERS, -1);
        T *p = p_;
        p_ = nullptr;
        return p;
    }
    void reset()
    {
        if (!p_) return;
        int cur = dev_;
        (void)hipGetDevice(&cur);
        if (cur != dev_) (void)hipSetDevice(dev_);
        (void)hipFree((void *)p_);
        if (cur != dev_) (void)hipSetDevice(cur);
        p_ = nullptr;
        count_live(LIVE_BUFFERS, -1);
    }

private:
    template <typename> friend class DevBuf;
    T *p_ = nullptr;
    int dev_ = 0;
};

// Pinned host memory, freed with its owner (counted with the buffers).
template <typename T>
class PinnedBuf {
public:
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { reset(); }
    hipError_t alloc(size_t count)
    {
        reset();
        if (fail_acquire()) return hipErrorOutOfMemory;
        hipError_t e = hipHostMalloc((void **)&p_, count * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) p_ = nullptr;
        else count_live(LIVE_BUFFERS, 1);
        return e;
    }
    T *get() const { return p_; }
    void reset()
    {
        if (!p_) return;
        (void)hipHostFree((void *)p_);
        p_ = nullptr;
        count_live(LIVE_BUFFERS, -1);
    }

private:
    T *p_ = nullptr;
};

// A stream or an event, destroyed with its owner.
template <typename H, hipError_t (*Create)(H *, unsigned), hipError_t (*Destroy)(H), int Kind>
class DevHandle {
public:
    DevHandle() = default;
    DevHandle(const DevHandle &) = delete;
    DevHandle &operator=(const DevHandle &) = delete;
    DevHandle(DevHandle &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
    ~DevHandle() { reset(); }
    hipError_t create(unsigned flags = 0)
    {
        reset();
        if (fail_acquire()) return hipErrorOutOfMemory; // (what hipStreamCreate* / hipEventCreate* return when the runtime cannot create one)
        hipError_t e = Create(&h_, flags);
        if (e != hipSuccess) h_ = nullptr;
        else count_live(Kind, 1);
        return e;
    }
    H get() const { return h_; }
    explicit operator bool() const { return h_ != nullptr; }
    void reset()
    {
        if (!h_) return;
        (void)Destroy(h_);
        h_ = nullptr;
        count_live(Kind, -1);
    }

private:
    H h_ = nullptr;
};
using DevStream = DevHandle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy, LIVE_STREAMS>;
using DevEvent = DevHandle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy, LIVE_EVENTS>;

// a failed HIP call: record it and return MMG_ERR_HIP (functions that return an MMG_* code) ...
#define HIP_TRY(expr)                                                                                         \
    do {                                                                                                      \
        hipError_t _e = (expr);                                                                               \
        if (_e != hipSuccess)                                                                                 \
            return mmg::fail(MMG_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));                 \
    } while (0)
// ... or return the error itself (functions that return a hipError_t: layout.hip, order.hip)
#define HIPE_TRY(expr)                                                                                        \
    do {                                                                                                      \
        hipError_t _e = (expr);                                                                               \
        if (_e != hipSuccess) return _e;                                                                      \
    } while (0)

} // namespace mmg

struct mmg_problem {
    int device = 0;
    uint64_t m = 0, nnz = 0, total_k = 0, row_id_base = 0, device_bytes = 0;
    uint64_t total_k_hit = 0;                   // the reads of the rows with at least one hit: what a sweep allocates (an empty row gets no count)
    uint32_t n = 0, max_row_len = 0;
    bool idx64 = false;
    int cu_count = 256;
    int layout = MMG_LAYOUT_CANONICAL;
    mmg::DevBuf<void> d_row_ptr;                // uint32_t or (idx64) uint64_t offsets
    mmg::DevBuf<uint32_t> d_col;
    mmg::DevBuf<uint32_t> d_k;
    mmg::DevBuf<double> d_l;                    // device numbering
    std::vector<double> h_l;                    // caller numbering
    // transcript renumbering (tx_order): empty / nullptr = identity
    std::vector<uint32_t> h_int_of_ext, h_ext_of_int;
    mmg::DevBuf<uint32_t> d_int_of_ext, d_ext_of_int;
    // sliced-ELL stream of k_sample_sell / k_em_sell
    mmg::DevBuf<uint8_t> d_sell;
    uint64_t sell_bytes = 0, n_sell_tiles = 0, n_fast_tiles = 0, n_far_tiles = 0, padded_slots = 0;
    mmg::DevBuf<mmg::SellTile> d_sell_tiles;
    mmg::DevBuf<uint64_t> d_sell_chunk;
    int grid_sell = 0;
    // problems with multiplicities: the SELL_HASK tiles and the others as two descriptor lists with their own ranges (null / 0: no
    // SELL_HASK tile -- the one launch over d_sell_tiles does everything)
    mmg::DevBuf<mmg::SellTile> d_sell_tiles_1, d_sell_tiles_k;
    mmg::DevBuf<uint64_t> d_sell_chunk_k;
    int grid_sell_k = 0;
    uint64_t n_hask_tiles = 0;
    // the rows on the conditional-binomial chain (mmg_types.h: bigk_row): their stored positions, ascending -- sampled by k_sample_bigk in
    // pieces of bigk_per_wave list entries per workgroup (the tile kernel skips them); h_bigk_list: the host's copy (the timed shard cut)
    mmg::DevBuf<uint64_t> d_bigk_list;
    uint64_t n_bigk = 0;
    uint32_t bigk_per_wave = 0;
    int grid_bigk = 0;
    std::vector<uint64_t> h_bigk_list;
    // chains advanced in pairs: k_sample_sell_multi walks the register-path tiles without multiplicities (d_sell_tiles_f; the whole
    // list when every tile is like that) in its own ranges (2 and 4 chains: fewer resident waves); the other tiles without
    // multiplicities -- far tiles, CSR-walked tiles -- are a third list (d_sell_tiles_x) that k_sample_sell walks for all the
    // chains of the sampler in ONE launch (grid.y = chain), and so are the SELL_HASK tiles
    mmg::DevBuf<mmg::SellTile> sell_tiles_f, d_sell_tiles_x; // sell_tiles_f: a list of its own, when not every tile is on the register path
    const mmg::SellTile *d_sell_tiles_f = nullptr;       // sell_tiles_f or d_sell_tiles (not owned)
    mmg::DevBuf<uint64_t> d_sell_chunk_m[2], d_sell_chunk_x;
    int grid_sell_m[2] = {0, 0}, grid_sell_x = 0;
    uint64_t n_x_tiles = 0;
    bool use_sell = false;
    std::vector<uint64_t> h_sell_cum;           // cumulative tile cost, kept for the EM kernel's own ranges
    // read shards (mmg_problem_shard_bounds): first row of every tile and the cumulative modelled cost of a sweep over the tiles
    // [0, t) -- multiplicities included, a register-path tile priced by its groups (the stream bounds K1: time follows bytes)
    std::vector<uint64_t> h_tile_row, h_shard_cum;
    // the tile lists of the one-chain sample launches as the host built them (mmg_problem_shard_bounds_timed launches the kernels over
    // sub-intervals of them): entry e of the main list is tile h_list1_tile[e] (empty: the identity) and costs h_cum1[e + 1] - h_cum1[e]
    // in the units of the launch's ranges; the same for the list of multiplicity tiles
    std::vector<uint64_t> h_cum1, h_cumk;
    std::vector<uint32_t> h_list1_tile, h_listk_tile;
    uint64_t resident1 = 0, residentk = 0;      // workgroups of the two kernels the device holds at once
    uint32_t cnt_replicas = 1;                  // replicas of a sampler's count vectors (mmg_types.h: CNT_REPLICAS), 1 or CNT_REPLICAS
    bool canonical_rows = false;                // the rows are in canonical order: a canonical problem, or a shard cut from one
    // CSR tiles of the fallback kernel k_sample (built only when the sliced-ELL stream is not used)
    mmg::DevBuf<mmg::TileDesc> d_tiles;
    uint64_t n_tiles = 0;
    mmg::DevBuf<uint64_t> d_chunk_tile;
    int grid_sample = 1;
    mmg::DevBuf<uint64_t> d_colcnt;             // hits per transcript, for the EM scale words (lazy)
    bool order_derived = false;                 // the renumbering came from the hit graph (order.hip), not from the caller's tx_order
    bool k1_fixed_walk = false;    // the k = 1 sample kernel's straight-line instantiation (fewer than 5 groups per register-path tile on average)
    // the single-chain launch runs k_sample_sell's lean instantiation (sell_kernels.h: LEAN): its list holds nothing but
    // register-path and empty tiles
    bool k1_lean = false;
    // what the constant model of the kernel choice and of the order derivation makes of a sweep (2 per register-path tile): those
    // thresholds were fitted in its units; the ranges are cut by h_sell_cum / h_cum1, which price a tile by its groups
    uint64_t sweep_cost_const = 0;
    uint64_t range_tile_cost = 0;  // the ranges price a register-path tile this + 1 per group of its block (0: the constant model, MMG_OPT_K1_RANGE_COST = 0)
    uint64_t range_cost_max = 0, range_cost_sum = 0, range_count = 0; // modelled cost of the single-chain launch's non-empty ranges
    uint64_t range_tiles_max = 0;                                     // tiles of its longest range
    std::vector<uint64_t> h_chunk1, h_chunk1_groups;                  // its ranges: entries of the list h_cum1 prices; groups in front of every bound
    // the five tile lists a sample call can launch over (main or list 1, multiplicity, pairs, fours, far / CSR of the paired chains):
    // entries, ranges, entries of the longest range (mmg_selftest_k1_lists); all 0 for a list the problem does not have
    uint64_t k1_lists[5][3] = {};
    bool groups_reordered = false; // tx_order given and the library reordered its groups (spec version 7)
    bool order_skipped = false;    // an order from the hit graph was called for but not tried (device memory) or could not be built: the caller's order stands
    bool renumbered() const { return !h_int_of_ext.empty(); }
};

struct mmg_sampler;
struct mmg_em;

namespace mmg {

// Device-to-host copies into the caller's (pageable) memory through two pinned buffers the handle keeps: the runtime would otherwise
// pin and unpin the destination pages for every copy, and a caller that fetches trace rows while the chain runs -- and while its other
// threads allocate and write files -- had the chain's kernels stall for 20-40 ms at a time around those (un)pinnings (the 50 M-read
// CLI run: the chain took 4.5 s instead of 3.9 s).  One copy at a time per stage (the owner's mutex).
struct PinnedStage {
    static constexpr size_t CHUNK = 16u << 20;
    void *buf[2] = {nullptr, nullptr};
    DevEvent ev[2];
    ~PinnedStage()
    {
        for (int i = 0; i < 2; ++i) if (buf[i]) (void)hipHostFree(buf[i]);
    }
    hipError_t copy_out(void *dst, const void *dsrc, size_t bytes, hipStream_t st)
    {
        for (int i = 0; i < 2; ++i) {
            if (!buf[i]) { hipError_t e = hipHostMalloc(&buf[i], CHUNK, hipHostMallocDefault); if (e != hipSuccess) { buf[i] = nullptr; return e; } }
            if (!ev[i]) HIPE_TRY(ev[i].create(hipEventDisableTiming));
        }
        const size_t chunks = (bytes + CHUNK - 1) / CHUNK;
        auto issue = [&](size_t c) {
            const size_t off = c * CHUNK, len = bytes - off < CHUNK ? bytes - off : CHUNK;
            hipError_t e = hipMemcpyAsync(buf[c & 1], (const char *)dsrc + off, len, hipMemcpyDeviceToHost, st);
            return e == hipSuccess ? hipEventRecord(ev[c & 1].get(), st) : e;
        };
        if (chunks) { hipError_t e = issue(0); if (e != hipSuccess) return e; }
        for (size_t c = 0; c < chunks; ++c) {
            if (c + 1 < chunks) { hipError_t e = issue(c + 1); if (e != hipSuccess) return e; } // (its buffer was emptied an iteration ago)
            hipError_t e = hipEventSynchronize(ev[c & 1].get());
            if (e != hipSuccess) return e;
            const size_t off = c * CHUNK, len = bytes - off < CHUNK ? bytes - off : CHUNK;
            std::memcpy((char *)dst + off, buf[c & 1], len);
        }
        return hipSuccess;
    }
};

// what the summary code needs to see of a sampler (sampler.hip)
struct SamplerView {
    const mmg_problem *p;
    mmg_config cfg;
    const double *d_trace;   // [C][trace_len][n] sample-major, device numbering; nullptr without keep_trace
    hipStream_t stream;
    int iter;
    int64_t n_kept;          // samples kept so far
    // how often mmg_sampler_extend has rewritten the trace: a handle that keeps rows derived from it compares the value at its
    // creation with the current one (shared: the counter outlives the sampler while such a handle exists)
    std::shared_ptr<const std::atomic<uint64_t>> extensions;
};
int sampler_view(mmg_sampler *s, SamplerView *v);

// what the contrast code needs to see of a summary (post.hip)
struct SummaryView {
    const mmg_problem *p;
    int device;
    uint32_t n, nv, S;
    const double *trace;     // the summary's chain: [S][n] sample-major, device numbering (the sampler's memory)
    bool finished;
    uint64_t seed;           // the simulated traces: Gamma(alpha) * vscale[v] keyed (seed, chain 0, TAG_SIMU, vid[v], sample)
    double alpha;
    const uint64_t *vid;     // [nv], host (the summary's)
    const double *vscale;
};
int summary_view(mmg_summary *q, SummaryView *v);
std::vector<double> series_twiddles(uint32_t S);   // the twiddle table of k_series_summary (post.hip)

// a host array as a device buffer of its own (one word for an empty array), copied in stream order
template <typename T>
inline hipError_t upload(DevBuf<T> &buf, const T *src, size_t count, hipStream_t st)
{
    HIPE_TRY(buf.alloc(count ? count : 1));
    if (count) HIPE_TRY(hipMemcpyAsync(buf.get(), src, count * sizeof(T), hipMemcpyHostToDevice, st));
    return hipSuccess;
}

// Where the member traces of the contrasts, the isoform groups and the pairs come from (contrast.hip): a chain of a sampler, [S][n]
// sample-major in device numbering, with the nv isoforms without hits drawn on demand (member n + v: Gamma(alpha) * vscale[v] keyed
// (seed, chain 0, TAG_SIMU, vid[v], sample)) -- or the caller's host traces [n][S], uploaded.  A handle that answers row queries after
// its creation keeps it as a member: the owned buffers go with the handle.
struct MemberSource {
    int device = 0;
    uint32_t S = 0, n = 0, nv = 0;
    bool from_traces = false;
    const double *trace = nullptr;        // the chain (the sampler's memory)
    const uint32_t *int_of_ext = nullptr; // the problem's; null: the identity
    uint64_t seed = 0;
    double alpha = 0.0;
    DevBuf<uint64_t> d_vid;               // [nv]
    DevBuf<double> d_vscale;
    DevBuf<double> d_traces;              // from host traces: [n][S]
    // The chain of summary q of sampler s, its simulated isoforms included, in two steps with the caller's own argument checks in
    // between (members < n + nv, S samples: known after the first, and checked before any device work).  view_summary: the views and
    // what can be wrong with them; not_finished: the message when the summary is not finished.  acquire: waits for the sampler,
    // leaves the summary's device current and copies the isoforms' ids and scales to it.
    int view_summary(mmg_sampler *s, mmg_summary *q, const char *not_finished);
    int acquire(mmg_sampler *s);
    // chain `chain` of a sampler's kept trace, no simulated isoforms; no device work
    void from_chain(const SamplerView &v, int chain);
    // host traces [n_series][S] to the current device, which is `device`
    int from_host(int device_, uint32_t S_, uint32_t n_series, const double *traces);
    // the series-major rows of the nm members d_cols[0 .. nm): gathered into M[nm][S] in stream order and M returned -- or, from host
    // traces, the uploaded matrix itself (the members are its rows: nothing is gathered)
    const double *rows(const uint32_t *d_cols, uint32_t nm, double *M, hipStream_t st) const;

private:
    const uint64_t *h_vid_ = nullptr;     // the summary's host arrays, between view_summary and acquire
    const double *h_vscale_ = nullptr;
};

// The distinct members of consecutive slabs of member lists: per slab its columns in ascending order (neighbours in the caller's
// numbering are mostly neighbours on the device) and every member's slot, its rank among them.  The cut rule is the caller's: it asks
// fresh(), adds the members of what it takes into the open slab, and closes the slab.
class SlabColumns {
public:
    std::vector<uint32_t> cols;   // the closed slabs' columns one after the other, then the open slab's in the order they came
    explicit SlabColumns(size_t limit) : slot_of_(limit, NONE) {}
    bool fresh(uint32_t member) const { return slot_of_[member] == NONE; }   // not in the open slab yet
    void add(uint32_t member) { if (fresh(member)) { slot_of_[member] = 0; cols.push_back(member); } }
    uint64_t first() const { return base_; }                 // the open slab is cols[first() .. first() + count())
    uint64_t count() const { return cols.size() - base_; }
    // Ends the open slab: sorts its columns, calls lists(slot), in which slot(member) is the member's slot and the caller rewrites the
    // slab's lists, and opens the next slab.
    template <typename F>
    void close(F &&lists)
    {
        std::sort(cols.begin() + (ptrdiff_t)base_, cols.end());
        for (size_t i = base_; i < cols.size(); ++i) slot_of_[cols[i]] = (uint32_t)(i - base_);
        lists([this](uint32_t member) { return slot_of_[member]; });
        for (size_t i = base_; i < cols.size(); ++i) slot_of_[cols[i]] = NONE;
        base_ = cols.size();
    }

private:
    static constexpr uint32_t NONE = 0xffffffffu;
    std::vector<uint32_t> slot_of_;
    size_t base_ = 0;
};

// read shards of one problem as one EM (em_host.hip): make_reduce(members, ctx) returns the exchange called between the phases with
// what = 0 (xe: max, int32), 1 (accumulators + log-likelihood limbs: sum, uint64), 2 (column counts: sum, uint64); the buffers of a
// member come from em_exchange_buffers
int em_create_sharded(const mmg_problem *const *shards, int n_shards, const double *mu0,
                      std::function<int(int)> (*make_reduce)(const std::vector<mmg_em *> &, void *), void *ctx, mmg_em **ems, double *loglik0);
void em_exchange_buffers(mmg_em *e, int what, void **ptr, size_t *count);
int em_device(const mmg_em *e);

// mmdiff's effect summaries (diff_effects.hip).  effects_check: the argument rules that mmg_effects_of_rows and
// mmg_diff_effects_summarize share, before any device work.  effects_of_device_rows: the summary of rows[S][P][F] that are on `device`
// already (checked, gamma 0.0 / 1.0, model_of[P - 1] on the host); the rows are free again when it returns.
int effects_check(uint32_t S, uint32_t P, uint32_t np, const double *percentiles);
int effects_of_device_rows(int device, uint32_t S, uint32_t P, uint32_t F, const double *d_rows, const uint8_t *model_of, uint32_t np,
                           const double *percentiles, mmg_effects **out);

// mmdiff's permutation null (qvalue.hip), both on stream st of the current device.  qvalue_stat_on_device: stat[R][F], the log Bayes
// factor of every replica and feature from R state blocks `stride` doubles apart (slots gsum and logitp); in stream order, not
// synchronised.  qvalues_on_device: mmg_qvalues of device arrays into device arrays; the stream has been waited for when it returns.
int qvalue_stat_on_device(hipStream_t st, const double *d_st, size_t stride, int gsum, int logitp, uint32_t F, uint32_t R, uint32_t sampled,
                          double *d_stat);
int qvalues_on_device(hipStream_t st, uint32_t F, const double *d_obs, uint64_t n_null, const double *d_null, uint64_t *d_null_ge, double *d_q);

// mmdiff's design rules (diff.hip), shared with the likelihood-ratio test (diff_lrt.hip).  df_nil: the reference's "nil" rule.
// df_classes: the classes of one model, C[i * stride]: labels 0 .. *nc - 1, every one of them used (MMG_ERR_ARG otherwise).
bool df_nil(const double *X, uint32_t N, uint32_t cols);
int df_classes(const int32_t *C, uint32_t stride, uint32_t N, int *nc);
// The argument checks the create entries of mmg_diff_*, mmg_diff_poly / chains / perm_* and mmg_diff_lrt* share, each MMG_ERR_ARG with
// the entries' message; an entry calls them in the order of its documented checks, its own counts in between.  df_check_shape: F, N and
// the columns of M; df_check_cols: the columns of P0 and of J matrices P1; df_check_finite: y, e, M, P0 and P1 (N x L1 values);
// df_check_classes: both models of a class table [N][2].
int df_check_shape(uint32_t F, uint32_t N, uint32_t K);
int df_check_cols(uint32_t L0, uint32_t J, const uint32_t *L1);
int df_check_prior(double d, double s, double pdash);
int df_check_finite(uint32_t F, uint32_t N, const double *y, const double *e, uint32_t K, const double *M, uint32_t L0, const double *P0,
                    uint64_t L1, const double *P1);
int df_check_classes(const int32_t *C, uint32_t N, int nc[2]);
// y and e^2 transposed to [N][F] (the lanes of a wave read adjacent words), copied to d_y / d_esq in stream order.  `staged` holds the
// sources of the asynchronous copies: it lives until the caller has waited for the stream.
struct DiffStaged { std::vector<double> ty, te; };
int df_upload_transposed(hipStream_t st, uint32_t F, uint32_t N, const double *y, const double *e, double *d_y, double *d_esq, DiffStaged &staged);

int require_device(int device);
void weighted_chunks(const std::vector<uint64_t> &cum, uint64_t grid, std::vector<uint64_t> &chunk);
void weighted_chunks_tapered(const std::vector<uint64_t> &cum, uint64_t grid, uint64_t resident, std::vector<uint64_t> &chunk);

// caller numbering <-> device numbering of per-transcript host arrays
template <typename T>
inline void to_int(const mmg_problem *p, const T *ext, std::vector<T> &out)
{
    out.resize(p->n);
    if (p->renumbered()) for (uint32_t i = 0; i < p->n; ++i) out[i] = ext[p->h_ext_of_int[i]];
    else std::memcpy(out.data(), ext, p->n * sizeof(T));
}
template <typename T>
inline void to_ext(const mmg_problem *p, const std::vector<T> &in, T *ext)
{
    if (p->renumbered()) for (uint32_t t = 0; t < p->n; ++t) ext[t] = in[p->h_int_of_ext[t]];
    else std::memcpy(ext, in.data(), p->n * sizeof(T));
}
template <typename T>
inline int download_ext(const mmg_problem *p, const T *d_src, T *ext)
{
    if (!p->renumbered()) { HIP_TRY(hipMemcpy(ext, d_src, p->n * sizeof(T), hipMemcpyDeviceToHost)); return MMG_OK; }
    std::vector<T> tmp(p->n);
    HIP_TRY(hipMemcpy(tmp.data(), d_src, p->n * sizeof(T), hipMemcpyDeviceToHost));
    to_ext(p, tmp, ext);
    return MMG_OK;
}

} // namespace mmg
