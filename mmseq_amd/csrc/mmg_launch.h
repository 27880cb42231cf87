// mmg_launch.h -- what the host side of the C ABI (mmgibbs.hip) sees of the device translation units.
// Every launcher enqueues on the given stream and returns; the caller checks hipGetLastError().
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include <vector>
#include "mmg_types.h"

namespace mmg {

template <typename T> class DevBuf; // mmg_host.h

// ---- k1.hip: the sample kernels (src/mmseq.cpp:857-891) and their stream builders
// k_sample_sell, 64 threads per workgroup; lean (k = 1 only): the instantiation for lists of register-path and empty tiles only (sell_kernels.h: LEAN)
const void *k1_sell_kernel(bool idx64, bool has_k, bool fixed_walk = false, bool lean = false);
const void *k1_sell_far_kernel(bool idx64);            // k_sample_sell for the list of far / CSR-walked tiles (far list prefetched), no multiplicities
const void *k1_sell_multi_kernel(bool idx64, int nch); // k_sample_sell_multi for nch = 2 or 4 chains (no multiplicities), 64 threads
const void *k1_csr_kernel(bool idx64, bool has_k);    // k_sample, K1C_BS threads per workgroup
const void *k1_bigk_kernel(bool idx64);                 // k_sample_bigk: the rows on the conditional-binomial chain, from their list (64 threads)
void launch_tile_desc(bool idx64, const void *row_ptr, const uint32_t *col, const uint32_t *kmult, const uint64_t *tile_row, uint64_t n_tiles,
                      TileDesc *out, hipStream_t s);
void launch_tile_far(bool idx64, const void *row_ptr, const uint32_t *col, const uint64_t *key, const uint64_t *tile_row,
                     const uint32_t *cand, uint64_t n_cand, uint32_t *out /* [3][n_cand] */, hipStream_t s);
void launch_encode_sell(bool idx64, const void *row_ptr, const uint32_t *col, const SellTile *tiles, uint64_t n_tiles,
                        uint8_t *stream, hipStream_t s);

// ---- em.hip: EM sweeps (src/mmseq.cpp:741-811)
const void *em_sell_kernel(bool idx64, bool has_k, bool measure); // k_em_sell, EM_SELL_BS threads per workgroup
constexpr int EM_SELL_W = 2, EM_SELL_REP = 4; // waves per workgroup (one window), accumulator replicas
constexpr unsigned EM_SELL_BS = 64 * EM_SELL_W;
void launch_em_rows_global(bool idx64, bool measure, const void *row_ptr, const uint32_t *col, const uint32_t *k, uint64_t m,
                           EmArgs a, hipStream_t s);
void launch_em_colcount(const uint32_t *col, uint64_t nnz, uint64_t *cnt, unsigned grid, hipStream_t s);
void launch_fill_i32(int32_t *p, uint32_t n, int32_t v, hipStream_t s);
void launch_combine(void *dst, const void *src, size_t n, bool max_i32, hipStream_t s); // dst[i] += src[i] (uint64) or max (int32), one device
void launch_em_prepare(uint32_t n, const double *mu, const double *l, const uint64_t *colcnt, const int32_t *ref, int measured,
                       uint32_t *word, uint64_t *hi, uint64_t *lo, double *partial, uint64_t *ll, const uint32_t *int_of_ext,
                       hipStream_t s);
void launch_em_check(uint32_t n, const uint32_t *word, const uint64_t *hi, uint64_t *ll, hipStream_t s);
void launch_em_finish(const double *partial, uint32_t np, const uint64_t *ll, EmOut *out, hipStream_t s);
void launch_em_apply(uint32_t n, double *mu, const double *l, const uint32_t *word, const uint64_t *hi, const uint64_t *lo,
                     int32_t *sexp, hipStream_t s);

// ---- misc.hip: Gamma redraw / trace (src/mmseq.cpp:896-917), read-out, start values, generator, self tests
void launch_update(const UpdateArgs &a, hipStream_t s, hipEvent_t start = nullptr, hipEvent_t stop = nullptr); // events: the launch's own time stamps (hipExtLaunchKernel)
// out[t_ext * S + smp] = in[smp * n + int_of_ext[t_ext]]   (int_of_ext == nullptr: identity)
void launch_transpose(const double *in, double *out, uint32_t n, uint32_t S, const uint32_t *int_of_ext, hipStream_t s);
// out[r * n + t_ext] = in[r * n + int_of_ext[t_ext]] for r < rows (element size 4 or 8 bytes)
void launch_gather_rows(const void *in, void *out, uint32_t n, uint32_t rows, int elem_bytes, const uint32_t *int_of_ext, hipStream_t s);
void launch_fold_counts(int32_t *cnt, uint64_t stride, size_t n, hipStream_t s); // replicas 1.. of the count vectors added into replica 0, zeroed
void launch_add_i32(int32_t *dst, const int32_t *src, size_t n, hipStream_t s); // dst[i] += src[i], one device
void launch_start_values(bool idx64, const void *row_ptr, const uint32_t *col, const uint32_t *k, uint64_t m, uint32_t n,
                         uint64_t *acc3, int32_t *unique_hits, hipStream_t s);
void launch_synth_len(const SynthArgs &a, double far_fraction, uint32_t *lens, hipStream_t s);
void launch_synth_fill(const SynthArgs &a, double far_fraction, const uint64_t *row_ptr, uint32_t *col, hipStream_t s);
void launch_selftest_math(int64_t n, const double *x, double *ol, double *oe, double *os, double *orc, hipStream_t s);
void launch_selftest_philox(const uint32_t *ctr, const uint32_t *key, uint32_t *out, hipStream_t s);
void launch_selftest_gamma(uint64_t seed, double shape, double scale, int64_t n, double *out, hipStream_t s);
void launch_selftest_binomial(uint64_t seed, uint32_t nn, double p, int64_t n, uint32_t *out, hipStream_t s);
void launch_selftest_btrs_pretest(uint64_t seed, int64_t n_cases, double n_lo, double n_hi, unsigned long long *counts /* [5], device */, hipStream_t s);
void launch_selftest_binv_pretest(uint64_t seed, int64_t n_cases, double n_lo, double n_hi, float slack, unsigned long long *counts /* [5], device */, hipStream_t s);
void launch_selftest_keyed(const mmg_keyed_io &io /* its pointers: device memory */, hipStream_t s);
void host_keyed(const mmg_keyed_io &io);
void launch_selftest_bigk_points(const mmg_bigk_points &io /* its pointers: device memory */, hipStream_t s);
void host_bigk_points(const mmg_bigk_points &io);
// host instantiations of the same inline code (device == -1 paths of the self tests, synthetic transcript tables)
void host_math(int64_t n, const double *x, double *ol, double *oe, double *os, double *orc);
void host_philox(const uint32_t *ctr, const uint32_t *key, uint32_t *out);
void host_gamma(uint64_t seed, uint32_t tag, uint64_t id0, int by_iter, double shape, double scale, int64_t n, double *out);
void host_binomial(uint64_t seed, uint32_t nn, double p, int64_t n, uint32_t *out);
void host_synth_tables(uint64_t seed, uint32_t T, double lambda, std::vector<double> &efflen, std::vector<double> &cdf,
                       std::vector<double> &len_cdf);
// exact start-value share limbs (host side of k_start_values)
double host_start_value(uint64_t a0, uint64_t a1, uint64_t a2, double l);

// ---- extend.hip: mmg_sampler_extend (extend_kernels.h)
// one chain's trace[S][n] (S even): row j becomes row 2 j for j < S / 2, rows S / 2 .. S - 1 become +0.0; scratch: n * S / 2 doubles
void launch_trace_halve(double *trace, double *scratch, uint32_t n, uint32_t S, hipStream_t s);
// sum_log / sum_log2 [n_chains][n] from the first `rows` rows of every chain of trace[n_chains][S][n], in sample order as k_update adds them
void launch_moments_rebuild(const double *trace, double *sum_log, double *sum_log2, uint32_t n, uint32_t n_chains, uint32_t S, uint32_t rows, hipStream_t s);

// ---- order.hip: a transcript order from the hit graph when the caller passes none
// sorted, duplicate-free directed edges u << 32 | v (both directions) of the co-occurrence graph of a content-hash sample of the rows
hipError_t order_cooccurrence_edges(bool idx64, uint64_t m, uint64_t nnz, const void *d_rp, const uint32_t *d_col, std::vector<uint64_t> &edges, hipStream_t s,
                                    const uint32_t *d_label = nullptr);
// pos[t] = position of transcript t in the derived order (level structures from pseudo-peripheral vertices; host code)
void order_from_edges(uint32_t n, const std::vector<uint64_t> &edges, std::vector<uint32_t> &pos, uint32_t hub_floor = 256);

// ---- layout.hip: the canonical row order (mmg_types.h) on the device
// Row keys of the CSR in its current order.  d_key: m u64 (caller frees).
hipError_t layout_map_cols(uint64_t nnz, uint32_t *d_col, const uint32_t *d_int_of_ext, hipStream_t s);
hipError_t layout_row_keys(uint64_t m, const uint64_t *d_rp, const uint32_t *d_col, const uint32_t *d_k, uint64_t *d_key, hipStream_t s);
// Sorts the CSR canonically: on return d_rp / d_col / d_k (k may be empty) are NEW device buffers in canonical order (the
// old ones are freed), d_key holds the sorted keys.  col_pad: extra u32 slots allocated (zeroed) behind col.  m < 2^32.
hipError_t layout_canonical_sort(uint64_t m, uint64_t nnz, DevBuf<uint64_t> &d_rp, DevBuf<uint32_t> &d_col, DevBuf<uint32_t> &d_k, uint64_t *d_key,
                                 size_t col_pad, hipStream_t s);
// Canonical layout, step 0: a row that draws k >= 2 categoricals becomes k rows with k = 1 (mmg_types.h: draws_categoricals).  *d_rp / *d_col / *d_k are replaced when
// any row expands; *m, *nnz follow; d_k is freed when no multiplicity other than 1 is left.
hipError_t layout_expand_rows(uint64_t *m, uint64_t *nnz, DevBuf<uint64_t> &d_rp, DevBuf<uint32_t> &d_col, DevBuf<uint32_t> &d_k, size_t col_pad, hipStream_t s);
// Start rows of the maximal runs of equal (near, band) in d_key (ascending; first entry 0).  Empty if there are more than
// max_segments runs (rows in no useful order).
hipError_t layout_segments(uint64_t m, const uint64_t *d_key, uint64_t max_segments, std::vector<uint64_t> &starts, hipStream_t s);
// d_out[0..rows] = row offsets of rows [lo, lo + rows) of a stored problem, rebased to 0 (d_out on the SAME device as d_rp)
hipError_t layout_rebase_row_ptr(bool idx64, const void *d_rp, uint64_t lo, uint64_t rows, uint64_t *d_out, hipStream_t s);
// narrow u64 row offsets to u32 on the device
hipError_t layout_narrow_row_ptr(uint64_t m, const uint64_t *d_rp64, uint32_t *d_rp32, hipStream_t s);
// d_rp[0..m] = running sum of d_len[0..m)
hipError_t layout_scan_lens(uint64_t m, const uint32_t *d_len, uint64_t *d_rp, hipStream_t s);
hipError_t layout_max_row_len(uint64_t m, const uint64_t *d_rp, uint32_t *max_len, hipStream_t s);
// The stored positions (ascending) of the rows on the conditional-binomial chain (mmg_types.h: bigk_row): d_list becomes a NEW device buffer
// of *n_list entries (empty / 0 without such rows or without multiplicities).  d_rp: the problem's row offsets (u32 or u64).
hipError_t layout_bigk_rows(bool idx64, uint64_t m, const void *d_rp, const uint32_t *d_k, DevBuf<uint64_t> &d_list, uint64_t *n_list, hipStream_t s);

// ---- post.hip: the convergence diagnostics across chains (conv_kernels.h) and the summary kernels they reuse (post_kernels.h)
// k_virtual_traces / k_group_sums of the summary, unchanged (V[s * nv + v], G[s * ng + g])
void launch_virtual_traces(uint64_t seed, uint32_t chain, uint32_t tag, double alpha, uint32_t nv, uint32_t S, const uint64_t *id, const double *scale,
                           double *V, hipStream_t s);
void launch_group_sums(uint32_t ng, uint32_t S, uint32_t n, uint32_t nv, const uint64_t *ptr, const uint32_t *member, const uint32_t *int_of_ext,
                       const double *trace, const double *V, double *G, hipStream_t s);
// out[(t * C + c) * S + s] = in[s * ld + col(t0 + t)], t < cnt (col null: the identity)
void launch_conv_slab(const double *in, uint64_t ld, uint32_t t0, uint32_t cnt, uint32_t S, uint32_t C, uint32_t c, const uint32_t *col, double *out,
                      hipStream_t s);
// k_convergence over cnt series X[series][C][S]: in LDS while C S <= 8192, else in ws (2 PP words per workgroup, ws_groups workgroups)
void launch_convergence(uint32_t cnt, uint32_t C, uint32_t S, const double *X, double inv_log10_p, double *rhat, double *ess_bulk, double *ess_tail,
                        uint64_t *ws, uint32_t ws_groups, hipStream_t s);

// ---- post.hip: the contrasts (contrast_kernels.h)
// M[j * S + s] = the trace of member col[j] < n (trace[s * n + int_of_ext[col[j]]]) or the simulated trace of isoform col[j] - n, j < nm
void launch_contrast_gather(uint32_t nm, uint32_t S, uint32_t n, const uint32_t *col, const uint32_t *int_of_ext, const double *trace, uint64_t seed,
                            double alpha, const uint64_t *vid, const double *vscale, double *M, hipStream_t s);
// R[w * S + s] = log N_s - log D_s of contrast c0 + w, w < cnt, its lists slots of M[slot][S]; gt[w] = samples with N_s > D_s (gt may be null)
void launch_contrast_series(uint32_t c0, uint32_t cnt, uint32_t S, const uint64_t *num_ptr, const uint32_t *num_slot, const uint64_t *den_ptr,
                            const uint32_t *den_slot, const double *M, double *R, uint32_t *gt, hipStream_t s);
// k_contrast_summary over cnt series R[series][S]: in LDS while S <= 8192, else in ws (3 SP words per workgroup, ws_groups workgroups)
void launch_contrast_summary(uint32_t cnt, uint32_t S, const double *R, uint32_t np, const int32_t *pind, const double *tw, double *log_ratio,
                             double *var, double *tau, int32_t *rc, double *pct, uint64_t *ws, uint32_t ws_groups, hipStream_t s);

// ---- post.hip: the summary over all chains (pool_kernels.h) and the summary kernels it reuses (post_kernels.h)
// k_proportions of the summary, unchanged: P[s * cnt + i] = X[s * stride + col_of(i)] / G[s * ng + gene_of[i]] (col_of null: the identity)
void launch_proportions(uint32_t cnt, uint32_t S, uint32_t stride, const double *X, const uint32_t *col_of, const uint32_t *gene_of, uint32_t ng,
                        const double *G, double *P, hipStream_t s);
// k_series_summary<., true> of the summary, unchanged, without percentiles, over count series X[series][S]: the per-chain columns of a
// slab X[series][chain][S] with count = series * chains.  ws: chain_columns_workspace_bytes(S) bytes (0: none needed)
int launch_chain_columns(uint32_t count, uint32_t S, const double *X, const double *tw, double *log_mean, double *var, double *tau, int32_t *rc,
                         uint64_t *ws, hipStream_t s);
size_t chain_columns_workspace_bytes(uint32_t S);
// k_pooled_summary over cnt series X[series][C][S]: in LDS while C S <= 8192, else in ws (PP words per workgroup, ws_groups workgroups).
// log mode: cm / cv / ct / crc [cnt][C] are the per-chain columns, results a = log_mean, b = var, c = tau, mcse2, rc;
// proportion mode: cm / cv / ct are scratch, multi [cnt], results a = mean, b = probit_mean, c = probit_sd
void launch_pooled_summary(bool log_mode, uint32_t cnt, uint32_t C, uint32_t S, const double *X, uint32_t np, const int32_t *pind, double *cm,
                           double *cv, double *ct, const int32_t *crc, const uint8_t *multi, double *a, double *b, double *c, double *mcse2,
                           int32_t *rc, double *pct, uint64_t *ws, uint32_t ws_groups, hipStream_t s);

} // namespace mmg
