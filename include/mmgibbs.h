/*
 * mmgibbs.h -- C ABI of libmmgibbs.so: the MI355X-native Gibbs hot path of mmseq.
 *
 * The reference (eturro/mmseq) has no in-process plugin / FFI boundary: the hot path is
 * the body of main() in src/mmseq.cpp.  This header is the boundary a maintainer would
 * bind instead of that body; each entry point cites the reference lines it replaces
 * (paths relative to the reference tree).  INTEGRATION.md shows the call sequence that
 * replaces src/mmseq.cpp:833-925 inside the reference's own main().
 *
 * Conventions: every function returns 0 on success, non-zero on error (message via
 * mmg_last_error(), thread-local).  No exceptions cross the boundary.  All host
 * buffers are caller-owned; handles own their device memory.  One handle is driven by
 * one host thread at a time.  There is NO CPU fallback: without a HIP device every
 * compute entry point fails with MMG_ERR_NO_DEVICE.
 */
#ifndef MMGIBBS_H
#define MMGIBBS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMG_ABI_VERSION 8
/* Version history of the SPEC behind the entry points: under one version a chain is a pure function of (problem, tx_order, seed,
 * chain, iteration); a bump means the same inputs may yield different bits (golden fixtures and the oracle move with it).
 *   3  (round 2) rows with 2 <= k <= 64 draw k categoricals (before: k <= 8), sorted by k inside their class.  The constant moved
 *      without a bump at the time; recorded here.
 *   4  (round 3) canonical row order: ties inside a key are broken by the CENTRE of the row -- the sum of its hits' offsets in the
 *      window its key names -- before the content hash, so that the 64 rows of a tile gather neighbouring window slots (LDS bank
 *      conflicts of the sample and EM kernels: -50 %).  The per-row random stream follows the stored position, so chains of
 *      problems stored in the canonical layout differ from version 3; MMG_LAYOUT_KEEP_ROWS problems (and the committed golden
 *      chain, which keeps its rows) do not.  The draw target is now specified as fma(x, t 2^-32, t 2^-33) (mmg_math.h:
 *      draw_target): the same real number rounded once, bit-identical to version 3 unless t 2^-33 underflows.
 *      EM (mmg_em_*): the LO limb of a term is the fraction of x 2^E truncated to sl bits (version 3: rounded to nearest through an
 *      fp64 addition); both limbs of a term are now shifts of the significand of x.  mu after a sweep may differ from version 3 in
 *      the last bit.
 *   5  (round 3) multiplicities: a row draws its k categoricals one by one not only for k <= MMG_K_SMALL but whenever
 *      k <= MMG_K_DRAWS_PER_HIT * (hits - 1): a draw costs about 1/22 of one step of the conditional-binomial chain, which has hits - 1
 *      steps whatever k (measured: 2 M rows of 20 hits with k = 65 in 0.32 instead of 1.9 ms per sweep, with k = 300 in 1.46 instead of
 *      2.0).  Rows above MMG_K_SMALL are
 *      ordered by a logarithmic bucket of k inside their class (a tile loops to its largest k).  Chains of problems with
 *      MMG_K_SMALL < k <= MMG_K_DRAWS_PER_HIT * (hits - 1) rows differ from version 4.  The committed golden chain
 *      (tests/golden/keyed_chain_tiny.json) has no such row and is byte for byte what it was; keyed_chain_k_draws.json was added for
 *      the new range.  Also version 4/5 (recorded late): a row with 2 <= k <= MMG_K_SMALL stored as k rows changes
 *      mmg_problem_info.m / mmg_problem_download (the STORED problem), the low bits of mmg_problem_start_values (k terms
 *      floor(2^52 / hits) instead of floor(k 2^52 / hits)) and of EM sweeps (k terms 1/d instead of one term k/d) of such problems.
 *   6  (round 4) a canonical problem WITHOUT tx_order whose rows do not fit LDS windows in the caller's numbering (modelled cost more
 *      than 1.25 x that of register-path tiles alone) gets a transcript order derived from the hit graph (order.hip; a pure function
 *      of the set of rows and the caller's numbering) when the model prices the result a fifth lower: stored order, and with it the
 *      chain, of exactly those problems differ from version 5 (they ran the CSR-tile kernel at 1/29 of the speed).  Problems with
 *      tx_order, kept rows, or locality in the caller's numbering are untouched.  New entry points: mmg_problem_shard_bounds_timed,
 *      mmg_selftest_gibbs_shards; mmg_problem_shard_bounds cuts by modelled cost instead of hits (any cut gives the same chain).
 *      Also version 6 (recorded late): the canonical layout's step 0 (rows with 2 <= k <= MMG_K_SMALL stored k times) is skipped when it
 *      would store more than 8 rows per uploaded row (LAYOUT_EXPAND_MAX_RATIO, layout.hip; oracle/binding.py mirrors it): such rows
 *      keep their k and draw their categoricals in the multiplicity kernel -- stored rows and chain bits of heavily collapsed problems
 *      differ from version 5.
 *   7  (round 5) tx_order with GROUPS: the high 32 bits of a key name the transcript's group (the CLI passes the gene, src/mmseq.cpp:
 *      337-357).  When a canonical problem built on the caller's keys does not fit LDS windows (modelled cost more than 1.25 x that of
 *      register-path tiles alone: reads that also hit paralogues, whose genes the caller's gene order puts anywhere) the library
 *      derives an order of the GROUPS from the group-level hit graph (order.hip, the machinery of version 6 on groups) and keeps the
 *      problem built on it -- the transcripts of a group stay together, in the caller's order -- if the model prices it a fifth lower.
 *      Stored order and chain of exactly those problems differ from version 6; keys whose high words are all equal (plain ranks) are
 *      untouched.  mmg_synth_desc gained gene_size / far_family (the struct grew: ABI 7); MMG_OPT_WIRE_CHECK; the first exchanges of an
 *      mmg_group are verified against the host's own reduction of the members' buffers.
 *   8  (round 6) multiplicities: a row draws its k categoricals one by one while k <= min(MMG_K_SMALL, MMG_K_DRAWS_PER_HIT * (hits - 1))
 *      (version 5: the LARGER of the two limits); above, the conditional-binomial chain.  The chain's rows are no longer drawn in the
 *      lane of a tile that owns them but from a list of their own, a lane per row running ahead of its neighbours (k_sample_bigk), at a
 *      third of the old cost per binomial; k categorical draws beyond 64 then cost more than the hits - 1 binomials they were meant to
 *      save (bench.py `heavy`: 0.74 -> 0.40 ms per sweep, `collapsed`: 0.30 -> 0.15, of which the new boundary is 0.21 and 0.11).
 *      Step 0 of the canonical layout follows the rule: the rows stored k times are the rows that draw categoricals (rows of ONE hit and
 *      empty rows are never stored twice: they need no draw).  Chains and stored rows of problems with rows of
 *      MMG_K_SMALL < k <= MMG_K_DRAWS_PER_HIT * (hits - 1), with k > MMG_K_DRAWS_PER_HIT * (hits - 1) on rows of 2-4 hits, or with
 *      k >= 2 on rows of one hit differ from version 7.  tests/golden/keyed_chain_tiny.json has no such row and is byte for byte what
 *      it was; keyed_chain_k_draws.json was regenerated for the new boundary (tools/gen_golden.py).  The conditional binomials themselves
 *      (mmg_math.h: binomial) are unchanged, uniform for uniform.  MMG_OPT_BIGK_PER_WAVE, MMG_OPT_BIGK_SIDE_STREAM.
 *      Also version 8: in the GROUP-level hit graph of version 7 a group that shares rows with more than max(32, 8 x the median) other groups
 *      is a hub (version 7: max(256, ...), the transcript-level rule) and stays out of the traversal -- a gene whose repeat-bearing UTR
 *      collects reads of hundreds of genes no longer ties the paralogue families into one component.  Stored order and chain of problems
 *      with such groups differ from version 7.
 *      Additive in version 8, no bump (the chain's specification does not change): mmcollapse (mmg_collapse_*), mmdiff (mmg_diff_*), the
 *      owners' self tests (MMG_OPT_FAIL_ALLOC, mmg_selftest_live, mmg_selftest_sampler_events), the convergence diagnostics across
 *      chains (mmg_convergence_*, MMG_OPT_CONV_SLAB), mmdiff's chains (mmg_diff_chains_*) and the posterior assignment probabilities
 *      of the hits (mmg_assign_*, MMG_OPT_ASSIGN_WAVES), and the posterior summary over the draws of all chains (mmg_pooled_*,
 *      MMG_OPT_POOL_SLAB), and the posterior correlation of pairs of transcripts (mmg_pairs_*, MMG_OPT_PAIRS_SLAB), and mmdiff's
 *      effect summaries (mmg_diff_effects_*, mmg_effects_*), and mmdiff's permutation null with its q-values (mmg_diff_perm_*,
 *      mmg_qvalues), and the self test of the streams' key space and of the scalar functions (mmg_selftest_keyed), and mmdiff's
 *      likelihood-ratio test (mmg_diff_lrt_*) with its permutation null (mmg_diff_lrt_perm_*), and the posterior fold change between
 *      two samples from all pairs of their draws (mmg_fold_*, MMG_OPT_FOLD_SLAB), and the posterior distances and correlations
 *      between samples from their joint draws (mmg_sim_*, MMG_OPT_SIM_CHUNK), and the pointwise self test of the binomial chain's
 *      three shortcuts (mmg_selftest_bigk_points), and the posterior isoform usage within groups of transcripts -- dominant-isoform
 *      probabilities and usage entropy (mmg_isoform_*, MMG_OPT_ISO_SLAB), and the extension of a finished run to twice its length
 *      (mmg_sampler_extend).
 *      mmg_sampler_create refuses chains beyond 2^24: the Gamma stream's key holds 24 bits of the chain index (the row stream all 32), so
 *      chain 2^24 + c would redraw mu from chain c's uniforms.  No chain that ran before is changed by the check. */
/* Layout.  The model does not care about the order of rows or the numbering of transcripts (src/mmseq.cpp:399-418 uses
 * first-seen order for both); the kernels do: they keep a window of consecutive transcripts in LDS and want the 64 rows of a
 * wave to have equal lengths.  mmg_problem_create therefore stores the rows in a CANONICAL order of its own (sorted on the
 * device by leading-transcript band, multiplicity class, length, row centre and a content hash -- a pure function of the set of rows, so
 * the chain does not depend on the order the caller happened to read them in) and, given tx_order, renumbers the transcripts
 * internally.  Every per-transcript array crossing this ABI stays in the CALLER's numbering; rows never cross it. */
#define MMG_LAYOUT_CANONICAL 0u /* default: rows re-ordered by the library                                      */
#define MMG_LAYOUT_KEEP_ROWS 1u /* rows kept as given (row i of the upload draws from random stream row_id_base + i):
                                   shards cut from an already canonical problem, tests of specific row orders    */

enum {
    MMG_OK = 0,
    MMG_ERR_ARG = 1,       /* invalid argument                                 */
    MMG_ERR_NO_DEVICE = 2, /* no usable HIP device (no fallback exists)        */
    MMG_ERR_HIP = 3,       /* a HIP runtime call failed                        */
    MMG_ERR_STATE = 4,     /* call sequence error (e.g. trace not kept)        */
    MMG_ERR_IO = 5
};

/* rows with k <= MMG_K_SMALL and k <= MMG_K_DRAWS_PER_HIT * (hits - 1) draw k categoricals; above either limit, a conditional-binomial
 * chain over the row's hits (one binomial per hit but the last, whatever k: src/mmseq.cpp:880's gsl_ran_multinomial).  The rows that
 * draw k >= 2 categoricals are stored k times by the canonical layout. */
#define MMG_K_SMALL 64u
#define MMG_K_DRAWS_PER_HIT 16u
/* chain indices (mmg_config.chain_base + the chain) fit 24 bits: that many enter the key of the Gamma stream */
#define MMG_MAX_CHAINS 16777216

typedef struct mmg_problem mmg_problem; /* device-resident CSR hit-set matrix M + k + l */
typedef struct mmg_sampler mmg_sampler; /* chains' state: mu, counts, trace, moments     */

/* Host description of the sparse problem: the reference's boolMat M (m x n), vector<int> k
 * and vector<double> l  (src/mmseq.cpp:117, :385, :593-608).  Rows are hit sets (or single
 * reads, k == NULL => all 1), columns the observed transcripts in first-seen order (:403);
 * within a row columns ascend (:412) -- the canonical layout sorts them itself, any order may be passed.
 * A column that occurs twice in a row counts twice (weight and pick): the reference's boolean matrix
 * cannot hold that case, its reader drops the second occurrence (:404-409) and so does the CLI of this
 * build; device and oracle agree on the list semantics (tools/fuzz_parity.py, `dups`). */
typedef struct mmg_problem_desc {
    uint64_t m;              /* rows                                                    */
    uint32_t n;              /* columns (observed transcripts)                          */
    const uint64_t *row_ptr; /* m+1 offsets into col_idx, row_ptr[0] == 0                */
    const uint32_t *col_idx; /* row_ptr[m] column indices                                */
    const uint32_t *k;       /* m multiplicities, or NULL for all ones                   */
    const double *l;         /* n: effective_length * mapped_reads / 1e9  (:603), > 0    */
    uint64_t row_id_base;    /* global index of stored row 0 (read-shard mode: the shard offset):
                                stored row i draws from random stream row_id_base + i      */
    uint32_t layout;         /* MMG_LAYOUT_*                                              */
    const uint64_t *tx_order;/* optional, n keys: transcripts are laid out on the device by ascending
                                (key, index).  A caller that knows which transcripts share reads (the
                                isoforms of a gene, src/mmseq.cpp:358) passes gene_ordinal << 32 | ordinal
                                within the gene, so that a read's hits are neighbours.  The high 32 bits of a key
                                name the transcript's GROUP: the library may reorder the groups (never the transcripts
                                inside one) when the rows do not fit LDS windows in the caller's group order -- reads
                                that also hit paralogues, spec version 7.  NULL: the caller's
                                numbering is the device numbering -- unless the rows do not fit LDS windows in it
                                (first-seen numbering, src/mmseq.cpp:399-408) and the layout is canonical: the library
                                then derives an order from the hit graph, a pure function of the set of rows
                                (spec version 6), and uses it like a caller's                 */
} mmg_problem_desc;

/* Synthetic problem generated directly into device CSR (no reference counterpart; the
 * benchmark inputs of BASELINE.md).  Every row is a pure function of (seed, row id). */
typedef struct mmg_synth_desc {
    uint64_t seed;        /* generator seed (1234 = reference default -seed)              */
    uint64_t rows;        /* rows generated on this device                                */
    uint64_t row0;        /* global id of the first row (shard offset)                    */
    uint32_t n;           /* transcripts                                                  */
    double avg_hits;      /* row length = min(100, 1 + Poisson(avg_hits - 1))             */
    int32_t uniform;      /* 0: hits inside a +-64 index window; 1: uniform over n        */
    int32_t sorted;       /* 1: canonical layout (MMG_LAYOUT_CANONICAL); 0: generator order kept
                             (a name-sorted BAM's order; MMG_LAYOUT_KEEP_ROWS)            */
    uint64_t mapped_reads;/* N in l = efflen * N / 1e9; 0 => rows                         */
    double far_fraction;  /* fraction of the rows (>= 2 hits) whose last drawn hit is replaced by a
                             transcript anywhere in [0, n): reads that also hit a paralogue */
    uint32_t gene_size;   /* 0: the band generator above.  G > 0 (ABI 7): GENE-BLOCK mode -- transcripts [gG, gG + G) are the isoforms of gene g
                             and the hits of a read lie inside its gene (row length <= G): what an aligner's output looks like, where
                             reads of different genes share nothing but paralogues (src/bam2hits.cpp:271-300)              */
    uint32_t far_family;  /* gene-block mode: 0 = a far hit goes anywhere (as above); F >= 2 = to an isoform of another gene of the read's
                             PARALOGUE FAMILY: the genes are grouped F at a time by a seeded bijection of the gene indices, so a family's
                             members lie anywhere in the transcriptome but are the same for every read of a gene                */
} mmg_synth_desc;

#define MMG_ORDER_SKIPPED 0x100
typedef struct mmg_problem_info {
    uint64_t m, nnz, total_k, row_id_base;
    uint32_t n;
    uint32_t max_row_len;
    uint64_t n_tiles;      /* tiles the sample kernel walks                               */
    uint64_t device_bytes; /* HBM held by the problem                                     */
    int32_t index_bits;    /* 32 or 64: width of the device row_ptr                       */
    int32_t sample_kernel; /* what mmg_sampler_sample launches: 2 k_sample_sell (sliced-ELL 8-bit stream; the default),
                              0 k_sample (32-bit CSR tiles: problems whose rows mostly span more than an LDS window) */
    uint64_t stream_bytes; /* bytes of the tile stream that kernel reads per launch (0 for kernel 0) */
    uint64_t fast_tiles;   /* sliced-ELL tiles walked from the register stream                               */
    uint64_t far_tiles;    /* sliced-ELL tiles with a far list (rows with hits outside the window); the rest
                              (n_tiles - fast - far - empty) are walked from the CSR                         */
    uint64_t padded_slots; /* hit slots of the sliced-ELL stream incl. padding (>= nnz of the fast tiles) */
    int32_t layout;        /* MMG_LAYOUT_* in force                                       */
    int32_t tx_renumbered; /* low byte -- 1: tx_order was given; 2: the library derived an order from the hit graph; 3: tx_order was given and
                              the library reordered its groups (the genes) by the group-level hit graph.  | MMG_ORDER_SKIPPED: such an order was
                              called for (spec versions 6 / 7) but the attempt could not be made -- it needs about 3 x the problem's device memory
                              free at the time, plus up to 4 GB -- or failed: the problem stands in the caller's order, and its chain is the one of
                              THAT order.  Under memory pressure a chain is therefore a pure function of (problem, tx_order, seed, chain,
                              iteration) AND of this flag; callers that need run-to-run identity check it (the CLI warns) */
    int32_t sample_grid;   /* workgroups of the sample kernel: the resident count (waves the runtime reports x CUs) times the
                              number of generations (1..16: tile ranges of about 24 tiles once the problem is large) */
    int32_t cu_count;
} mmg_problem_info;

/* Parameters of the Gibbs loop: alpha/beta are the Gamma prior (src/mmseq.cpp:184-185),
 * seed the reference's -seed (:203), gibbs_iter/trace_len as :190-192, :284. */
typedef struct mmg_config {
    double alpha, beta;
    uint64_t seed;
    int32_t n_chains;   /* independent chains advanced per sweep on this device (>= 1)   */
    int32_t chain_base; /* global index of chain 0 here (multi-device chains mode); >= 0,
                           chain_base + n_chains <= MMG_MAX_CHAINS                        */
    int32_t gibbs_iter; /* planned chain length; sample s kept when iter % (gibbs_iter/trace_len) == 0 (:911) */
    int32_t trace_len;  /* samples per chain: 1024 in the reference (:191)                */
    int32_t keep_trace; /* !=0: store the samples (n*trace_len doubles per chain); 0: moments only */
    int32_t timing;     /* N > 0: bracket the kernel launches of every N-th iteration with HIP events; 0: none */
} mmg_config;

typedef struct mmg_timing {
    double sample_ms, update_ms; /* sums of per-launch HIP-event durations                */
    uint64_t sample_launches, update_launches;
} mmg_timing;

const char *mmg_last_error(void);
int mmg_abi_version(void);
/* number of HIP devices visible (0 and MMG_OK when none). */
int mmg_device_count(int *count);

/* ---- problem ------------------------------------------------------------------------ */
/* Uploads M, k, l (src/mmseq.cpp:456-462, :582-608 produce them) to `device`. */
int mmg_problem_create(const mmg_problem_desc *desc, int device, mmg_problem **out);
int mmg_problem_create_synthetic(const mmg_synth_desc *desc, int device, mmg_problem **out);
int mmg_problem_info_get(const mmg_problem *p, mmg_problem_info *info);
/* The single-chain sample launch of a sliced-ELL problem (mmg_problem_info stays as ABI 8 laid it out; this is what it would have
 * gained): which instantiation of k_sample_sell runs, and how the launch's ranges are balanced by the cost model that cut them. */
typedef struct mmg_k1_info {
    int32_t lean;            /* 0: the general kernel; 1: the instantiation for lists of register-path and empty tiles only */
    int32_t fixed_walk;      /* straight-line walks for every group count up to 8 (fewer than 5 groups per tile on average) */
    int32_t range_tile_cost; /* v >= 1: the ranges price a register-path tile v + 1 per group of its block; 0: a constant (MMG_OPT_K1_RANGE_COST = 0) */
    int32_t reserved;
    uint64_t n_ranges;       /* ranges of the launch that hold work */
    uint64_t range_cost_max; /* the dearest range, in the model's units */
    double range_cost_mean;  /* over the n_ranges ranges (a launch of several generations ends in ranges of half the cost) */
    uint64_t range_tiles_max;/* tiles of the longest range */
    uint64_t n_list;         /* entries of the tile list the launch walks */
    uint64_t list_cost;      /* their modelled cost */
} mmg_k1_info;
int mmg_problem_k1_info_get(const mmg_problem *p, mmg_k1_info *info);
/* The ranges themselves: bound[0 .. n] (n = mmg_problem_info.sample_grid) are list entries, range c holds entries [bound[c], bound[c + 1]);
 * cum_cost[c] is the modelled cost of the entries in front of bound[c], cum_groups[c] the 256-byte groups of their blocks (whatever the
 * model).  The list is every tile in stored order -- unless the problem has tiles with multiplicities: then it is the list WITHOUT
 * them (they have a launch and ranges of their own), entry e is the e-th tile without multiplicities and bound[n] = mmg_k1_info.n_list
 * is their number, not the number of tiles; a problem whose every tile has multiplicities has the single empty entry (n_list = 1, cost 0).
 * Any may be NULL.  MMG_ERR_STATE without a sliced-ELL stream. */
int mmg_problem_k1_ranges(const mmg_problem *p, uint64_t *bound, uint64_t *cum_cost, uint64_t *cum_groups);
/* Copies the device CSR back in STORED order (row_ptr m+1 u64, col_idx nnz u32 in the caller's transcript numbering,
 * k m u32; any may be NULL): what a checker needs to replay the chain row by row -- stored row i walks its hits in the
 * returned order and draws from random stream row_id_base + i. */
int mmg_problem_download(const mmg_problem *p, uint64_t *row_ptr, uint32_t *col_idx, uint32_t *k);
/* Rows [lo, hi) of a stored problem as a problem of its own on `device`: a read shard (its rows draw from the random streams
 * row_id_base + lo + i, like the rows of the parent) or, with lo = 0 and hi = m, a replica for chains mode.  Cut on the parent's
 * device and copied device to device (peer copy); rows, hit order and transcript numbering stay as stored. */
int mmg_problem_shard(const mmg_problem *full, uint64_t lo, uint64_t hi, int device, mmg_problem **out);
/* Contiguous ranges of the stored rows of p for `parts` read shards: bounds[i] = first row of shard i, bounds[parts] = m.  The ranges
 * have (nearly) equal modelled COST of a sweep, not equal hit counts: the library knows what its tiles cost (a register-path tile by
 * the bytes of its block, a far tile three times that per far entry, multiplicity tiles by their draws), and the canonical order puts
 * every far row behind every near row -- the reference's static split of the rows (src/mmseq.cpp:864) would give the last devices the
 * expensive ones.  Boundaries are tile starts on even random-stream ids.  Problems on the CSR-tile kernel are cut by hits
 * (mmg_shard_bounds). */
int mmg_problem_shard_bounds(const mmg_problem *p, int parts, uint64_t *bounds);
/* The same cut by MEASURED cost: every candidate shard is run as what it will be -- the one-chain sample kernels over its interval of
 * p's tile lists, in ranges cut the way a problem of that size is cut, with replicated count vectors and the weights mu (n doubles, the
 * caller's numbering: the start values or the EM optimum) -- on p's device, timed with HIP events on the null stream; tiles of a shard
 * that ran long get dearer in proportion and the rows are cut again, until the slowest shard is within 2 % of the mean: at most 6
 * rounds of parts x 7 launches behind a 50 ms warm-up (0.09 s at 50 M reads, 0.2-0.3 s at 400 M).  What a model cannot know -- what a
 * far entry costs on this part, hit sets that give most of their reads to one transcript -- is in the measurement.  The chain does
 * not depend on where the rows are cut. */
int mmg_problem_shard_bounds_timed(const mmg_problem *p, const double *mu, int parts, uint64_t *bounds);
int mmg_problem_get_l(const mmg_problem *p, double *l);
/* Start values and the unique-hit column, src/mmseq.cpp:617-638: mu0[t] = sum_{i: t in row i}
 * k_i/|row i| / l[t]; unique_hits[t] = sum of k_i over rows {t} (bit-exact integer). Either
 * output may be NULL.  The shares are summed exactly (fixed point, 2^-52 resolution), so mu0 does not
 * depend on the order of the rows. */
int mmg_problem_start_values(const mmg_problem *p, double *mu0, int32_t *unique_hits);
/* EM to convergence from mu (in/out), src/mmseq.cpp:741-811: stop when the log-likelihood
 * gain <= epsilon or after max_iter sweeps. */
int mmg_problem_em(const mmg_problem *p, double *mu, int max_iter, double epsilon, int *iters,
                   double *loglik);

/* ---- EM, sweep by sweep (src/mmseq.cpp:741-811) ------------------------------------------
 * mmg_em_create uploads the start value and returns its log-likelihood (:745-754);
 * mmg_em_step performs one sweep of :761-806 and returns the new log-likelihood, so the caller
 * owns the loop, its stopping rule (:761) and its per-iteration output (:762-768).  mu stays on
 * the device between sweeps; mmg_em_get_mu downloads it (n doubles).  The sums are accumulated
 * exactly (fixed point, integer atomics): results do not depend on the traversal order. */
typedef struct mmg_em mmg_em;
int mmg_em_create(const mmg_problem *p, const double *mu0, mmg_em **out, double *loglik0);
int mmg_em_step(mmg_em *e, double *loglik);
int mmg_em_get_mu(mmg_em *e, double *mu);
/* sweeps done, rows passes repeated on measured scale exponents, rows-pass kernel (2 sliced-ELL stream,
 * 1 16-bit tile stream, 0 row per thread from the CSR) */
int mmg_em_stats(const mmg_em *e, int *sweeps, int *repeated_passes, int *stream_kernel);
void mmg_em_destroy(mmg_em *e);
/* Samplers and EM handles created from a problem must be destroyed before the problem. */
void mmg_problem_destroy(mmg_problem *p);

/* ---- sampler ------------------------------------------------------------------------ */
/* mu0: n doubles (every chain starts there, like mu = EM optimum at src/mmseq.cpp:820). */
int mmg_sampler_create(const mmg_problem *p, const mmg_config *cfg, const double *mu0, mmg_sampler **out);
/* Launch on a caller-owned hipStream_t (e.g. the framework's current stream) instead of
 * the sampler's own stream.  NULL restores the own stream (a non-blocking stream: NOT ordered against the legacy
 * default stream); to run on the legacy default stream itself pass hipStreamLegacy, (void *)1. */
int mmg_sampler_set_stream(mmg_sampler *s, void *hip_stream);
/* n_iter full Gibbs iterations = src/mmseq.cpp:851-918 (sample+scatter, gamma redraw,
 * trace capture), enqueued asynchronously. */
int mmg_sampler_run(mmg_sampler *s, int n_iter);
/* Turns a run that has reached its planned end into the first half of a run of twice the length.  A chain is a function of (problem,
 * seed, chain, iteration) alone and gibbs_iter enters only the thinning gibbs_iter / trace_len, so the samples a run of 2 gibbs_iter
 * keeps from its first half are every second sample of this run: for every chain, trace row j becomes row 2 j (j < trace_len / 2),
 * rows trace_len / 2 .. trace_len - 1 become +0.0 as in a new sampler, the moment sums are added up again from the kept rows in sample
 * order, the configuration's gibbs_iter doubles and the number of kept samples becomes trace_len / 2.  The iteration, mu, the counts
 * and the timing sums stay; mmg_sampler_run continues and the next kept sample is row trace_len / 2.
 * IDENTITY: after mmg_sampler_extend and gibbs_iter more iterations (the value before the call), the trace, the moments, mu, the counts
 * and the iteration equal, bit for bit, those of a sampler created with 2 gibbs_iter and run to its end -- and so at every iteration
 * in between.
 * MMG_ERR_ARG: trace_len odd; gibbs_iter >= 2^30 (twice its value must fit the configuration's int32).  MMG_ERR_STATE: created with
 * keep_trace == 0; between mmg_sampler_sample and mmg_sampler_update; the planned run is not complete (iteration == gibbs_iter and all
 * trace_len samples kept).  The argument rules are checked first.  The call waits for the sampler's stream, allocates a scratch buffer
 * of 8 n trace_len / 2 bytes (a failure leaves the sampler untouched) and has completed on the device when it returns.
 * A summary begun (mmg_summary_begin) before the call holds rows of samples that no longer exist: its mmg_summary_advance / _finish /
 * _get_rows return MMG_ERR_STATE from then on.  The handles made from a full trace (mmg_fold_*, mmg_pairs_*, mmg_assign_*) refuse the
 * sampler until its trace is full again.  The samplers of a group must be extended alike (the group calls compare gibbs_iter and the
 * kept samples). */
int mmg_sampler_extend(mmg_sampler *s);
/* The two halves of one iteration, for read-shard mode where the caller all-reduces the
 * counts in between:  sample = :857-891 (+ :887 column sums), update = :905-917. */
int mmg_sampler_sample(mmg_sampler *s);
int mmg_sampler_update(mmg_sampler *s);
/* Device pointers for collectives: counts int32 [n_chains][n]; moments double
 * [2][n_chains][n] (sum log mu, sum log^2 mu over kept samples).  Element t of these buffers is DEVICE transcript t
 * (mmg_problem_tx_perm); ranks that passed the same tx_order agree on it, which is all a sum needs. */
int mmg_sampler_counts_devptr(mmg_sampler *s, void **ptr, uint64_t *count);
int mmg_sampler_moments_devptr(mmg_sampler *s, void **ptr, uint64_t *count);
int mmg_sampler_sync(mmg_sampler *s);
/* Wait until the first n_done iterations (n_done <= mmg_sampler_iteration) have completed on the device -- not for what is enqueued
 * behind them.  The reference prints sample s inside its loop (src/mmseq.cpp:911-917); a caller that streams the trace out enqueues
 * the next stretch of iterations, THEN waits for the previous one and fetches its rows (mmg_sampler_get_trace_rows_done), so the device
 * does not idle while the host formats.  An event follows the iteration that stored sample 16 j - 1 (j = 1, 2, ...) and the last sample;
 * other values of n_done wait for the next such iteration (or the whole stream when there is none). */
int mmg_sampler_wait_iterations(mmg_sampler *s, int n_done);
int mmg_sampler_iteration(const mmg_sampler *s, int *iter);
/* Trace of one chain, transcript-major exactly like mu_trace at src/mmseq.cpp:914:
 * out[t*trace_len + s]. */
int mmg_sampler_get_trace(mmg_sampler *s, int chain, double *out);
/* Same samples, sample-major (the row order of .trace_gibbs.gz, :912-916): out[s*n + t]. */
int mmg_sampler_get_trace_rows(mmg_sampler *s, int chain, int first_sample, int n_samples, double *out);
/* The same rows for samples the device has FINISHED (the caller synchronised after the iteration that produced the last of them):
 * copied on a stream of their own, without waiting for -- or delaying -- iterations enqueued behind those samples.  May be called
 * from another thread than the one driving the sampler: the trace writers of src/mmseq.cpp:911-917 print sample s inside the loop,
 * right after iteration s * gibbs_ss; this is how a caller does the same while the device runs on. */
int mmg_sampler_get_trace_rows_done(mmg_sampler *s, int chain, int first_sample, int n_samples, double *out);
int mmg_sampler_get_mu(mmg_sampler *s, int chain, double *mu);
/* Xcolsum of the last completed iteration (src/mmseq.cpp:896-899). */
int mmg_sampler_get_counts(mmg_sampler *s, int chain, int32_t *cnt);
int mmg_sampler_get_moments(mmg_sampler *s, int chain, double *sum_log, double *sum_log2, int64_t *n_samples);
int mmg_sampler_get_timing(mmg_sampler *s, mmg_timing *t);
int mmg_sampler_reset_timing(mmg_sampler *s);
void mmg_sampler_destroy(mmg_sampler *s);

/* ---- posterior summary of the resident trace ---------------------------------------------------
 * Everything src/mmseq.cpp:927-1363 derives from mu_trace, computed where the trace lives: simulated traces of isoforms
 * without hits (:971-978), trace sums over sets of identical transcripts and over genes (:927-1008), proportions of gene
 * expression (:1014-1031), and per series the percentiles (:1110-1192), the mean of the logged trace (:1195-1227), Sokal's
 * variance / autocorrelation time of the logged trace (:1307-1363, src/sokal.cc:33-87) and the proportion summaries
 * (:1235-1305).  The host downloads summary columns and, for the trace writers (:1033-1108), sample rows. */
typedef struct mmg_summary mmg_summary;
typedef struct mmg_summary_desc {
    int32_t chain;
    /* isoforms that received no hit: trace v is Gamma(alpha) * virtual_scale[v] keyed (seed, id virtual_id[v], sample), :974 */
    uint32_t n_virtual;
    const uint64_t *virtual_id;
    const double *virtual_scale;
    /* groups whose trace is the sum of their members' traces, members added in the given order; a member < n is the caller's
     * transcript, n + v is virtual transcript v */
    uint32_t n_identical;            /* sets of identical transcripts, :927-945 */
    const uint64_t *identical_ptr;   /* n_identical + 1 offsets into identical_member */
    const uint32_t *identical_member;
    uint32_t n_genes;                /* genes, :947-1008; a transcript's proportion is relative to the gene that lists it */
    const uint64_t *gene_ptr;
    const uint32_t *gene_member;
    uint32_t n_percentiles;          /* positions in the sorted trace, round(p / 100 * (trace_len - 1)), :1111-1114 */
    const int32_t *percentile_index;
} mmg_summary_desc;
enum { MMG_SERIES_TRANSCRIPT = 0, MMG_SERIES_VIRTUAL = 1, MMG_SERIES_IDENTICAL = 2, MMG_SERIES_GENE = 3 };
/* Any trace_len: a series is sorted and Fourier-transformed in LDS up to 8192 samples (the reference's trace length is 1024,
 * src/mmseq.cpp:190) and in a global workspace beyond (the same steps, slower).  Sokal's estimator needs a power of two in
 * [4, 2^21] (src/sokal.cc:36-39); for other lengths the percentiles and means exist and sokal_rc says why var / tau do not. */
int mmg_summary_create(mmg_sampler *s, const mmg_summary_desc *d, mmg_summary **out);
/* The same in steps, for a caller that prints the trace files while the chain runs (src/mmseq.cpp:911-917 prints sample s inside the
 * loop): _begin checks and uploads the description and draws the simulated traces (the chain may be running: its trace is not read);
 * _advance computes the derived rows of the samples [done, samples_done) -- the caller vouches that the chain has finished them (it
 * synchronised after iteration samples_done * gibbs_iter / trace_len - 1); mmg_summary_get_rows serves rows below samples_done;
 * _finish, once every sample is in, computes the summary columns.  The summary works on a stream of its own: it neither waits for nor
 * delays iterations enqueued behind the samples it reads.  One thread at a time drives _advance / _finish; mmg_summary_get_rows may be
 * called from several threads for rows already advanced. */
int mmg_summary_begin(mmg_sampler *s, const mmg_summary_desc *d, mmg_summary **out);
int mmg_summary_advance(mmg_summary *q, int samples_done);
int mmg_summary_finish(mmg_summary *q);
/* Per series of `kind` (n, n_virtual, n_identical or n_genes of them): mean of the logged trace, Sokal's var and tau of the
 * logged trace with its return code (0; 200 / 201 when trace_len is no power of two >= 4: var = tau = 0), and the
 * n_percentiles order statistics of the trace itself, [series][percentile].  Any output may be NULL. */
int mmg_summary_get(mmg_summary *q, int kind, double *log_mean, double *var, double *tau, int32_t *sokal_rc, double *percentiles);
/* Proportions of gene expression, kind MMG_SERIES_TRANSCRIPT or MMG_SERIES_VIRTUAL: mean proportion, mean and sd of the probit
 * of the proportion clamped to [1e-9, 1 - 1e-9] (+inf terms for the only transcript of its gene, as at :1243-1262), percentiles. */
int mmg_summary_get_proportions(mmg_summary *q, int kind, double *mean_prop, double *mean_probit, double *sd_probit, double *percentiles);
/* Sample rows of the derived traces as the trace writers print them: out[r * width + i], r over [first_sample, first_sample +
 * n_samples).  MMG_SERIES_IDENTICAL / MMG_SERIES_GENE: the summed traces; MMG_SERIES_TRANSCRIPT: the proportions (width n). */
int mmg_summary_get_rows(mmg_summary *q, int kind, int first_sample, int n_samples, double *out);
void mmg_summary_destroy(mmg_summary *q);

/* ---- convergence across chains ------------------------------------------------------------------------------------------
 * Per series the rank-normalized split R-hat and the bulk and tail effective sample sizes (Vehtari et al. 2021, as Stan and ArviZ
 * report them; DESIGN.md section 11 states the definitions): every chain is cut in two halves (for odd trace lengths the middle draw is
 * dropped), the pooled draws are ranked (ties: average rank) and mapped to normal scores.  rhat = fmax(R-hat of the scores, R-hat of
 * the scores of the draws folded about the median); ess_bulk = ESS of the scores; ess_tail = fmin(ESS of I[x <= q05], ESS of
 * I[x <= q95]).  NaN for a series whose draws are all equal.  Reruns are bit-identical.  Additive in ABI version 8. */
typedef struct mmg_convergence mmg_convergence;
/* After the chain (the call synchronises with the sampler, then works on a stream of its own and touches nothing of the sampler):
 * every chain's trace of the sampler (keep_trace, trace_len >= 4), the series of every kind of mmg_summary_desc -- transcripts,
 * isoforms without hits (simulated per chain: keyed (seed, chain c, id, sample)), identical sets and genes (sums of the members in the
 * given order over chain c).  d->chain and the percentiles are ignored.  The results are kept on the host; no device memory is held
 * after the call. */
int mmg_convergence_create(mmg_sampler *s, const mmg_summary_desc *d, mmg_convergence **out);
/* rhat, ess_bulk, ess_tail of the series of `kind` (MMG_SERIES_*), in the numbering of mmg_summary_get; any output may be NULL */
int mmg_convergence_get(mmg_convergence *h, int kind, double *rhat, double *ess_bulk, double *ess_tail);
void mmg_convergence_destroy(mmg_convergence *h);
/* The same diagnostics of `count` series of traces from the host: traces[(c * S + s) * count + i] is draw s of chain c of series i. */
int mmg_convergence_of_traces(int device, uint32_t n_chains, uint32_t S, uint32_t count, const double *traces, double *rhat, double *ess_bulk,
                              double *ess_tail);

/* ---- the posterior summary over all chains ----------------------------------------------------------------------------------
 * What mmg_summary_* computes from one chain, from the N = n_chains * trace_len draws of every chain of a sampler (DESIGN.md section 14
 * states the definitions, tests/pooled_ref.py restates them).  With m_c, var_c, tau_c, rc_c the columns mmg_summary_get returns for
 * chain c alone (S = trace_len, sums over the chains in ascending order, every operation rounded once):
 *   log_mean = (sum m_c) / C;   var = ((S - 1) sum var_c + S sum (m_c - log_mean)^2) / (N - 1), the sample variance of the N logged draws;
 *   mcse2 = (sum tau_c var_c) / S / (C C), the variance of the mean of C independent chain means;   tau = (sum tau_c var_c) / (sum var_c);
 *   rc = the first non-zero rc_c, else 0; with rc != 0, tau = mcse2 = 0.  One chain: its own columns, copied, mcse2 = tau_0 var_0 / S.
 *   percentiles: the order statistics of the N pooled draws at positions in [0, N) (NaN outside), NaNs last.
 * Proportions: mean = (sum over all N draws) / N, the probit mean and sd over the N draws, each chain's sums taken in sample order and
 * added over the chains; percentiles of the pooled proportions.  Reruns are bit-identical.  Additive in ABI version 8. */
typedef struct mmg_pooled mmg_pooled;
/* After the chain (the call synchronises with the sampler, then works on a stream of its own and touches nothing of the sampler): every
 * chain's trace of the sampler (keep_trace; MMG_ERR_ARG without), the series of every kind of mmg_summary_desc as mmg_convergence_create
 * builds them (isoforms without hits simulated per chain, keyed (seed, chain c, id, sample)).  d->chain is ignored; d->percentile_index
 * are positions in [0, n_chains * trace_len).  The results are kept on the host; no device memory is held after the call. */
int mmg_pooled_create(mmg_sampler *s, const mmg_summary_desc *d, mmg_pooled **out);
/* The pooled columns of the series of `kind` (MMG_SERIES_*), in the numbering of mmg_summary_get; percentiles [series][percentile];
 * any output may be NULL */
int mmg_pooled_get(mmg_pooled *h, int kind, double *log_mean, double *var, double *tau, double *mcse2, int32_t *rc, double *percentiles);
/* The columns of chain `chain` alone: what mmg_summary_get returns for a summary of that chain (for the isoforms without hits and the
 * groups that contain them: of the traces simulated for that chain) */
int mmg_pooled_get_chain(mmg_pooled *h, int kind, int chain, double *log_mean, double *var, double *tau, int32_t *rc);
/* kind MMG_SERIES_TRANSCRIPT or MMG_SERIES_VIRTUAL, as mmg_summary_get_proportions */
int mmg_pooled_get_proportions(mmg_pooled *h, int kind, double *mean_prop, double *mean_probit, double *sd_probit, double *percentiles);
void mmg_pooled_destroy(mmg_pooled *h);
/* The pooled log columns of `count` series of traces from the host: traces[(c * S + s) * count + i] is draw s of chain c of series i;
 * pind: np positions in [0, n_chains * S); percentiles [series][np]; any output may be NULL.  MMG_ERR_ARG for n_chains == 0 or S == 0. */
int mmg_pooled_of_traces(int device, uint32_t n_chains, uint32_t S, uint32_t count, const double *traces, uint32_t np, const int32_t *pind,
                         double *log_mean, double *var, double *tau, double *mcse2, int32_t *rc, double *percentiles);
/* Device memory mmg_pooled_create held while it ran (all of it from the first launch to the last).  With C chains of S samples, the counts
 * n, nv, ni, ng of the four kinds, np percentiles, cap = max(1, min(max count, 256 MiB / (8 C S), MMG_OPT_POOL_SLAB if set)) series per
 * slab and L the largest number of gene members the genes of one slab of transcripts (or of isoforms without hits) list:
 *   16 max(nv, 1) + 8 (ni + 1 | 1) + 4 max(members of the sets, 1) + 8 (ng + 1 | 1) + 4 max(members of the genes, 1)    the description
 *   + 8 C S max(nv, 1)                                                                                              the simulated traces
 *   + 8 cap C S + 16 cap S                                                                  a slab, its group sums and its proportions
 *   + 8 (cap + 1) + 4 max(L, 1) + 5 cap                                                                      the slab's genes and flags
 *   + 28 cap C + 36 cap + 8 cap max(np, 1) + 4 max(np, 1) + 16 max(S, 1)            the chains' columns, the results, the twiddle table
 *   + (S > 8192: 24 * 1024 SP, SP = S rounded up to a power of two) + (C S > 8192: 8 PP min(1024, cap, max(1, 256 MiB / (8 PP)))). */
int mmg_pooled_device_bytes(mmg_pooled *h, uint64_t *bytes);

/* ---- several GPUs of one node, one process (RCCL over xGMI) ----------------------------------------
 * The reference parallelises with OpenMP threads inside one process (src/mmseq.cpp:834-838, :864); here the unit is a device.
 * A group owns one RCCL communicator per device (ncclCommInitAll); sampler i of every call below must live on device i of the
 * group.  RCCL is loaded on first use. */
typedef struct mmg_group mmg_group;
int mmg_group_create(const int *devices, int n, mmg_group **out);
int mmg_group_size(const mmg_group *g, int *n);
void mmg_group_destroy(mmg_group *g);
/* Read-shard mode: the samplers hold contiguous ranges of the stored rows of ONE chain (same seed, chain_base, iteration;
 * row_id_base = offset of the range).  n_iter iterations of: sample on every device (:857-891), ncclAllReduce(int32, sum) of
 * the count vectors in place (:896-899 across devices), the identical update everywhere (:905-917).  Asynchronous, like
 * mmg_sampler_run; the chain equals the chain of the unsharded problem bit for bit. */
int mmg_group_run_sharded(mmg_group *g, mmg_sampler *const *samplers, int n_iter);
/* Chains mode: every sampler advances its own chains (distinct chain_base) by n_iter iterations; nothing is exchanged. */
int mmg_group_run_chains(mmg_group *g, mmg_sampler *const *samplers, int n_iter);
/* Both run calls drive every device from its own host thread (thread i binds device i and enqueues its kernels and collectives
 * in order).  Host time the slowest of them spent per iteration in the last run call, in microseconds: what a device waits
 * for between iterations when its kernels are shorter than that. */
int mmg_group_enqueue_us(const mmg_group *g, double *us_per_device_iteration);
/* ncclAllReduce(fp64, sum) of the posterior moments over the devices (into scratch buffers: the samplers keep their own moments,
 * the call may be repeated), then summed over the chains of a device: sum_log[n], sum_log2[n] (caller's numbering) over n_samples
 * kept samples of all chains. */
int mmg_group_pool_moments(mmg_group *g, mmg_sampler *const *samplers, double *sum_log, double *sum_log2, int64_t *n_samples);
/* EM (src/mmseq.cpp:741-811) over read shards: shards[i] on device i holds a contiguous range of the stored rows.  Every phase of a
 * sweep runs on every device, then xe (max), the exact fixed-point accumulators with the log-likelihood limbs (uint64 sums) and,
 * once, the hits per transcript are all-reduced: integer sums, so every device holds the bits the unsharded EM produces, takes the
 * same repeat decisions and applies the same update.  ems[0..G) are returned; step and read ems[0] with mmg_em_step /
 * mmg_em_get_mu, destroy every member with mmg_em_destroy. */
int mmg_group_em_create(mmg_group *g, const mmg_problem *const *shards, const double *mu0, mmg_em **ems, double *loglik0);
/* Host helper: contiguous row ranges of (nearly) equal hit counts for `parts` shards: bounds[i] = first row of part i (even),
 * bounds[parts] = m. */
int mmg_shard_bounds(const uint64_t *row_ptr, uint64_t m, int parts, uint64_t *bounds);

/* int_of_ext[t] = device index of the caller's transcript t (identity without tx_order). */
int mmg_problem_tx_perm(const mmg_problem *p, uint32_t *int_of_ext);

/* ---- host-side keyed draws ------------------------------------------------------------ */
/* out[i] = Gamma(shape, scale) from the keyed stream (seed, tag SIMU, id, i): the simulated traces
 * of isoforms without hits, src/mmseq.cpp:971-978 (which uses rg[0] there).  Pure host code. */
int mmg_host_gamma_trace(uint64_t seed, uint64_t id, double shape, double scale, int n, double *out);

/* ---- self-test hooks (used by tests only) ------------------------------------------- */
/* Process-wide overrides of choices the library normally makes itself, so that tests can reach every kernel on small
 * inputs.  They never change a result.  value < 0 restores the default. */
enum {
    MMG_OPT_SAMPLE_KERNEL = 0,     /* 0: k_sample (CSR tiles), 2: k_sample_sell even if few tiles qualify            */
    MMG_OPT_FORCE_IDX64 = 1,       /* 1: 64-bit device row offsets regardless of nnz                                 */
    MMG_OPT_SELL_WAVES_PER_CU = 2, /* cap on resident single-wave workgroups per CU (long tile ranges on small inputs) */
    MMG_OPT_EM_KERNEL = 3,         /* 0: row-per-thread EM kernel, 2: sliced-ELL EM kernel                           */
    MMG_OPT_EM_GRID = 4,           /* cap on the EM kernel's grid                                                    */
    MMG_OPT_FUSE_CHAINS = 5,       /* chains advanced per K1 launch: 1 (never fuse), 2 (the default), 4              */
    MMG_OPT_CNT_REPLICAS = 6,      /* 1: one global count vector per chain, 8: replicated (default: by ranges per band) */
    MMG_OPT_GROUP_FAIL = 7,        /* v >= 0: member v % size of a group fails in its second iteration of the next run call (error path) */
    MMG_OPT_DERIVE_ORDER = 8,      /* 0: never derive a transcript order from the hit graph, 1: try it on every canonical problem without tx_order */
    MMG_OPT_WIRE_CHECK = 9,        /* 0: no verification of a group's first exchanges, 1: verify in groups of one device too, 2: 1 + damage a word behind the exchange (the failure path) */
    MMG_OPT_BIGK_PER_WAVE = 10,    /* list entries per workgroup of k_sample_bigk (the rows on the conditional-binomial chain)                      */
    MMG_OPT_BIGK_SIDE_STREAM = 11, /* 0: k_sample_bigk on the sampler's stream, in front of the tile kernels instead of beside them                    */
    MMG_OPT_FAIL_ALLOC = 12,       /* v >= 0: the v-th acquisition of device memory, a stream or an event after this option is set (counted from 0) fails
                                      without reaching the runtime (error paths) */
    MMG_OPT_CONV_SLAB = 13,        /* v >= 1: at most v series per slab of mmg_convergence_create / _of_traces (slab edges on small inputs)     */
    MMG_OPT_DIFF_TRACE_ROWS = 14,  /* v >= 1: at most v rows per row buffer of mmg_diff_trace_open (shortened traced launches on small inputs)    */
    MMG_OPT_ASSIGN_WAVES = 15,     /* v >= 1: at most v waves per launch of mmg_assign_run_* (several scratch chunks on small inputs)             */
    MMG_OPT_CONTRAST_SLAB = 16,    /* v >= 1: at most v contrasts per slab of mmg_contrast_create / _of_traces (slab edges on small inputs)      */
    MMG_OPT_POOL_SLAB = 17,        /* v >= 1: at most v series per slab of mmg_pooled_create / _of_traces (slab edges on small inputs)          */
    MMG_OPT_PAIRS_SLAB = 18,       /* v >= 1: at most v pairs per slab of mmg_pairs_create / _of_traces (slab edges on small inputs)             */
    MMG_OPT_FOLD_SLAB = 19,        /* v >= 1: at most v features per slab of mmg_fold_create / _of_traces (slab edges on small inputs)           */
    MMG_OPT_SIM_CHUNK = 20,        /* v >= 1: v features per chunk of mmg_sim_run's Gram kernel (chunk edges on small inputs; read by mmg_sim_create) */
    MMG_OPT_ISO_SLAB = 21,         /* v >= 1: at most v groups per slab of mmg_isoform_create / _of_traces (slab edges on small inputs)          */
    MMG_OPT_K1_LEAN = 22,          /* k_sample_sell's instantiation for lists of register-path and empty tiles only, read by mmg_problem_create*: 0 never,
                                      1 forced -- refused with MMG_ERR_ARG for a problem
                                      that has far, CSR-walked or multiplicity tiles; default: wherever the list allows it */
    MMG_OPT_K1_RANGE_COST = 23,    /* 0: the ranges of the k = 1 launches cut by a constant per tile, as before the tiles were priced by their groups;
                                      v >= 1: a register-path tile priced v + 1 per group of its block (the A/B of the ratio; default 6) */
    MMG_OPT_K1_RANGES = 24,        /* v >= 1: at most v ranges (workgroups) per launch over a tile list (mmg_selftest_k1_lists names the five), one generation,
                                      no tapered end (long ranges on small inputs) */
    MMG_OPT_SERIES_GROUPS = 25,    /* v >= 1: at most v workgroups per launch of a workspace instantiation of k_series_summary, k_convergence,
                                      k_pooled_summary and k_contrast_summary (a workgroup walks several series on small inputs).  The workspaces
                                      keep their size: every *_device_bytes formula holds as stated.  Under the option such a launch also
                                      starts from result columns of 0xFF bytes: a series no workgroup reached reads NaN, return code -1 */
    MMG_OPT_COUNT_ = 26
};
int mmg_selftest_option(int option, int value);
/* The last launch in this process of a workspace instantiation (the series too long for LDS: S > 8192, or C S > 8192) of kernel 0:
 * k_series_summary (mmg_summary_finish, mmg_collapse_summarize, the chains' columns of mmg_pooled_*), 1: k_convergence, 2: k_pooled_summary,
 * 3: k_contrast_summary -- *grid workgroups walked *count series.  Recorded on the host where the launch is made; zeros before any such
 * launch.  MMG_ERR_ARG for another kernel or a NULL pointer.  (Tests: MMG_OPT_SERIES_GROUPS reached the launch.) */
int mmg_selftest_series_launch(int kernel, uint32_t *grid, uint32_t *count);
/* What the library holds: counts[3] = device buffers, streams, events (tests: every call gives back what it acquired). */
int mmg_selftest_live(int64_t *counts);
/* A sampler's pool of timing events: *pool events, *free_idx of them on the free list, *pending_idx in pairs not yet harvested
 * (tests: pool == free_idx + pending_idx between calls). */
int mmg_selftest_sampler_events(const mmg_sampler *s, int *pool, int *free_idx, int *pending_idx);
/* The sharded EM of mmg_group_em_create with every shard on ONE device and the exchange done by plain kernels: `sweeps` sweeps from
 * mu0, mu (caller's numbering), the log-likelihood and the number of repeated passes -- the same bits as mmg_problem_em on the
 * unsharded problem. */
int mmg_selftest_em_shards(const mmg_problem *const *shards, int n_shards, const double *mu0, int sweeps, double *mu, double *loglik,
                           int *repeated_passes);
/* The sharded chain of mmg_group_run_sharded with every shard on ONE device and the count exchange done by a plain kernel: n_iter
 * iterations of sample on every shard (src/mmseq.cpp:857-891), the count vectors summed over the shards into every sampler
 * (:896-899), the identical update everywhere (:905-917) -- the same bits as mmg_sampler_run on the unsharded problem.  With
 * cfg.timing set, mmg_sampler_get_timing of sampler i reports what shard i's sample kernels took. */
int mmg_selftest_gibbs_shards(mmg_sampler *const *samplers, int n_shards, int n_iter);
/* What the HIP runtime reports about the k == NULL sliced-ELL sample kernel on `device`: registers, LDS and scratch bytes per
 * thread, and resident 64-thread workgroups per CU (hipOccupancyMaxActiveBlocksPerMultiprocessor). */
int mmg_selftest_kernel_info(int device, int *vgprs, int *lds_bytes, int *scratch_bytes, int *resident_per_cu);
/* The same about the instantiation the single-chain launch of a problem with 32-bit offsets runs for (lean, fixed_walk) as
 * mmg_k1_info reports them. */
int mmg_selftest_k1_kernel_info(int device, int lean, int fixed_walk, int *vgprs, int *lds_bytes, int *scratch_bytes, int *resident_per_cu);
/* The five tile lists a sample call of the problem can launch over -- 0: the main list (with multiplicity tiles: the list without them,
 * as mmg_problem_k1_ranges), 1: the tiles with multiplicities, 2 / 3: the register-path tiles of chains in pairs / in fours, 4: the far
 * and CSR-walked tiles of paired chains -- out[3 * i + 0 .. 2] = entries of list i, its ranges, the entries of its longest range; all 0
 * for a list the problem does not have (and without a sliced-ELL stream).  MMG_OPT_K1_RANGES = v caps the ranges of every one at v. */
int mmg_selftest_k1_lists(const mmg_problem *p, uint64_t *out);
/* Evaluates the library's own log / exp / sqrt / 1/x on x[0..n) (device >= 0: in a kernel
 * on that device; device == -1: the host instantiation of the same inline code). */
int mmg_selftest_math(int device, int64_t n, const double *x, double *out_log, double *out_exp,
                      double *out_sqrt, double *out_rcp);
/* out[0..4) = Philox4x32-10(ctr[4], key[2]); out[4..6) = Philox2x32-10(ctr[0..2), key[0]). */
int mmg_selftest_philox(int device, const uint32_t *ctr, const uint32_t *key, uint32_t *out);
/* out[i] = shape-`shape` gamma draw of stream (seed, chain 0, iter 0, id i) times scale. */
int mmg_selftest_gamma(int device, uint64_t seed, double shape, double scale, int64_t n, double *out);
/* out[i] = Binomial(nn, p) draw of row stream (seed, id i). */
int mmg_selftest_binomial(int device, uint64_t seed, uint32_t nn, double p, int64_t n, uint32_t *out);
/* n_cases BTRS attempts over n log-uniform in [n_lo, n_hi] (21 <= n_lo <= n_hi < 2^32) and p log-uniform in [10 / n, 1/2]: counts[0] attempts that
 * reach the exact acceptance test, [1] of them decided by the fp32 estimate k_sample_bigk tries first (mmg_math.h: btrs_pretest), [2] decided
 * AND different from the fp64 test -- must be 0 --, [3] accepted by the fp64 test, [4] the largest |estimate - fp64 difference| seen, in
 * millionths of the estimate's own error bound (counts: 5 words). */
int mmg_selftest_btrs_pretest(int device, uint64_t seed, int64_t n_cases, double n_lo, double n_hi, uint64_t *counts);

/* Diagnostics: the same for the inversion (n p < 10): n_cases searches, n log-uniform in [n_lo, n_hi] (1 <= n_lo), n p log-uniform in
 * [1e-6, 10), through the fp32 search k_sample_bigk tries first (mmg_math.h: binv_pretest) and the fp64 search of the sequential code.
 * counts[0] cases, [1] decided in fp32, [2] decided AND different from the fp64 search -- must be 0 --, [3] cases whose fp64 search ran off
 * the end (the sequential code draws again), [4] the sum of the outcomes (counts: 5 words).  slack scales the error bound the fp32 search
 * allows itself: 1 is what the sampler runs; smaller values show how much room the bound has. */
int mmg_selftest_binv_pretest(int device, uint64_t seed, int64_t n_cases, double n_lo, double n_hi, double slack, uint64_t *counts);

/* The keyed streams over their whole key space, and the scalar functions behind them pointwise (device >= 0: in kernels on that device;
 * device == -1: the host instantiation of the same inline code).  Three independent parts; a part with count 0 is skipped, its pointers
 * may be NULL.
 *   streams, element i keyed (seed[i], chain[i], tag[i], id[i], iter[i]) -- the chain as the kernels pass it, all 32 bits:
 *     out_uniforms[4 i ..]  the first two pairs of uniforms of the Philox4x32 stream (K2's Gamma stream, the simulated traces)
 *     out_words[3 i ..]     the first three words of the Philox2x32 row stream
 *     out_gamma[i]          the Gamma(shape[i]) draw of the Philox4x32 stream times scale (NaN unless shape[i] > 0)
 *   math, element i at x[i]:
 *     out_probit, out_lgamma   the inverse normal CDF of the proportion summaries (AS 241), log Gamma of mmdiff's densities
 *     out_normal[i]            the N(0,1) draw of stream (normal_seed, chain 0, the Gamma tag, id i, iteration 0): x is not used
 *     out_stirling[i]          the binomial sampler's Stirling remainder of log(x!), 0 <= x < 2^32 (NaN elsewhere)
 *     out_ilogb[i]             the exponent of x, 0 < x < inf, subnormals included (INT32_MIN elsewhere)
 *   words, element i:
 *     out_u32[i], out_u52[i]   the uniforms made of the word w0[i] and of the pair (w0[i], w1[i])
 *     out_target[i]            the categorical draw's target of word w0[i] over weights of total t[i]
 * Additive in version 8. */
typedef struct mmg_keyed_io {
    int64_t n_streams;
    const uint64_t *seed, *id;
    const uint32_t *chain, *tag, *iter;
    const double *shape;
    double scale;
    double *out_uniforms;
    uint32_t *out_words;
    double *out_gamma;
    int64_t n_math;
    const double *x;
    uint64_t normal_seed;
    double *out_probit, *out_lgamma, *out_normal, *out_stirling;
    int32_t *out_ilogb;
    int64_t n_words;
    const uint32_t *w0, *w1;
    const double *t;
    double *out_u32, *out_u52, *out_target;
} mmg_keyed_io;
int mmg_selftest_keyed(int device, const mmg_keyed_io *io);

/* The three shortcuts of the conditional-binomial chain's kernel (k_sample_bigk) on caller-given points (device >= 0: in kernels on that
 * device; device == -1: the host instantiation of the same inline code, which has no fp32 tests).  Two independent parts; a part with
 * count 0 is skipped, its pointers may be NULL.  Out-of-domain input is MMG_ERR_ARG.
 *   inversion, element i: inv_n[i] >= 1, 0 < inv_p[i] <= 1/2 with n p < 10, 0 < inv_u[i] < 1; inv_slack > 0 scales the fp32 search's bound
 *     out_inv_bound[i]  binv_zero_bound(n, n p): a uniform at or below it is x = 0 without the search (the kernel's STEP)
 *     out_inv_x[i]      the x of the fp64 search on the uniform u, -1 where the sum of its terms fell short of u.  The search walks as
 *                       far as u sends it: a caller keeps u away from 1 at large n
 *     out_inv_pre[i]    the x of the fp32 search where its bound decides, -1 where it does not (always -1 on the host)
 *   BTRS, element i: btrs_n[i] >= 21, btrs_p[i] <= 1/2 with n p >= 10, the attempt's two uniforms 0 < btrs_u[i], btrs_v[i] < 1; constants
 *   and candidate formed as the kernel forms them
 *     out_btrs_kf[i]     the candidate
 *     out_btrs_reach[i]  0: the candidate is outside [0, n]; 1: the squeeze accepts it; 2: the exact test is reached, and then
 *     out_btrs_exact[i]  1 / 0: the fp64 test accepts / rejects (-1 unless reach is 2);  out_btrs_diff[i]: its ub - v (0 unless reach is 2)
 *     out_btrs_d32[i], out_btrs_e32[i]  the fp32 estimate of the difference and the bound on its error (0, 0 on the host or unless reach is 2)
 *     out_btrs_pre[i]    +1 / -1: the fp32 test accepts / rejects, 0: undecided (0 on the host or unless reach is 2)
 * Additive in version 8. */
typedef struct mmg_bigk_points {
    int64_t n_inv;
    const uint32_t *inv_n;
    const double *inv_p, *inv_u;
    double inv_slack;
    double *out_inv_bound;
    int64_t *out_inv_x;
    int32_t *out_inv_pre;
    int64_t n_btrs;
    const uint32_t *btrs_n;
    const double *btrs_p, *btrs_u, *btrs_v;
    double *out_btrs_kf;
    int32_t *out_btrs_reach, *out_btrs_exact;
    double *out_btrs_diff;
    float *out_btrs_d32, *out_btrs_e32;
    int32_t *out_btrs_pre;
} mmg_bigk_points;
int mmg_selftest_bigk_points(int device, const mmg_bigk_points *io);

/* ---- mmcollapse: candidates collapsed by their mean posterior anti-correlation across samples ----------------------------
 * src/mmcollapse.cpp:483-561 (covariances of the candidates' traces per sample, mean correlations), :713-747 (row maxima for the
 * threshold), :758-819 with collapse() at :398-441 (the greedy loop).  The device holds the centred traces of every sample and the
 * C x C matrix V of mean correlations, not the reference's C x C x S cube of covariances.  Every sum runs in a fixed order and
 * without floating-point atomics: reruns are bit-identical.  Additive in ABI version 8. */
typedef struct mmg_collapse mmg_collapse;
/* observed: [n_cand][n_samples], non-zero where candidate c was observed in sample s (the mask S of :688-698).
 * trace_len: a positive multiple of 16 (the reference: 1024). */
int mmg_collapse_create(int device, uint32_t n_samples, uint32_t n_cand, uint32_t trace_len, const uint8_t *observed, mmg_collapse **out);
/* the raw (not logged) traces of sample s, trace[k * n_cand + c] (the layout of the trace files); centred on the device */
int mmg_collapse_set_sample(mmg_collapse *h, uint32_t sample, const double *trace);
/* V once every sample is set: V(i, j) = sum over samples observed in both of cov / sqrt(var) / sqrt(var), over their count */
int mmg_collapse_correlate(mmg_collapse *h);
/* rows [first, first + count) of V as it stands, out[r * n_cand + j] */
int mmg_collapse_get_rows(mmg_collapse *h, uint32_t first, uint32_t count, double *out);
/* per row of the initial V, the maximum over the off-diagonal entries starting from -1, NaN skipped (:719-730) */
int mmg_collapse_row_max(mmg_collapse *h, double *out);
/* The greedy loop: while min V < thr (Armadillo's min: NaN skipped, ties to the first entry in column-major order), merge the pair
 * (a < b) at the minimum into a -- the summed trace, a's observed mask --, b leaves.  pairs[2 m], pairs[2 m + 1] = a, b and values[m]
 * = the minimum of merge m.  At most max_merges merges per call; a later call continues.  *stopped = 1 once the minimum reached thr. */
int mmg_collapse_run(mmg_collapse *h, double thr, uint32_t max_merges, uint32_t *pairs, double *values, uint32_t *n_merges, int32_t *stopped);
/* device memory the handle holds (it allocates everything at creation) */
int mmg_collapse_device_bytes(mmg_collapse *h, uint64_t *bytes);
void mmg_collapse_destroy(mmg_collapse *h);
/* The output stage (:827-1107) on host traces: trace[k * n_cols + c] (trace_len rows), virtual traces v = Gamma(alpha) * virtual_scale[v]
 * keyed (seed, stream, a tag of their own, virtual_id[v], row), and n_series output series, series g the sum of its members
 * (series_member[series_ptr[g] .. series_ptr[g + 1]), in that order; member < n_cols a trace column, n_cols + v virtual trace v).  Per
 * series: mean of the logged trace, Sokal's var and tau of the logged trace and the return code (as mmg_summary_get). */
int mmg_collapse_summarize(int device, uint32_t trace_len, uint32_t n_cols, const double *trace, uint32_t n_virtual, const uint64_t *virtual_id,
                           const double *virtual_scale, double alpha, uint64_t seed, uint32_t stream, uint32_t n_series, const uint64_t *series_ptr,
                           const uint32_t *series_member, double *log_mean, double *var, double *tau, int32_t *sokal_rc);


/* ---- posterior assignment probability of every hit ----------------------------------------------------------------------
 * What the sample kernel draws and discards (src/mmseq.cpp:857-891), Rao-Blackwellised: for a hit (i, t) the mean over the samples s
 * of a range of mu_s[t] / sum_{t' in row i} mu_s[t'] (1 / hits of the row where that sum is 0 or not finite, the oracle's degenerate
 * case; exactly 1 for the hit of a row of one).  Every sum runs in a fixed order (tests/assign_ref.py) without floating-point atomics: reruns are
 * bit-identical.  The handle has its own copy of the rows, in the CALLER's order and numbering -- hit j of the results is entry j of
 * col_idx; no mmg_problem is needed.  Additive in ABI version 8. */
typedef struct mmg_assign mmg_assign;
/* row_ptr: n_rows + 1 offsets from 0, not decreasing (empty rows are allowed and produce nothing); col_idx: row_ptr[n_rows] columns
 * below n_tx.  Checked before any device work. */
int mmg_assign_create(int device, uint64_t n_rows, uint32_t n_tx, const uint64_t *row_ptr, const uint32_t *col_idx, mmg_assign **out);
/* The samples [first_sample, first_sample + n_samples) of chain `chain` of a sampler with keep_trace on the same device whose problem
 * has n_tx transcripts.  The call waits for the chain; the sampler's trace (sample-major, device numbering) is transposed on the
 * device into the handle's copy and never touches the host.  MMG_ERR_STATE for samples the chain has not kept yet. */
int mmg_assign_run_sampler(mmg_assign *h, mmg_sampler *s, int chain, int first_sample, int n_samples);
/* The same over a host trace laid out as mmg_sampler_get_trace returns it: trace[t * trace_len + s]. */
int mmg_assign_run_host(mmg_assign *h, const double *trace, int trace_len, int first_sample, int n_samples);
/* P of the hits [first_hit, first_hit + n_hits) of the last run; MMG_ERR_STATE before the first one */
int mmg_assign_get(mmg_assign *h, uint64_t first_hit, uint64_t n_hits, double *P);
/* 8 (n_rows + 1) + 12 max(hits, 1) bytes from creation; after a run over n_samples of a trace of T samples also 8 n_tx T (the
 * trace copy) + 8 W ceil64(n_samples) (the scratch slices), W = max(1, min(ceil(hits / 256), 64 MiB / (8 ceil64(n_samples)),
 * MMG_OPT_ASSIGN_WAVES if set)), ceil64 rounding up to a multiple of 64.  Both are kept until a run of another shape. */
int mmg_assign_device_bytes(mmg_assign *h, uint64_t *bytes);
void mmg_assign_destroy(mmg_assign *h);

/* ---- contrasts: posterior log-ratios between sets of transcripts of one sample ------------------------------------------
 * The kept samples of a chain are draws from the joint posterior, so they carry the posterior of any comparison between features of
 * the same sample: an allele against the other, an isoform against its gene, a gene against its family.  Contrast c has an ordered
 * numerator list num_member[num_ptr[c] .. num_ptr[c + 1]) and a denominator list alike; a member < n is the caller's transcript,
 * n + v isoform without hits v (the members of mmg_summary_desc's groups).  Both lists are non-empty; a member may be on both sides
 * (a proportion), not twice on one.  Per kept sample s: N_s, D_s = the members' traces added in list order from 0, r_s = log N_s -
 * log D_s (the library's log; never the logarithm of the quotient, which underflows where the difference does not; non-finite values
 * propagate), gt_s = N_s > D_s.  Per contrast: log_ratio = the mean of r (samples added in order); var, tau and the return code of
 * Sokal's estimator on r, as mmg_summary_get gives them for log mu; the order statistics of r at percentile_index; p_gt = the share
 * of samples with gt_s.  Every sum runs in a fixed order (tests/contrast_ref.py) without floating-point
 * atomics: reruns are bit-identical.  Additive in ABI version 8. */
typedef struct mmg_contrast mmg_contrast;
typedef struct mmg_contrast_desc {
    uint32_t n_contrasts;                                  /* at least 1 */
    const uint64_t *num_ptr; const uint32_t *num_member;   /* n_contrasts + 1 offsets from 0, not decreasing */
    const uint64_t *den_ptr; const uint32_t *den_member;
    uint32_t n_percentiles; const int32_t *percentile_index;   /* sample indices of the sorted series; outside [0, S): NaN */
} mmg_contrast_desc;
/* After mmg_summary_finish (or _create) of a summary q of sampler s: the chain is the summary's, and so are the isoforms without hits
 * (their simulated traces are drawn again, the same bits).  Checked before any device work.  The sampler must outlive the handle. */
int mmg_contrast_create(mmg_sampler *s, mmg_summary *q, const mmg_contrast_desc *d, mmg_contrast **out);
/* The same from host traces, series-major traces[member * S + s]; members < n_series only. */
int mmg_contrast_of_traces(int device, uint32_t S, uint32_t n_series, const double *traces, const mmg_contrast_desc *d, mmg_contrast **out);
/* log_ratio, var, tau, sokal_rc, p_gt: [n_contrasts]; percentiles: [n_contrasts][n_percentiles]; any output may be NULL.  The results
 * are on the host from creation: no device work. */
int mmg_contrast_get(mmg_contrast *h, double *log_ratio, double *var, double *tau, int32_t *sokal_rc, double *p_gt, double *percentiles);
/* r of the contrasts [first, first + count), R[(c - first) * S + s]: computed again on the device, the same bits as at creation */
int mmg_contrast_get_rows(mmg_contrast *h, uint32_t first, uint32_t count, double *R);
/* What the handle holds between calls: 16 (n_contrasts + 1) + 4 (numerator members + denominator members) bytes of lists; from a
 * sampler also 4 bytes per distinct member of each slab (summed over the slabs) and 16 bytes per isoform without hits of the summary;
 * from host traces also 8 n_series S.  A slab is cap = max(1, min(n_contrasts, 256 MiB / (8 S), MMG_OPT_CONTRAST_SLAB if set))
 * contrasts.  While creation or mmg_contrast_get_rows runs, on top of that: 8 S cap of series (get_rows: 8 S min(cap, count)),
 * from a sampler 8 S times the largest number of distinct members of a slab, and at creation 16 max(S, 1) + 4 n_percentiles +
 * cap (32 + 8 n_percentiles) bytes of tables and results, plus 24 SP min(cap, 1024) of workspace when S > 8192 (SP = S rounded up to
 * a power of two). */
int mmg_contrast_device_bytes(mmg_contrast *h, uint64_t *bytes);
void mmg_contrast_destroy(mmg_contrast *h);

/* ---- the posterior correlation of transcripts that share reads -----------------------------------------------------------
 * Which transcripts of a sample are confounded with which: for ordered pairs (a, b) of transcripts, a != b, from the S kept samples
 * of one chain.  Per sample u = log x_a, v = log x_b, w = log(x_a + x_b) (the library's log).  Every sum over the samples runs in
 * the order of a wave with one lane per sample (lane l adds its samples l, l + 64, ... ascending from 0.0, the 64 partial sums are
 * folded by halving).  mean_a, mean_b, mean_sum = the sums of u, v, w over S; then with du = u - mean_a, dv = v - mean_b,
 * dw = w - mean_sum: saa, sbb, sab, sss = the sums of du du, dv dv, du dv, dw dw (each product rounded, then added); n_gt = the
 * number of samples with x_a > x_b.  Non-finite values propagate.  mean_a and saa depend on a alone: the same bits in every pair a is
 * in, whatever the slab.  The caller derives cor = sab / (sqrt(saa) sqrt(sbb)), sd_a = sqrt(saa / (S - 1)), p_gt = n_gt / S.
 * The same pair may occur twice, and a member may be in any number of pairs; the output order is the caller's pair order.
 * tests/pairs_ref.py; no floating-point atomics: reruns are bit-identical.  Additive in ABI version 8. */
typedef struct mmg_pairs mmg_pairs;
/* Over the trace_len kept samples of `chain` of sampler s, a and b in the caller's numbering.  The sampler must hold a trace and be
 * past its last kept sample (MMG_ERR_STATE otherwise).  MMG_ERR_ARG, with a message that names the pair: n_pairs == 0, a NULL array or
 * output, a == b, a member >= n, a chain out of range.  Checked before any device work. */
int mmg_pairs_create(mmg_sampler *s, int chain, uint64_t n_pairs, const uint32_t *a, const uint32_t *b, mmg_pairs **out);
/* The same from host traces, series-major traces[member * S + s]. */
int mmg_pairs_of_traces(int device, uint32_t S, uint32_t n_series, const double *traces, uint64_t n_pairs, const uint32_t *a, const uint32_t *b,
                        mmg_pairs **out);
/* Every output [n_pairs]; any pointer may be NULL.  The results are on the host from creation: no device work. */
int mmg_pairs_get(mmg_pairs *h, double *mean_a, double *mean_b, double *mean_sum, double *saa, double *sbb, double *sab, double *sss, uint32_t *n_gt);
/* The handle holds nothing on the device once it exists; this is what its creation held at its peak.  The pairs are cut into slabs
 * of consecutive pairs: a slab ends in front of the pair that would bring its distinct members over max(2, 256 MiB / (16 S)) or its
 * pairs over min(2^22, MMG_OPT_PAIRS_SLAB if set).  With Mx the largest number of distinct members of a slab and Px the largest
 * number of pairs of one: 4 Mx of member list + 8 S Mx of centred logarithms + 16 Mx of member means and squares + 8 Px of slots +
 * 60 Px of results; from a sampler also 8 S Mx of gathered traces, from host traces also 8 n_series S. */
int mmg_pairs_device_bytes(mmg_pairs *h, uint64_t *bytes);
void mmg_pairs_destroy(mmg_pairs *h);

/* ---- the posterior fold change of a feature between two samples, from all pairs of their draws ---------------------------
 * Two samples are independent given their reads, so every pair (draw i of A, draw j of B) is a draw from the joint posterior of the
 * log fold change: Sa Sb draws per feature.  This is the posterior given the reads of these two libraries; it says nothing about
 * biological variability -- for groups with replicates the tool is mmdiff.
 * Feature f has the draws a[0 .. Sa) and b[0 .. Sb) on the mu scale and the offset `off` on the natural-log scale.  It is valid when
 * every draw of both sides is finite and > 0; otherwise its status byte gets bit 0 (a draw of A) and / or bit 1 (a draw of B), all
 * its outputs are NaN and its counts 0 (checked before anything else is done with the series).  For a valid feature, status 0 and:
 *   x_i = log a_i (the library's log), y_j = log b_j + off, d_ij = x_i - y_j, each rounded once; -0.0 counts as +0.0.
 *   n_gt = #{(i, j): x_i > y_j}, n_eq = #{(i, j): x_i == y_j}, exact, from x and y (never through d); the caller forms
 *       p_gt = (n_gt + n_eq / 2) / (Sa Sb).
 *   quantiles[f * n_ranks + r] = the ranks[r]-th smallest (zero-based) of the Sa Sb values d_ij, exactly: numpy's
 *       np.sort(np.subtract.outer(x, y), axis=None)[k].  A rank >= Sa Sb gives NaN for that rank alone.
 *   mean_a = sum x_i / Sa, mean_b = sum y_j / Sb (offset included), ss_a = sum (x_i - mean_a)^2, ss_b likewise (each square rounded,
 *       then added).  Every sum runs over the series in the caller's sample order, as a wave with one lane per sample adds: lane l
 *       adds its samples l, l + 64, ... ascending from 0.0, the 64 partial sums are folded by halving.  The caller derives
 *       lfc = mean_a - mean_b and sd = sqrt(ss_a / (Sa - 1) + ss_b / (Sb - 1)).
 * 1 <= Sa, Sb <= 4096 (they need not be equal, nor powers of two), n_features >= 1, n_ranks <= 64, off finite: MMG_ERR_ARG otherwise,
 * with a message that names the argument; every argument is checked before any device work.  tests/fold_ref.py, DESIGN.md
 * section 16; no floating-point atomics: reruns are bit-identical.  Additive in ABI version 8. */
typedef struct mmg_fold mmg_fold;
/* From host traces, series-major: a[f * Sa + s], b[f * Sb + s]. */
int mmg_fold_of_traces(int device, uint32_t n_features, uint32_t Sa, const double *a, uint32_t Sb, const double *b, double off, uint32_t n_ranks,
                       const uint32_t *ranks, mmg_fold **out);
/* From the resident traces of two samplers on one device: feature f compares transcript ia[f] of chain chain_a of sampler sa with
 * transcript ib[f] of chain chain_b of sampler sb (the caller's numbering; sa and sb may be the same sampler), over their trace_len
 * kept samples (Sa, Sb).  Both samplers must hold a trace and be past their last kept sample (MMG_ERR_STATE otherwise).  MMG_ERR_ARG:
 * a NULL sampler, array or output, a chain out of range, a member >= n (the message names the feature), samplers on different
 * devices, and the rules above.  The same bits as mmg_fold_of_traces on the downloaded traces. */
int mmg_fold_create(mmg_sampler *sa, int chain_a, mmg_sampler *sb, int chain_b, uint32_t n_features, const uint32_t *ia, const uint32_t *ib, double off,
                    uint32_t n_ranks, const uint32_t *ranks, mmg_fold **out);
/* mean_a, mean_b, ss_a, ss_b, n_gt, n_eq, status: [n_features]; quantiles: [n_features][n_ranks]; any pointer may be NULL.  The
 * results are on the host from creation: no device work. */
int mmg_fold_get(mmg_fold *h, double *mean_a, double *mean_b, double *ss_a, double *ss_b, uint32_t *n_gt, uint32_t *n_eq, double *quantiles,
                 uint8_t *status);
/* The handle holds nothing on the device once it exists; this is what its creation held at its peak.  The features are cut into
 * slabs of cap = max(1, min(n_features, 256 MiB / (8 (Sa + Sb)), MMG_OPT_FOLD_SLAB if set)) consecutive features:
 * 8 cap (Sa + Sb) of series + cap (41 + 8 n_ranks) of results + 4 n_ranks of ranks; from samplers also 8 cap of member lists. */
int mmg_fold_device_bytes(mmg_fold *h, uint64_t *bytes);
void mmg_fold_destroy(mmg_fold *h);

/* ---- posterior distances and correlations between samples, from their joint draws ----------------------------------------
 * Samples are independent given their reads, so draw t of every one of S samples together is one draw from the joint posterior of all
 * S expression profiles, and a distance matrix computed per draw gives T posterior draws of that matrix.
 * Sizes: 2 <= S <= 256 samples, 1 <= F < 2^31 features, 1 <= T <= 4096 joint draws; at most 64 zero-based ranks, a rank >= T gives
 * NaN for that rank alone.
 * Values: x = log v (the library's log), or x = v with MMG_SIM_LOGGED; z_s[t][f] = (x + off_s) - c[f], each operation rounded once,
 * -0.0 stored as +0.0; c the handle's centre (NULL: zeros), off_s the sample's offset on the natural-log scale.
 * Used features: mask[f] != 0 (NULL: all ones) and every one of the feature's S T values valid -- finite and > 0, or just finite with
 * MMG_SIM_LOGGED; the check comes before the logarithm.  n is their number; the others contribute nothing anywhere (their z is 0.0
 * once mmg_sim_run has run).  With n < 2 the status byte has bit 0, every summary is NaN and the counts are 0.
 * Stage 1, per draw t: G[t][r][s] = sum over the used f of z_r[t][f] z_s[t][f] and m[t][r] = sum of z_r[t][f], in fp64 on the matrix
 * cores.  The order of the sum is the kernel's own -- fixed for given inputs and settings, no floating-point atomics, so reruns give
 * the same bits -- and not part of the specification.  G is symmetric.
 * Stage 2, per draw and pair r < s, exactly these operations in this order, each rounded once, from the stage-1 numbers as stored:
 *   D[t] = sqrt(max(0, (G_rr + G_ss) - 2 G_rs) / n): the root-mean-square log ratio over the used features (the centre cancels);
 *   R[t] = (G_rs - m_r m_s / n) / sqrt((G_rr - m_r m_r / n) (G_ss - m_s m_s / n)): Pearson's correlation across the features.  A
 *       variance term <= 0 or an R that is not finite in any draw gives the pair status bit 1 and NaN in every R output of the pair;
 *   nn[a][b] = #{t: b = argmin over b' != a of (G_aa + G_b'b') - 2 G_ab'}, ties to the smallest b': integers, every row sums to T.
 * Per pair (r < s, r-major) over the T draws: mean_D = sum D / T, ss_D = sum (D - mean_D)^2 and the same of R, every sum in the
 * draws' order as a wave with one lane per draw adds (as mmg_fold_*); q_D, q_R [pair][n_ranks]: the order statistics at the ranks.
 * The caller derives sd = sqrt(ss / (T - 1)) and p_nearest = nn / T.  tests/sim_ref.py, DESIGN.md section 17.  Additive in ABI
 * version 8. */
#define MMG_SIM_LOGGED 1u /* the traces are on the log scale already */
typedef struct mmg_sim mmg_sim;
/* Allocates everything the handle ever holds: S T F 8 bytes of draws plus the results (mmg_sim_device_bytes).  MMG_ERR_ARG, with a
 * message that names the argument, before the device is touched: S, F or T outside the sizes above, flags with unknown bits, a
 * centre that is not finite; and, with both numbers in the message, a need above the device's free memory. */
int mmg_sim_create(int device, uint32_t S, uint32_t F, uint32_t T, const double *centre, const uint8_t *mask, uint32_t flags, mmg_sim **out);
/* trace[t * F + f], the layout of the trace files (as mmg_collapse_set_sample takes it); off finite.  A sample may be set again before
 * mmg_sim_run (MMG_ERR_STATE after it). */
int mmg_sim_set_sample(mmg_sim *h, uint32_t s, const double *trace, double off);
/* Both stages.  MMG_ERR_STATE while a sample is unset; MMG_ERR_ARG for n_ranks > 64 or NULL ranks with n_ranks > 0.  A later call
 * summarises again (other ranks); the stage-1 numbers come out the same.  The calls out of sequence are MMG_ERR_STATE, as everywhere
 * in this library, not MMG_ERR_ARG: no argument is wrong.  The getters of results (used, gram, get) serve the last run that
 * succeeded: after a run that failed they are MMG_ERR_STATE again, as before the first. */
int mmg_sim_run(mmg_sim *h, uint32_t n_ranks, const uint32_t *ranks);
/* used[F] (0 / 1) and n of the last run; either may be NULL */
int mmg_sim_get_used(mmg_sim *h, uint8_t *used, uint64_t *n);
/* z of sample s, draws [first_draw, first_draw + n_draws): out[n_draws][F] as it stands on the device */
int mmg_sim_get_z(mmg_sim *h, uint32_t s, uint32_t first_draw, uint32_t n_draws, double *out);
/* G[n_draws][S][S] and m[n_draws][S] of the draws [first_draw, first_draw + n_draws); either may be NULL */
int mmg_sim_get_gram(mmg_sim *h, uint32_t first_draw, uint32_t n_draws, double *G, double *m);
/* mean_D, ss_D, mean_R, ss_R, pair_status: [S (S - 1) / 2]; q_D, q_R: [S (S - 1) / 2][n_ranks]; nn: [S][S], diagonal 0; status: one
 * byte; any pointer may be NULL.  The results are on the host since the run: no device work. */
int mmg_sim_get(mmg_sim *h, double *mean_D, double *ss_D, double *q_D, double *mean_R, double *ss_R, double *q_R, uint32_t *nn,
                uint8_t *pair_status, uint8_t *status);
/* What the handle holds from creation to destruction.  With NT = ceil((S + 1) / 16), U = NT (NT + 1) / 2 tiles,
 * CH = min(F, max(MMG_OPT_SIM_CHUNK if set, else 4096, ceil(F / 65535)))
 * features per chunk, C = ceil(F / CH) chunks and P = S (S - 1) / 2 pairs: 8 S T F of draws + F (S + 18) of centre, ones, mask, used
 * and marks + 2048 T C U of partial tiles + 8 T (S S + S + 1) of G, m, n + 8 + 1057 P of summaries (64 ranks) + 4 S S + 256. */
int mmg_sim_device_bytes(mmg_sim *h, uint64_t *bytes);
void mmg_sim_destroy(mmg_sim *h);

/* ---- isoform usage within groups of transcripts of one sample: dominant-isoform probabilities and usage entropy ----------
 * Isoforms of a gene share their reads, so their draws are strongly anti-correlated, and which one is the major isoform, or whether
 * the gene is spread over several, cannot be read off the marginal summaries: it needs the joint draws of the group's members.
 * Group g is the ordered list member[ptr[g] .. ptr[g + 1]) of K >= 1 distinct members, laid out as mmg_summary_desc's genes are; a
 * member < n is the caller's transcript, n + v isoform without hits v (its simulated trace).  A member may be in several groups, not
 * twice in one.  Up to 8 thresholds theta_q, each finite in [0, 1); up to 64 zero-based ranks, a rank >= S gives NaN for that rank
 * alone; 1 <= S <= 4096 kept samples of one chain; n_groups >= 1.
 * Per sample s, with x_j = the trace of the member at position j, every operation one IEEE double operation rounded once, in this
 * order:
 *   valid: every x_j is finite and >= 0, and T_s is finite and > 0.  If any sample of a group is not valid the group's status byte
 *       gets bit 0, every floating-point output of the group is NaN (rows included; its top / second rows are 0xffffffff) and every
 *       count of the group and of its members is 0 (major is then position 0).  The check comes before the logarithms and the sort;
 *       other groups are unaffected.
 *   T_s = ((0.0 + x_0) + x_1) + ... in list order: the order of the summary's gene sums, so the bits of the gene's trace row.
 *   top_s = the smallest j with x_j = the maximum (the draws are compared, never the proportions); second_s = the smallest j != top_s
 *       with x_j = the maximum over j != top_s, 0xffffffff when K = 1.
 *   p_j = x_j / T_s (the summary's proportion), P_s = x_top / T_s.
 *   H_s: a = 0.0; for j ascending: if (p_j > 0) a = a + p_j * log(p_j) (the library's log); H_s = -a, -0.0 stored as +0.0.
 *   above_s[j][q] = x_j > theta_q * T_s.
 * Per member of a group, exact integers: n_top[j] = #{s: top_s = j}, n_second[j] alike, n_above[j][q].
 * Per group: major = the smallest j with the largest n_top (a position in the list); n_distinct = #{j: n_top[j] > 0};
 * mean_H = sum H / S, ss_H = sum (H - mean_H)^2, mean_P, ss_P alike, every sum in the samples' order as a wave with one lane per
 * sample adds (lane l adds its samples l, l + 64, ... ascending from 0.0, the 64 partial sums are folded by halving, as mmg_pairs_*);
 * q_H, q_P [group][n_ranks]: the order statistics of H and of P at the ranks.  The caller derives p_top = n_top / S,
 * sd = sqrt(ss / (S - 1)) and the effective number of isoforms exp(mean_H).  For the same group in two samples A and B, which are
 * independent given their reads, P(their major isoforms differ) = 1 - sum_j nA_top[j] nB_top[j] / (S_A S_B) over all pairs of draws:
 * host arithmetic on the counts.  No floating-point atomics; counts are population counts of ballots: reruns and any slab cut give the
 * same bits.  tests/isoforms_ref.py, DESIGN.md section 18.  Additive in ABI version 8. */
typedef struct mmg_isoform mmg_isoform;
typedef struct mmg_isoform_desc {
    uint32_t n_groups;                                /* at least 1 */
    const uint64_t *ptr; const uint32_t *member;      /* n_groups + 1 offsets from 0, increasing */
    uint32_t n_thresholds; const double *threshold;   /* at most 8, each finite in [0, 1) */
    uint32_t n_ranks; const uint32_t *rank;           /* at most 64, zero-based */
} mmg_isoform_desc;
/* After mmg_summary_finish (or _create) of a summary q of sampler s (MMG_ERR_STATE before): the chain is the summary's, and so are the
 * isoforms without hits (their simulated traces are drawn again, the same bits).  MMG_ERR_ARG, with a message that names the
 * argument, the group and the member, before the device is touched: a NULL pointer, n_groups == 0, an empty group, a member twice in
 * a group, a member out of range, a threshold outside [0, 1) or not finite, more than 8 thresholds, more than 64 ranks, S outside
 * [1, 4096].  The sampler must outlive the handle. */
int mmg_isoform_create(mmg_sampler *s, mmg_summary *q, const mmg_isoform_desc *d, mmg_isoform **out);
/* The same from host traces, series-major traces[member * S + s]; members < n_series only. */
int mmg_isoform_of_traces(int device, uint32_t S, uint32_t n_series, const double *traces, const mmg_isoform_desc *d, mmg_isoform **out);
/* n_top, n_second: one entry per entry of member[], in its flat order; n_above: [entry][n_thresholds].  Any output may be NULL; served
 * from the host. */
int mmg_isoform_get_members(mmg_isoform *h, uint32_t *n_top, uint32_t *n_second, uint32_t *n_above);
/* status, major, n_distinct, mean_H, ss_H, mean_P, ss_P: [n_groups]; q_H, q_P: [n_groups][n_ranks].  Any output may be NULL; served
 * from the host: no device work. */
int mmg_isoform_get_groups(mmg_isoform *h, uint8_t *status, uint32_t *major, uint32_t *n_distinct, double *mean_H, double *ss_H, double *mean_P,
                           double *ss_P, double *q_H, double *q_P);
/* top, second, H, P of the groups [first, first + count), [(g - first) * S + s]: computed again on the device, the same bits as at
 * creation.  Any output may be NULL. */
int mmg_isoform_get_rows(mmg_isoform *h, uint32_t first, uint32_t count, uint32_t *top, uint32_t *second, double *H, double *P);
/* What the handle holds between calls: 8 (n_groups + 1) + 4 (entries of member[]) bytes of lists; from a sampler also 4 bytes per
 * distinct member of each slab (summed over the slabs) and 16 bytes per isoform without hits of the summary; from host traces also
 * 8 n_series S.  The groups are cut into slabs of consecutive groups: a slab ends in front of the group that would bring its groups
 * over gcap = max(1, min(n_groups, 256 MiB / (16 S), MMG_OPT_ISO_SLAB if set)) or, from a sampler, its distinct members over
 * max(1, 256 MiB / (8 S)); a slab holds at least one group.  While creation or mmg_isoform_get_rows runs, with Gx the most groups and
 * Mx the most distinct members of a slab, on top of that: 16 S Gx of H and P rows (get_rows: min(Gx, count) for Gx, and 4 S of that
 * for each of top and second that is asked for), from a sampler 8 S Mx of gathered series, and at creation
 * 4 (2 + n_thresholds) (entries of member[]) of counters + Gx (41 + 16 n_ranks) of results + 4 n_ranks. */
int mmg_isoform_device_bytes(mmg_isoform *h, uint64_t *bytes);
void mmg_isoform_destroy(mmg_isoform *h);

/* ---- mmdiff: Bayesian model selection between two linear models per feature -------------------------------------------
 * src/bms.cpp driven as src/mmdiff.cpp:744-866: per feature an independent MCMC over both models with pseudopriors, the model
 * indicator gamma and a tuned prior log odds.  One lane per feature, state in device memory; the host drives the phases:
 * create, burnin once, tune_batch until the untuned count is 0 or the caller's batch limit (none for -notune), sample, get_results.
 * Keyed streams (seed, 0, TAG_DIFF, feature, iteration): reruns are bit-identical.  Additive in ABI version 8. */
typedef struct mmg_diff mmg_diff;
/* y, e: [F][N] estimates and their standard deviations; M: [N][K] covariates; P0: [N][L0], P1: [N][L1] the models' predictors;
 * C: [N][2] the variance class of sample i under model m, labelled 0 .. n_m - 1.  A single column that varies by less than 1e-5 is
 * "nil" (no covariate), as in the reference.  Caps: N <= 512, K <= 8, L0, L1 <= 16, 16 classes per model. */
int mmg_diff_create(int device, uint32_t n_features, uint32_t n_samples, const double *y, const double *e, uint32_t K, const double *M,
                    uint32_t L0, const double *P0, uint32_t L1, const double *P1, const int32_t *C, double d, double s, double pdash,
                    int fixalpha, uint64_t seed, mmg_diff **out);
/* the burn-in (at least 104 iterations, recorded from iteration 102; the CLI takes multiples of 1024, as the reference does), then
 * the pseudopriors from its record */
int mmg_diff_burnin(mmg_diff *h, uint32_t iters);
/* one tuning batch of 128 iterations; *untuned = the features still untuned after the batch's tuning step */
int mmg_diff_tune_batch(mmg_diff *h, uint32_t *untuned);
/* iters sampling iterations (may be called again to continue) */
int mmg_diff_sample(mmg_diff *h, uint32_t iters);
/* gamma_mean[F], logitp[F], alpha[2][F], beta[2][K][F], eta[L0 + L1][F] (model 0's columns first): posterior means over the
 * sampling iterations, each as sum / count; any pointer may be NULL */
int mmg_diff_get_results(mmg_diff *h, double *gamma_mean, double *logitp, double *alpha, double *beta, double *eta);
/* flags[3] = (M nil, P0 nil, P1 nil), n_classes[2], the tuning batches run so far; any pointer may be NULL */
int mmg_diff_info(mmg_diff *h, int32_t *flags, uint32_t *n_classes, uint32_t *batches);
int mmg_diff_device_bytes(mmg_diff *h, uint64_t *bytes);
void mmg_diff_destroy(mmg_diff *h);

/* ---- mmdiff: traces (what the reference writes under -tracedir).  Additive in ABI version 8. ----
 * The traced parameters, in the order of BMS::initialise_streams and named as its files are: alpha0, alpha1; beta0_i, beta1_i per
 * column of M; eta0_l, eta1_l; lambda0_l, lambda1_l per column of P0 / P1; sigmasq0_c, sigmasq1_c per class; rho0, rho1; gamma (as
 * 0.0 / 1.0).  A nil M or P keeps its columns, at their starting values.  *n_params counts gamma, the last one; *n_pseudo is the
 * number of columns of mmg_diff_get_pseudo.  Either pointer may be NULL. */
int mmg_diff_trace_layout(mmg_diff *h, uint32_t *n_params, uint32_t *n_pseudo);
/* the name of traced parameter `param` into name[len] */
int mmg_diff_trace_name(mmg_diff *h, uint32_t param, char *name, uint32_t len);
/* The sink of recorded rows: phase 0 is the burn-in, 1 sampling; rows [first_row, first_row + n_rows) of that phase, row r the state
 * after the iteration r * every of the phase (sampling iterations count from the first one), as rows[(r - first_row) * P + s][F]
 * with P = n_params in sampling and n_params - 1 (no gamma) in burn-in.  `rows` is valid during the call.  A non-zero return stops
 * the run: the entry that was running returns MMG_ERR_IO, and every later burnin / tune_batch / sample MMG_ERR_STATE. */
typedef int (*mmg_diff_trace_sink)(void *user, int phase, uint32_t first_row, uint32_t n_rows, const double *rows);
/* Before mmg_diff_burnin: record every every_burnin-th burn-in and every every_sample-th sampling iteration (both >= 1) and hand
 * the rows to `sink` on the calling thread while the next launch runs.  Recording draws nothing: the chain is the one of an untraced
 * handle, bit for bit.  The handle then holds two row buffers on the device (counted by mmg_diff_device_bytes: together
 * 2 * R * n_params * F * 8 bytes, R = min(ceil(512 / min(every_burnin, every_sample)), max(1, 64 MiB / (n_params * F * 8))) rows (at most MMG_OPT_DIFF_TRACE_ROWS, if set), and
 * 2 * 496 bytes of launch descriptors) and two of each in pinned host memory.  MMG_ERR_ARG for an interval of 0 or above
 * 2^30 = 1073741824, or once the burn-in has run. */
int mmg_diff_trace_open(mmg_diff *h, uint32_t every_burnin, uint32_t every_sample, mmg_diff_trace_sink sink, void *user);
/* After the burn-in: mean_lo[F] = (the sum of the log odds since the feature's last tuning step) / 128 and logitp[F] = logit p' as
 * they stand -- before tuning batch b >= 1 what BMS::printtune prints at its start, for tuned (frozen) features too.  Either may be NULL. */
int mmg_diff_get_tune_state(mmg_diff *h, double *mean_lo, double *logitp);
/* After the burn-in: the pseudopriors as out[n_pseudo][F], in the column order of BMS::print_pseudo -- per model A, Valpha; B, Vbeta
 * per column of M; F, Veta, S = 1 / S_inv per column of P; J, L per class; Q, R. */
int mmg_diff_get_pseudo(mmg_diff *h, double *out);
/* Self test, no device: the row buffer and one launch of a traced run as mmg_diff_trace_open and the traced phases plan them.  *cap = the
 * rows a buffer holds for n_params x n_features at the denser interval every_min (max_rows: MMG_OPT_DIFF_TRACE_ROWS, 0 = none); the
 * launch at phase index tt with `left` iterations to go at interval `every` covers *n iterations and rows [*first_row, *first_row + *rows). */
int mmg_selftest_diff_trace_plan(uint32_t n_params, uint32_t n_features, uint32_t every_min, uint32_t max_rows, uint32_t tt, uint32_t left,
                                 uint32_t every, uint32_t *cap, uint32_t *first_row, uint32_t *rows, uint32_t *n);

/* ---- mmdiff: effects (credible intervals of alpha, beta, eta, ... from the chain's own rows, on the device).  Additive in ABI
 * version 8.  DESIGN.md section 10.3. ----
 * Before mmg_diff_burnin: keep row r = the state after sampling iteration r * every (counted from the first sampling iteration, the
 * rule of mmg_diff_trace_open) of every traced parameter and gamma in one buffer [max_rows][n_params][F] on the device.  Burn-in and
 * tuning run as on a plain handle and the chain is the plain handle's, bit for bit; mmg_diff_sample may be called again and recording
 * continues, and a call that would need a row beyond max_rows returns MMG_ERR_ARG before it launches anything.  mmg_diff_device_bytes
 * grows by max_rows * n_params * F * 8 + 496 bytes (the launch descriptor): 2.3 GB at 20 000 features, 14 parameters and 1024 rows.
 * MMG_ERR_ARG for every outside [1, 2^30], max_rows outside [1, 4096], or once the burn-in has run; MMG_ERR_STATE while
 * mmg_diff_trace_open is open on the handle (and mmg_diff_trace_open returns it after this call) or when called twice. */
int mmg_diff_effects_open(mmg_diff *h, uint32_t every, uint32_t max_rows);
typedef struct mmg_effects mmg_effects;
/* The summary of the rows recorded so far (MMG_ERR_STATE before the first sampling call, or without mmg_diff_effects_open); the
 * handle's rows stay and sampling may go on.  Parameter s belongs to model m(s), the digit after its name's stem (alpha1: 1), and its
 * draws for a feature are the rows whose own gamma equals m(s), in row order; n of them:
 *   n[m][F]          the rows with gamma == m
 *   mean, sd         [n_params - 1][F]: the sequential sum over n, and sqrt(sum (x - mean)^2 / (n - 1)), summed sequentially in a second pass
 *   n_gt             [n_params - 1][F]: the draws with x > 0 (neither zero counts)
 *   q                [n_params - 1][np][F]: the sorted draw at index floor(percentiles[j] / 100 * (n - 1) + 0.5)
 * mean, sd and q are NaN for n == 0, sd for n == 1.  MMG_ERR_ARG, before any device work: a percentile outside [0, 100], np > 32, a
 * NULL array, more than 4096 rows. */
int mmg_diff_effects_summarize(mmg_diff *h, uint32_t np, const double *percentiles, mmg_effects **out);
/* The same summary of host rows[S][P][F] (gamma = parameter P - 1, every value 0.0 or 1.0: MMG_ERR_ARG otherwise) with model_of[P - 1]
 * (0 or 1) the model of each parameter.  MMG_ERR_ARG also for S == 0, S > 4096, P < 2, F == 0. */
int mmg_effects_of_rows(int device, uint32_t S, uint32_t P, uint32_t F, const double *rows, const uint8_t *model_of, uint32_t np,
                        const double *percentiles, mmg_effects **out);
/* The results, which stay on the device until here; any pointer may be NULL. */
int mmg_effects_get(mmg_effects *e, uint32_t *n, double *mean, double *sd, uint32_t *n_gt, double *q);
/* what the results hold: 8 F + (P - 1) F (20 + 8 np) + 8 np + (P - 1) bytes */
int mmg_effects_device_bytes(mmg_effects *e, uint64_t *bytes);
void mmg_effects_destroy(mmg_effects *e);

/* ---- mmdiff, polytomous: J alternatives against one model 0 on one handle ------------------------------------------------
 * Comparison j (0 <= j < J <= 16) is model 0 against alternative j, and its chain is bit for bit the chain of an mmg_diff handle
 * created from the same y, e, M, P0, alternative and seed and driven the same way: the stream key holds no comparison index.  y, e,
 * M and P0 are held once; every launch covers all comparisons.  Additive in ABI version 8. */
typedef struct mmg_diff_poly mmg_diff_poly;
/* As mmg_diff_create, with C0: [N] the classes under model 0, L1: [J] the columns of each alternative's P1, P1: the J matrices
 * [N][L1[j]] one after the other, C1: [J][N] the classes under each alternative. */
int mmg_diff_poly_create(int device, uint32_t n_features, uint32_t n_samples, const double *y, const double *e, uint32_t K, const double *M,
                         uint32_t L0, const double *P0, const int32_t *C0, uint32_t J, const uint32_t *L1, const double *P1,
                         const int32_t *C1, double d, double s, double pdash, int fixalpha, uint64_t seed, mmg_diff_poly **out);
int mmg_diff_poly_burnin(mmg_diff_poly *h, uint32_t iters);
/* One tuning batch for every comparison that has not ended tuning.  untuned[J]: the features of comparison j still untuned after the
 * batch's tuning step (0 for a comparison that had ended before).  A comparison whose count is 0 has ended: it takes no part in later
 * batches and keeps its batch count.  ended[J] (may be NULL): 1 for the comparisons that have ended, this batch included.  The caller
 * stops at its batch limit; mmg_diff_poly_sample then starts every comparison at its own index, burnin + 128 * (its batches). */
int mmg_diff_poly_tune_batch(mmg_diff_poly *h, uint32_t *untuned, int32_t *ended);
int mmg_diff_poly_sample(mmg_diff_poly *h, uint32_t iters);
/* comparison j's results, laid out as mmg_diff_get_results lays them out (eta: [L0 + L1[j]][F]) */
int mmg_diff_poly_get_results(mmg_diff_poly *h, uint32_t j, double *gamma_mean, double *logitp, double *alpha, double *beta, double *eta);
/* comparison j: flags[3] = (M nil, P0 nil, P1 nil), n_classes[2], its tuning batches, whether it has ended tuning; any pointer may be NULL */
int mmg_diff_poly_info(mmg_diff_poly *h, uint32_t j, int32_t *flags, uint32_t *n_classes, uint32_t *batches, int32_t *ended);
/* 8 (2 F N + N K + N L0 + sum_j (F nslot_j + N L1_j)) + 4 sum_j (2 N + 2 F) + 488 J bytes (nslot_j: DESIGN.md section 10) */
int mmg_diff_poly_device_bytes(mmg_diff_poly *h, uint64_t *bytes);
void mmg_diff_poly_destroy(mmg_diff_poly *h);

/* ---- mmdiff, several chains: C independent chains of one comparison on one handle, pooled ------------------------------------
 * Chain c (0 <= c < C <= 16) draws from the streams (seed, c, TAG_DIFF, feature, iteration).  The stream key is
 * (seed >> 32) ^ chain ^ (tag << 24), so chain c is bit for bit the chain of an mmg_diff handle created from the same inputs with
 * seed ^ ((uint64_t)c << 32) and driven the same way; chain 0 is the chain of mmg_diff_create.  y, e, M, P0, P1 and the classes are
 * held once; every launch covers all chains; each chain tunes on its own, as a comparison of mmg_diff_poly_* does.  Additive in ABI
 * version 8. */
typedef struct mmg_diff_chains mmg_diff_chains;
/* As mmg_diff_create, with the number of chains and the total number of sampling iterations (a positive multiple of 16): the
 * sampling run is cut into 16 batches of sample_total / 16 iterations whose sums of gamma are kept per chain and feature. */
int mmg_diff_chains_create(int device, uint32_t n_features, uint32_t n_samples, const double *y, const double *e, uint32_t K, const double *M,
                           uint32_t L0, const double *P0, uint32_t L1, const double *P1, const int32_t *C, double d, double s, double pdash,
                           int fixalpha, uint64_t seed, uint32_t n_chains, uint32_t sample_total, mmg_diff_chains **out);
int mmg_diff_chains_burnin(mmg_diff_chains *h, uint32_t iters);
/* One tuning batch for every chain that has not ended tuning: untuned[C], ended[C] (may be NULL) as mmg_diff_poly_tune_batch fills
 * them per comparison.  mmg_diff_chains_sample starts chain c at its own index, burnin + 128 * (its batches). */
int mmg_diff_chains_tune_batch(mmg_diff_chains *h, uint32_t *untuned, int32_t *ended);
/* iters more sampling iterations of every chain; MMG_ERR_ARG if that would pass sample_total in all */
int mmg_diff_chains_sample(mmg_diff_chains *h, uint32_t iters);
/* the pooled estimates, once sample_total iterations have been sampled */
int mmg_diff_chains_pool(mmg_diff_chains *h);
/* chain c's results, laid out as mmg_diff_get_results lays them out */
int mmg_diff_chains_get_results(mmg_diff_chains *h, uint32_t c, double *gamma_mean, double *logitp, double *alpha, double *beta, double *eta);
/* sums[16][F]: chain c's sum of gamma over each sixteenth of the sampling run (integers; their sum is gamma_mean * iterations sampled) */
int mmg_diff_chains_get_batch_sums(mmg_diff_chains *h, uint32_t c, double *sums);
/* log_bf[F], log_bf_sd[F], log_bf_mcse[F], chains_mixed[F]; alpha, beta, eta laid out as mmg_diff_get_results lays them out, each the
 * chains' summed sums over their summed counts; any pointer may be NULL.  After mmg_diff_chains_pool. */
int mmg_diff_chains_get_pooled(mmg_diff_chains *h, double *log_bf, double *log_bf_sd, double *log_bf_mcse, uint32_t *chains_mixed,
                               double *alpha, double *beta, double *eta);
/* chain c: flags[3] = (M nil, P0 nil, P1 nil), n_classes[2], its tuning batches, whether it has ended tuning; any pointer may be NULL */
int mmg_diff_chains_info(mmg_diff_chains *h, uint32_t c, int32_t *flags, uint32_t *n_classes, uint32_t *batches, int32_t *ended);
/* 8 (2 F N + N K + N L0 + N L1 + C F (nslot + 16) + F (8 + 4 K + 2 L0 + 2 L1)) + 4 (2 N + 2 C F) + 488 C bytes (nslot: DESIGN.md
 * section 10) */
int mmg_diff_chains_device_bytes(mmg_diff_chains *h, uint64_t *bytes);
void mmg_diff_chains_destroy(mmg_diff_chains *h);

/* ---- mmdiff, a permutation null: the data and B shuffled copies of it on one handle, q-values --------------------------------
 * The handle holds R = n_perm + 1 replicas (1 <= n_perm <= 31: the tuning launch takes a 32-bit mask of replicas).  Replica 0 is
 * the data as given; replica b >= 1 is the data with every feature's samples shuffled on the device: a Fisher-Yates on the
 * replica's own column, for j = N - 1 .. 1: k = min((size_t)(u (j + 1)), j), entries j and k of y and e^2 swapped, u the next
 * uniform of SeqStream(Stream(seed, b, TAG_DIFF_PERM, feature, 0)).  The stream key is (seed >> 32) ^ chain ^ (tag << 24), so that
 * is the shuffle mmdiff -permute applies with the seed seed ^ ((uint64_t)b << 32), and replica b draws its chain from the streams
 * (seed, b, TAG_DIFF, ...): replica b is bit for bit the mmg_diff handle created from that -permute data with the seed
 * seed ^ ((uint64_t)b << 32) and driven the same way; replica 0 is the handle of mmg_diff_create.  Every replica has its own y, e^2,
 * state block and tuning state; M, P0, P1 and the classes are held once; every launch covers all replicas, and each replica tunes on
 * its own, as a chain of mmg_diff_chains_* does.  Additive in ABI version 8. */
typedef struct mmg_diff_perm mmg_diff_perm;
int mmg_diff_perm_create(int device, uint32_t n_features, uint32_t n_samples, const double *y, const double *e, uint32_t K, const double *M,
                         uint32_t L0, const double *P0, uint32_t L1, const double *P1, const int32_t *C, double d, double s, double pdash,
                         int fixalpha, uint64_t seed, uint32_t n_perm, mmg_diff_perm **out);
/* iters: a positive multiple of 1024, as for mmg_diff_chains_burnin */
int mmg_diff_perm_burnin(mmg_diff_perm *h, uint32_t iters);
/* One tuning batch for every replica that has not ended tuning: untuned[R], ended[R] (may be NULL) as mmg_diff_poly_tune_batch fills
 * them per comparison.  mmg_diff_perm_sample starts replica b at its own index, burnin + 128 * (its batches). */
int mmg_diff_perm_tune_batch(mmg_diff_perm *h, uint32_t *untuned, int32_t *ended);
int mmg_diff_perm_sample(mmg_diff_perm *h, uint32_t iters);
/* replica b's results, laid out as mmg_diff_get_results lays them out; MMG_ERR_ARG for b >= R */
int mmg_diff_perm_get_results(mmg_diff_perm *h, uint32_t b, double *gamma_mean, double *logitp, double *alpha, double *beta, double *eta);
/* replica b: flags[3] = (M nil, P0 nil, P1 nil), n_classes[2], its tuning batches, whether it has ended tuning; any pointer may be NULL */
int mmg_diff_perm_info(mmg_diff_perm *h, uint32_t b, int32_t *flags, uint32_t *n_classes, uint32_t *batches, int32_t *ended);
/* After sampling (MMG_ERR_STATE before): per replica and feature the log Bayes factor T = log(g) - log(1 - g) - logit p', g the mean
 * of gamma (the library's own log; -inf for g == 0, +inf for g == 1, NaN for a logit p' that is not finite), and mmg_qvalues of
 * replica 0's T against the pooled T of replicas 1 .. B.  Everything stays on the device; sampling further makes it stale. */
int mmg_diff_perm_qvalues(mmg_diff_perm *h);
/* stat[R][F], null_ge[F], q[F] of the last mmg_diff_perm_qvalues (MMG_ERR_STATE without one); any pointer may be NULL */
int mmg_diff_perm_get_qvalues(mmg_diff_perm *h, double *stat, uint64_t *null_ge, double *q);
/* 8 (2 R F N + N K + N L0 + N L1 + R F (nslot + 1) + 2 F) + 4 (2 N + 2 R F) + 488 R bytes (nslot: DESIGN.md section 10); the working
 * memory of mmg_diff_perm_qvalues is taken and given back inside the call and not counted */
int mmg_diff_perm_device_bytes(mmg_diff_perm *h, uint64_t *bytes);
void mmg_diff_perm_destroy(mmg_diff_perm *h);

/* q-values of F observed statistics against n_null null statistics (host arrays; computed on `device`).  With m and m0 the observed
 * and null values that are not NaN, -0.0 equal to 0.0, R(t) the observed values >= t and V(t) the null values >= t:
 *   fdr(t) = min(1, ((double)V(t) * (double)m) / ((double)m0 * (double)R(t))),
 *   q[f] = min { fdr(t') : t' an observed value, t' <= obs[f] },   null_ge[f] = V(obs[f]).
 * An observed NaN gets q = NaN and null_ge = 0 and counts in no R; with m0 == 0 every q is NaN.
 * MMG_ERR_ARG for F == 0, n_null == 0, n_null > 2^31 - 1 or a NULL pointer. */
int mmg_qvalues(int device, uint32_t F, const double *obs, uint64_t n_null, const double *null, uint64_t *null_ge, double *q);

/* ---- mmdiff -lrt: the per-feature likelihood-ratio test ---------------------------------------------
 * Both models of mmg_diff_create fitted by maximum likelihood, without priors: y_i ~ N((X_m theta_m)_i, e_i^2 + sigma^2_{C_m(i)}),
 * X_m = [1 unless fixalpha | M unless nil | P_m unless nil] with p_m columns, theta_m free, sigma^2_c >= 0 per variance class;
 * l_m = -1/2 sum_i [log 2 pi + log v_i + r_i^2 / v_i].  One lane per feature profiles theta by weighted least squares and moves
 * sigma^2 by projected Fisher scoring with step halving, from sigma^2_c = the class mean of e_i^2, for at most max_iters scoring
 * iterations per model (0: the default, 200).  No sampler, no stream: reruns are bit-identical.  The model sets are not checked for
 * nesting.  Additive in ABI version 8. */
typedef struct mmg_diff_lrt mmg_diff_lrt;
/* Arguments, caps and refusals as mmg_diff_create (MMG_ERR_ARG with the same messages, before any device work).  The call computes
 * everything, keeps the results on the host and holds no device memory when it returns. */
int mmg_diff_lrt_create(int device, uint32_t n_features, uint32_t n_samples, const double *y, const double *e, uint32_t K, const double *M,
                        uint32_t L0, const double *P0, uint32_t L1, const double *P1, const int32_t *C, int fixalpha, uint32_t max_iters,
                        mmg_diff_lrt **out);
/* loglik[2][F]; stat[F] = 2 (l_1 - l_0); df = (p_1 + classes_1) - (p_0 + classes_0); p_value[F] = Q(df / 2, max(stat, 0) / 2), NaN for
 * df <= 0 or a NaN stat; q_value[F]: Benjamini-Hochberg over the p that are not NaN, ties in input order; theta0[p_0][F], theta1[p_1][F]
 * in the column order of X_m; sigmasq0[classes_0][F], sigmasq1[classes_1][F]; iters[2][F] the scoring iterations used; status[2][F]
 * bits: 1 the cap was reached before the stopping rule held, 2 X'WX is not positive definite or a weight is not finite (l, theta
 * and sigma^2 of that model are NaN, iters 0; the bit stands alone), 4 some sigma^2_c is 0 (the estimate is on the boundary, where
 * the chi-squared reference is conservative).  Any pointer may be NULL. */
int mmg_diff_lrt_get(mmg_diff_lrt *h, double *loglik, double *stat, double *p_value, double *q_value, int32_t *df, double *theta0,
                     double *theta1, double *sigmasq0, double *sigmasq1, uint32_t *iters, uint32_t *status);
/* flags[3] as mmg_diff_info (M, P0, P1 nil), n_classes[2], n_cols[2] = p_0, p_1; any pointer may be NULL */
int mmg_diff_lrt_info(mmg_diff_lrt *h, int32_t *flags, uint32_t *n_classes, uint32_t *n_cols);
/* The peak during creation: 8 (2 F N + (N + F) (p_0 + p_1) + F (classes_0 + classes_1) + 2 F + F W) + 4 (2 N + 4 F) bytes, with
 * W = 2 max(classes_0, classes_1) + (pm <= 4 ? 0 : pm (pm + 1) / 2) workspace slots per feature, pm = max(p_0, p_1). */
int mmg_diff_lrt_device_bytes(mmg_diff_lrt *h, uint64_t *bytes);
void mmg_diff_lrt_destroy(mmg_diff_lrt *h);

/* ---- mmdiff -lrt FILE -lrtperm B: a permutation null for the likelihood-ratio test ------------------
 * The test of mmg_diff_lrt_create on the data (copy 0) and on B shuffled copies of it.  Copy b = 1 .. B is the data with every
 * feature's samples shuffled as replica b of mmg_diff_perm_create shuffles them (a Fisher-Yates keyed (seed, b, feature), y and e moved
 * together); its statistic T[b][f] = 2 (l_1 - l_0) is, bit for bit, the stat of mmg_diff_lrt_create on that copy, NaN where a fit has
 * status 2.  The copies are fitted slab_copies at a time (0: as many as keep the slab and its workspace under 1 GiB, at least 1);
 * no result depends on it.  Additive in ABI version 8. */
typedef struct mmg_diff_lrt_perm mmg_diff_lrt_perm;
/* Arguments, caps, refusals and messages as mmg_diff_lrt_create; also MMG_ERR_ARG, before any device work, for n_perm outside
 * 1 .. 65535 and for n_perm * n_features > 2^31 - 1 (mmg_qvalues' cap on the null).  The call computes everything, keeps the results
 * on the host and holds no device memory when it returns. */
int mmg_diff_lrt_perm_create(int device, uint32_t n_features, uint32_t n_samples, const double *y, const double *e, uint32_t K, const double *M,
                             uint32_t L0, const double *P0, uint32_t L1, const double *P1, const int32_t *C, int fixalpha, uint32_t max_iters,
                             uint32_t n_perm, uint64_t seed, uint32_t slab_copies, mmg_diff_lrt_perm **out);
/* The test on the data: every output bit-identical to mmg_diff_lrt_create on the same arguments.  Borrowed: read it with
 * mmg_diff_lrt_get / _info / _device_bytes, do not destroy it; it goes with h. */
mmg_diff_lrt *mmg_diff_lrt_perm_observed(mmg_diff_lrt_perm *h);
/* Per feature against its own copies: perm_ge[F] = #{b : T[b][f] >= T[0][f]}, perm_n[F] = #{b : T[b][f] is not NaN},
 * perm_p[F] = (double)(1 + perm_ge) / (double)(1 + perm_n); a NaN copy counts in neither, -0.0 equals 0.0, an observed NaN gives
 * perm_p NaN and perm_ge 0.  Pooled: null_ge[F], q_perm[F] = mmg_qvalues(obs = T[0][.], null = T[1 .. B][.]).  Any pointer may be NULL. */
int mmg_diff_lrt_perm_get(mmg_diff_lrt_perm *h, uint64_t *perm_ge, uint64_t *perm_n, double *perm_p, uint64_t *null_ge, double *q_perm);
/* Copies b0 + 1 .. b0 + nb: stat[nb][F] and status[nb][F] = status0 | status1 << 4 (the bits of mmg_diff_lrt_get).  MMG_ERR_ARG for
 * b0 + nb > B; either pointer may be NULL. */
int mmg_diff_lrt_perm_get_null(mmg_diff_lrt_perm *h, uint32_t b0, uint32_t nb, double *stat, uint8_t *status);
/* The peak of the handle's own device memory during creation: mmg_diff_lrt_device_bytes of the observed test
 *   + 8 Sc F (2 N + W') + 9 B F + 48 F bytes,
 * with Sc the copies of one slab (y and e^2 of each, [Sc][N][F]), W' = 3 max(classes_0, classes_1) + (pm <= 4 ? 0 : pm (pm + 1) / 2 + pm)
 * workspace slots per copy and feature, 9 B F the statistics and status bytes of the copies, 48 F the six per-feature results.  The
 * slab and its workspace are released before the q-values; mmg_qvalues' working memory (40 F + 16 B F + 16 bytes and the sorts') is
 * taken and given back inside the call and not counted. */
int mmg_diff_lrt_perm_device_bytes(mmg_diff_lrt_perm *h, uint64_t *bytes);
void mmg_diff_lrt_perm_destroy(mmg_diff_lrt_perm *h);

#ifdef __cplusplus
}
#endif
#endif /* MMGIBBS_H */
