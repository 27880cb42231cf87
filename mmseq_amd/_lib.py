"""ctypes loader for libmmgibbs.so (the C ABI declared in include/mmgibbs.h).

The library is built in-tree (mmseq_amd/csrc/Makefile, via __graft_entry__.build()).
There is no fallback: if the shared object is missing, loading raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# MMSEQ_AMD_LIB: another build of the same library (A/B timing of kernel changes on one box, tools/k1_ab.py)
LIB_PATH = os.environ.get("MMSEQ_AMD_LIB") or os.path.join(_HERE, "csrc", "libmmgibbs.so")
_lib = None


def _point_rccl_at_pytorchs_copy():
    """One RCCL per process: the library loads RCCL on first use of a device group (dlopen); a Python process that ALSO imports torch
    (mmseq_amd/dist.py does) must not get /opt/rocm's build from here and PyTorch's bundled one from torch -- two builds in one process
    crash in the exit handlers.  So when a PyTorch installation carries its own librccl, MMG_RCCL_LIBRARY (read by csrc/group.hip)
    names that file; whichever of the two loads it first, the other gets the same handle.  torch itself is not imported here."""
    if os.environ.get("MMG_RCCL_LIBRARY"):
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        return
    for base in (spec.submodule_search_locations or []) if spec else []:
        cand = os.path.join(base, "lib", "librccl.so")
        if os.path.exists(cand):
            os.environ["MMG_RCCL_LIBRARY"] = cand
            return


class MMGError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libmmgibbs error %d: %s" % (code, msg))
        self.code = code


LAYOUT_CANONICAL, LAYOUT_KEEP_ROWS = 0, 1
# mmg_selftest_option ids
OPT_SAMPLE_KERNEL, OPT_FORCE_IDX64, OPT_SELL_WAVES_PER_CU, OPT_EM_KERNEL, OPT_EM_GRID, OPT_FUSE_CHAINS, OPT_CNT_REPLICAS, OPT_GROUP_FAIL, OPT_DERIVE_ORDER, OPT_WIRE_CHECK, OPT_BIGK_PER_WAVE, OPT_BIGK_SIDE_STREAM, OPT_FAIL_ALLOC, OPT_CONV_SLAB, OPT_DIFF_TRACE_ROWS, OPT_ASSIGN_WAVES, OPT_CONTRAST_SLAB, OPT_POOL_SLAB, OPT_PAIRS_SLAB, OPT_FOLD_SLAB, OPT_SIM_CHUNK, OPT_ISO_SLAB, OPT_K1_LEAN, OPT_K1_RANGE_COST, OPT_K1_RANGES, OPT_SERIES_GROUPS = range(26)


class ProblemDesc(C.Structure):
    _fields_ = [("m", C.c_uint64), ("n", C.c_uint32), ("row_ptr", C.c_void_p), ("col_idx", C.c_void_p),
                ("k", C.c_void_p), ("l", C.c_void_p), ("row_id_base", C.c_uint64), ("layout", C.c_uint32),
                ("tx_order", C.c_void_p)]


class SynthDesc(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("rows", C.c_uint64), ("row0", C.c_uint64), ("n", C.c_uint32),
                ("avg_hits", C.c_double), ("uniform", C.c_int32), ("sorted", C.c_int32),
                ("mapped_reads", C.c_uint64), ("far_fraction", C.c_double), ("gene_size", C.c_uint32), ("far_family", C.c_uint32)]


class ProblemInfo(C.Structure):
    _fields_ = [("m", C.c_uint64), ("nnz", C.c_uint64), ("total_k", C.c_uint64), ("row_id_base", C.c_uint64),
                ("n", C.c_uint32), ("max_row_len", C.c_uint32), ("n_tiles", C.c_uint64),
                ("device_bytes", C.c_uint64), ("index_bits", C.c_int32), ("sample_kernel", C.c_int32),
                ("stream_bytes", C.c_uint64), ("fast_tiles", C.c_uint64), ("far_tiles", C.c_uint64), ("padded_slots", C.c_uint64),
                ("layout", C.c_int32), ("tx_renumbered", C.c_int32), ("sample_grid", C.c_int32), ("cu_count", C.c_int32)]


class K1Info(C.Structure):
    _fields_ = [("lean", C.c_int32), ("fixed_walk", C.c_int32), ("range_tile_cost", C.c_int32), ("reserved", C.c_int32),
                ("n_ranges", C.c_uint64), ("range_cost_max", C.c_uint64), ("range_cost_mean", C.c_double),
                ("range_tiles_max", C.c_uint64), ("n_list", C.c_uint64), ("list_cost", C.c_uint64)]


class SummaryDesc(C.Structure):
    _fields_ = [("chain", C.c_int32), ("n_virtual", C.c_uint32), ("virtual_id", C.c_void_p), ("virtual_scale", C.c_void_p),
                ("n_identical", C.c_uint32), ("identical_ptr", C.c_void_p), ("identical_member", C.c_void_p),
                ("n_genes", C.c_uint32), ("gene_ptr", C.c_void_p), ("gene_member", C.c_void_p),
                ("n_percentiles", C.c_uint32), ("percentile_index", C.c_void_p)]


class ContrastDesc(C.Structure):
    _fields_ = [("n_contrasts", C.c_uint32), ("num_ptr", C.c_void_p), ("num_member", C.c_void_p), ("den_ptr", C.c_void_p),
                ("den_member", C.c_void_p), ("n_percentiles", C.c_uint32), ("percentile_index", C.c_void_p)]


class IsoformDesc(C.Structure):
    _fields_ = [("n_groups", C.c_uint32), ("ptr", C.c_void_p), ("member", C.c_void_p), ("n_thresholds", C.c_uint32), ("threshold", C.c_void_p),
                ("n_ranks", C.c_uint32), ("rank", C.c_void_p)]


class Config(C.Structure):
    _fields_ = [("alpha", C.c_double), ("beta", C.c_double), ("seed", C.c_uint64), ("n_chains", C.c_int32),
                ("chain_base", C.c_int32), ("gibbs_iter", C.c_int32), ("trace_len", C.c_int32),
                ("keep_trace", C.c_int32), ("timing", C.c_int32)]


class KeyedIO(C.Structure):
    _fields_ = [("n_streams", C.c_int64), ("seed", C.c_void_p), ("id", C.c_void_p), ("chain", C.c_void_p), ("tag", C.c_void_p),
                ("iter", C.c_void_p), ("shape", C.c_void_p), ("scale", C.c_double), ("out_uniforms", C.c_void_p),
                ("out_words", C.c_void_p), ("out_gamma", C.c_void_p),
                ("n_math", C.c_int64), ("x", C.c_void_p), ("normal_seed", C.c_uint64), ("out_probit", C.c_void_p),
                ("out_lgamma", C.c_void_p), ("out_normal", C.c_void_p), ("out_stirling", C.c_void_p), ("out_ilogb", C.c_void_p),
                ("n_words", C.c_int64), ("w0", C.c_void_p), ("w1", C.c_void_p), ("t", C.c_void_p), ("out_u32", C.c_void_p),
                ("out_u52", C.c_void_p), ("out_target", C.c_void_p)]


class BigkPoints(C.Structure):
    _fields_ = [("n_inv", C.c_int64), ("inv_n", C.c_void_p), ("inv_p", C.c_void_p), ("inv_u", C.c_void_p), ("inv_slack", C.c_double),
                ("out_inv_bound", C.c_void_p), ("out_inv_x", C.c_void_p), ("out_inv_pre", C.c_void_p),
                ("n_btrs", C.c_int64), ("btrs_n", C.c_void_p), ("btrs_p", C.c_void_p), ("btrs_u", C.c_void_p), ("btrs_v", C.c_void_p),
                ("out_btrs_kf", C.c_void_p), ("out_btrs_reach", C.c_void_p), ("out_btrs_exact", C.c_void_p), ("out_btrs_diff", C.c_void_p),
                ("out_btrs_d32", C.c_void_p), ("out_btrs_e32", C.c_void_p), ("out_btrs_pre", C.c_void_p)]


class Timing(C.Structure):
    _fields_ = [("sample_ms", C.c_double), ("update_ms", C.c_double), ("sample_launches", C.c_uint64),
                ("update_launches", C.c_uint64)]


# every symbol include/mmgibbs.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "mmg_last_error": (C.c_char_p, []),
    "mmg_abi_version": (C.c_int, []),
    "mmg_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "mmg_problem_create": (C.c_int, [C.POINTER(ProblemDesc), C.c_int, C.POINTER(C.c_void_p)]),
    "mmg_problem_create_synthetic": (C.c_int, [C.POINTER(SynthDesc), C.c_int, C.POINTER(C.c_void_p)]),
    "mmg_problem_info_get": (C.c_int, [C.c_void_p, C.POINTER(ProblemInfo)]),
    "mmg_problem_k1_info_get": (C.c_int, [C.c_void_p, C.POINTER(K1Info)]),
    "mmg_problem_k1_ranges": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_selftest_k1_kernel_info": (C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mmg_selftest_k1_lists": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mmg_problem_download": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_problem_tx_perm": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mmg_selftest_option": (C.c_int, [C.c_int, C.c_int]),
    "mmg_selftest_live": (C.c_int, [C.c_void_p]),
    "mmg_selftest_series_launch": (C.c_int, [C.c_int, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
    "mmg_selftest_sampler_events": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mmg_selftest_kernel_info": (C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mmg_problem_get_l": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mmg_problem_start_values": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_problem_em": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.POINTER(C.c_int),
                                 C.POINTER(C.c_double)]),
    "mmg_problem_destroy": (None, [C.c_void_p]),
    "mmg_em_create": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_double)]),
    "mmg_em_step": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "mmg_em_get_mu": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mmg_em_stats": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "mmg_em_destroy": (None, [C.c_void_p]),
    "mmg_sampler_create": (C.c_int, [C.c_void_p, C.POINTER(Config), C.c_void_p, C.POINTER(C.c_void_p)]),
    "mmg_sampler_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mmg_sampler_run": (C.c_int, [C.c_void_p, C.c_int]),
    "mmg_sampler_extend": (C.c_int, [C.c_void_p]),
    "mmg_sampler_sample": (C.c_int, [C.c_void_p]),
    "mmg_sampler_update": (C.c_int, [C.c_void_p]),
    "mmg_sampler_counts_devptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "mmg_sampler_moments_devptr": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]),
    "mmg_sampler_sync": (C.c_int, [C.c_void_p]),
    "mmg_sampler_wait_iterations": (C.c_int, [C.c_void_p, C.c_int]),
    "mmg_sampler_iteration": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "mmg_sampler_get_trace": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "mmg_sampler_get_trace_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mmg_sampler_get_trace_rows_done": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mmg_sampler_get_mu": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "mmg_sampler_get_counts": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "mmg_sampler_get_moments": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    "mmg_sampler_get_timing": (C.c_int, [C.c_void_p, C.POINTER(Timing)]),
    "mmg_sampler_reset_timing": (C.c_int, [C.c_void_p]),
    "mmg_sampler_destroy": (None, [C.c_void_p]),
    "mmg_summary_create": (C.c_int, [C.c_void_p, C.POINTER(SummaryDesc), C.POINTER(C.c_void_p)]),
    "mmg_summary_begin": (C.c_int, [C.c_void_p, C.POINTER(SummaryDesc), C.POINTER(C.c_void_p)]),
    "mmg_summary_advance": (C.c_int, [C.c_void_p, C.c_int]),
    "mmg_summary_finish": (C.c_int, [C.c_void_p]),
    "mmg_summary_get": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_summary_get_proportions": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_summary_get_rows": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]),
    "mmg_summary_destroy": (None, [C.c_void_p]),
    "mmg_collapse_create": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mmg_collapse_set_sample": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "mmg_collapse_correlate": (C.c_int, [C.c_void_p]),
    "mmg_collapse_get_rows": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "mmg_collapse_row_max": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mmg_collapse_run": (C.c_int, [C.c_void_p, C.c_double, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_collapse_device_bytes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mmg_collapse_destroy": (None, [C.c_void_p]),
    "mmg_diff_create": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                  C.c_uint32, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_uint64, C.c_void_p]),
    "mmg_diff_burnin": (C.c_int, [C.c_void_p, C.c_uint32]),
    "mmg_diff_tune_batch": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mmg_diff_sample": (C.c_int, [C.c_void_p, C.c_uint32]),
    "mmg_diff_get_results": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_diff_info": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_diff_device_bytes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mmg_diff_destroy": (None, [C.c_void_p]),
    "mmg_diff_lrt_create": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                      C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]),
    "mmg_diff_lrt_get": (C.c_int, [C.c_void_p] * 12),
    "mmg_diff_lrt_info": (C.c_int, [C.c_void_p] * 4),
    "mmg_diff_lrt_device_bytes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mmg_diff_lrt_destroy": (None, [C.c_void_p]),
    "mmg_diff_lrt_perm_create": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                           C.c_uint32, C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p]),
    "mmg_diff_lrt_perm_observed": (C.c_void_p, [C.c_void_p]),
    "mmg_diff_lrt_perm_get": (C.c_int, [C.c_void_p] * 6),
    "mmg_diff_lrt_perm_get_null": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mmg_diff_lrt_perm_device_bytes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mmg_diff_lrt_perm_destroy": (None, [C.c_void_p]),
    "mmg_diff_trace_layout": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_diff_trace_name": (C.c_int, [C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint32]),
    "mmg_diff_trace_open": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mmg_diff_get_tune_state": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_diff_get_pseudo": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mmg_selftest_diff_trace_plan": (C.c_int, [C.c_uint32] * 7 + [C.c_void_p] * 4),
    "mmg_diff_effects_open": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32]),
    "mmg_diff_effects_summarize": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p)]),
    "mmg_effects_of_rows": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                      C.POINTER(C.c_void_p)]),
    "mmg_effects_get": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_effects_device_bytes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mmg_effects_destroy": (None, [C.c_void_p]),
    "mmg_diff_poly_create": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                       C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int,
                                       C.c_uint64, C.c_void_p]),
    "mmg_diff_poly_burnin": (C.c_int, [C.c_void_p, C.c_uint32]),
    "mmg_diff_poly_tune_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_diff_poly_sample": (C.c_int, [C.c_void_p, C.c_uint32]),
    "mmg_diff_poly_get_results": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_diff_poly_info": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_diff_poly_device_bytes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mmg_diff_poly_destroy": (None, [C.c_void_p]),
    "mmg_diff_chains_create": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                         C.c_uint32, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_uint64, C.c_uint32,
                                         C.c_uint32, C.c_void_p]),
    "mmg_diff_chains_burnin": (C.c_int, [C.c_void_p, C.c_uint32]),
    "mmg_diff_chains_tune_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_diff_chains_sample": (C.c_int, [C.c_void_p, C.c_uint32]),
    "mmg_diff_chains_pool": (C.c_int, [C.c_void_p]),
    "mmg_diff_chains_get_results": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_diff_chains_get_batch_sums": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "mmg_diff_chains_get_pooled": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_diff_chains_info": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_diff_chains_device_bytes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mmg_diff_chains_destroy": (None, [C.c_void_p]),
    "mmg_diff_perm_create": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p,
                                       C.c_uint32, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int, C.c_uint64, C.c_uint32,
                                       C.c_void_p]),
    "mmg_diff_perm_burnin": (C.c_int, [C.c_void_p, C.c_uint32]),
    "mmg_diff_perm_tune_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_diff_perm_sample": (C.c_int, [C.c_void_p, C.c_uint32]),
    "mmg_diff_perm_get_results": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_diff_perm_info": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_diff_perm_qvalues": (C.c_int, [C.c_void_p]),
    "mmg_diff_perm_get_qvalues": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_diff_perm_device_bytes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mmg_diff_perm_destroy": (None, [C.c_void_p]),
    "mmg_qvalues": (C.c_int, [C.c_int, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_collapse_summarize": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_double,
                                         C.c_uint64, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "mmg_assign_create": (C.c_int, [C.c_int, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "mmg_assign_run_sampler": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "mmg_assign_run_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int]),
    "mmg_assign_get": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    "mmg_assign_device_bytes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mmg_assign_destroy": (None, [C.c_void_p]),
    "mmg_contrast_create": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(ContrastDesc), C.POINTER(C.c_void_p)]),
    "mmg_contrast_of_traces": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(ContrastDesc), C.POINTER(C.c_void_p)]),
    "mmg_contrast_get": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_contrast_get_rows": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]),
    "mmg_contrast_device_bytes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mmg_contrast_destroy": (None, [C.c_void_p]),
    "mmg_pairs_create": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "mmg_pairs_of_traces": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "mmg_pairs_get": (C.c_int, [C.c_void_p] * 9),
    "mmg_pairs_device_bytes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mmg_pairs_destroy": (None, [C.c_void_p]),
    "mmg_fold_of_traces": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_double, C.c_uint32, C.c_void_p,
                                     C.POINTER(C.c_void_p)]),
    "mmg_fold_create": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_double, C.c_uint32, C.c_void_p,
                                  C.POINTER(C.c_void_p)]),
    "mmg_fold_get": (C.c_int, [C.c_void_p] * 9),
    "mmg_fold_device_bytes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mmg_fold_destroy": (None, [C.c_void_p]),
    "mmg_sim_create": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]),
    "mmg_sim_set_sample": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_double]),
    "mmg_sim_run": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p]),
    "mmg_sim_get_used": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "mmg_sim_get_z": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]),
    "mmg_sim_get_gram": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    "mmg_sim_get": (C.c_int, [C.c_void_p] * 10),
    "mmg_sim_device_bytes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mmg_sim_destroy": (None, [C.c_void_p]),
    "mmg_isoform_create": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(IsoformDesc), C.POINTER(C.c_void_p)]),
    "mmg_isoform_of_traces": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_void_p, C.POINTER(IsoformDesc), C.POINTER(C.c_void_p)]),
    "mmg_isoform_get_members": (C.c_int, [C.c_void_p] * 4),
    "mmg_isoform_get_groups": (C.c_int, [C.c_void_p] * 10),
    "mmg_isoform_get_rows": (C.c_int, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_isoform_device_bytes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mmg_isoform_destroy": (None, [C.c_void_p]),
    "mmg_convergence_create": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "mmg_convergence_get": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_convergence_destroy": (None, [C.c_void_p]),
    "mmg_convergence_of_traces": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_pooled_create": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]),
    "mmg_pooled_get": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_pooled_get_chain": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_pooled_get_proportions": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_pooled_destroy": (None, [C.c_void_p]),
    "mmg_pooled_of_traces": (C.c_int, [C.c_int, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_pooled_device_bytes": (C.c_int, [C.c_void_p, C.c_void_p]),
    "mmg_group_create": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]),
    "mmg_group_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "mmg_group_destroy": (None, [C.c_void_p]),
    "mmg_group_run_sharded": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "mmg_group_run_chains": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int]),
    "mmg_group_enqueue_us": (C.c_int, [C.c_void_p, C.POINTER(C.c_double)]),
    "mmg_problem_shard": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]),
    "mmg_problem_shard_bounds": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "mmg_problem_shard_bounds_timed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "mmg_group_em_create": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]),
    "mmg_selftest_em_shards": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)]),
    "mmg_selftest_gibbs_shards": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "mmg_group_pool_moments": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_int64)]),
    "mmg_shard_bounds": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]),
    "mmg_host_gamma_trace": (C.c_int, [C.c_uint64, C.c_uint64, C.c_double, C.c_double, C.c_int, C.c_void_p]),
    "mmg_selftest_math": (C.c_int, [C.c_int, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_selftest_philox": (C.c_int, [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmg_selftest_gamma": (C.c_int, [C.c_int, C.c_uint64, C.c_double, C.c_double, C.c_int64, C.c_void_p]),
    "mmg_selftest_binomial": (C.c_int, [C.c_int, C.c_uint64, C.c_uint32, C.c_double, C.c_int64, C.c_void_p]),
    "mmg_selftest_btrs_pretest": (C.c_int, [C.c_int, C.c_uint64, C.c_int64, C.c_double, C.c_double, C.c_void_p]),
    "mmg_selftest_binv_pretest": (C.c_int, [C.c_int, C.c_uint64, C.c_int64, C.c_double, C.c_double, C.c_double, C.c_void_p]),
    "mmg_selftest_keyed": (C.c_int, [C.c_int, C.POINTER(KeyedIO)]),
    "mmg_selftest_bigk_points": (C.c_int, [C.c_int, C.POINTER(BigkPoints)]),
}


def _share_hip_runtime_with_torch():
    """PyTorch wheels bundle their own libamdhip64.so (same SONAME as /opt/rocm's).  Two HIP runtimes in
    one process cannot both own the GPU, so when torch is installed its copy is loaded first and
    libmmgibbs.so binds to it by SONAME; a later `import torch` then reuses the same object."""
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.origin:
            return
        cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:
        pass  # no torch (or an unusual layout): the system HIP runtime is used


def load():
    """Load libmmgibbs.so and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    _share_hip_runtime_with_torch()
    _point_rccl_at_pytorchs_copy()
    if not os.path.exists(LIB_PATH):
        raise OSError("libmmgibbs.so not built at %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(there is no CPU fallback)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        raise MMGError(rc, load().mmg_last_error().decode("utf-8", "replace"))
