"""ctypes binding of librnamc.so (the C ABI declared in include/rnamc.h).

The HIP extension is the product: if the shared library is missing this module
raises ImportError("... not built ...") — there is no CPU fallback and nothing
under oracle/ is ever imported from here.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RNAMC_LIB") or os.path.join(_HERE, "librnamc.so")

OK = 0
ERR_INVALID_ARG, ERR_INVALID_BASE, ERR_EMPTY_SEQ, ERR_SEQ_TOO_LONG = 1, 2, 3, 4
ERR_NO_DEVICE, ERR_OOM, ERR_HIP, ERR_IO, ERR_FORMAT = 5, 6, 7, 8, 9

# every entry point include/rnamc.h declares
SYMBOLS = [
    "rnamc_abi_version", "rnamc_params_sizeof", "rnamc_strerror", "rnamc_last_error",
    "rnamc_bytes2seq", "rnamc_bpp_len", "rnamc_bpp_index",
    "rnamc_fold_score_sets_new", "rnamc_fold_score_sets_accumulate",
    "rnamc_fold_score_sets_transfer", "rnamc_params_new", "rnamc_params_synthetic",
    "rnamc_params_save", "rnamc_params_load", "rnamc_params_field",
    "rnamc_params_set_special_hairpins", "rnamc_params_set_hairpin_limits",
    "rnamc_ctx_create", "rnamc_ctx_destroy", "rnamc_ctx_set", "rnamc_ctx_set_params",
    "rnamc_bpp_batch", "rnamc_bpp_batch_device", "rnamc_ctx_last_stats", "rnamc_ctx_stats",
    "rnamc_debug_fetch", "rnamc_debug_fetch_tree", "rnamc_fold_scores", "rnamc_fold_sums", "rnamc_centroid_fold",
    "rnamc_centroid_fold_multi",
    "rnamc_align_scores_new", "rnamc_align_scores_transfer", "rnamc_durbin_batch",
    "rnamc_pool_create", "rnamc_pool_destroy", "rnamc_pool_size", "rnamc_pool_ctx",
    "rnamc_pool_set_params", "rnamc_pool_set", "rnamc_bpp_batch_multi", "rnamc_shard_plan",
    "rnamc_sweep_cost", "rnamc_sample_batch", "rnamc_structure_score", "rnamc_mfe_batch",
    "rnamc_bpp_batch_constrained", "rnamc_bpp_batch_multi_constrained",
    "rnamc_sample_batch_constrained", "rnamc_mfe_batch_constrained", "rnamc_log_partition_batch",
    "rnamc_constraint_check", "rnamc_centroid_fold_batch", "rnamc_centroid_fold_batch_multi",
    "rnamc_bpp_batch_sparse", "rnamc_bpp_batch_sparse_multi",
    "rnamc_window_plan", "rnamc_bpp_windowed", "rnamc_bpp_windowed_multi",
    "rnamc_mutant_plan", "rnamc_mutant_scan", "rnamc_mutant_scan_multi",
    "rnamc_bpp_alignment", "rnamc_bpp_alignment_multi",
    "rnamc_context_profile_batch", "rnamc_context_profile_batch_multi", "rnamc_context_profile_stats",
    "rnamc_duplex_batch", "rnamc_duplex_batch_multi", "rnamc_duplex_score",
    "rnamc_match_align", "rnamc_match_align_mats", "rnamc_durbin_align_batch",
]


class RnamcError(RuntimeError):
    def __init__(self, status, detail=""):
        self.status = status
        msg = lib().rnamc_strerror(status).decode()
        if detail:
            msg += ": " + detail
        super().__init__(f"rnamc status {status}: {msg}")


class BatchStats(C.Structure):
    _fields_ = [
        ("n_groups", C.c_uint64), ("launches_inside", C.c_uint64),
        ("launches_outside", C.c_uint64), ("launches_other", C.c_uint64),
        ("ms_inside", C.c_double), ("ms_outside", C.c_double), ("ms_other", C.c_double),
        ("workspace_bytes", C.c_uint64),
        ("launches_outside_main", C.c_uint64), ("launches_outside_tail", C.c_uint64),
        ("launches_outside_small", C.c_uint64),
        ("ms_outside_main", C.c_double), ("ms_outside_tail", C.c_double),
        ("ms_outside_small", C.c_double), ("tree_side_stream", C.c_uint64),
        ("launches_window", C.c_uint64), ("ms_window", C.c_double),
        ("launches_mutant", C.c_uint64), ("ms_mutant", C.c_double),
    ]


_lib = None


def _preload_torch_hip():
    """One HIP runtime per process.  torch bundles its own libamdhip64.so / libhsa-runtime64.so;
    librnamc.so needs `libamdhip64.so.7`.  If librnamc is loaded first it brings in /opt/rocm's
    runtime, and a later `import torch` adds its bundled pair as a second HSA runtime, which
    then sees no GPU ("No HIP GPUs are available").  Loading torch's copy first (without
    importing torch) lets the dynamic loader satisfy librnamc's NEEDED entry with it (same
    SONAME) and torch find its own library already mapped.  RNAMC_NO_TORCH_PRELOAD=1 skips this
    (processes that never use torch and want /opt/rocm's runtime)."""
    import importlib.util
    import sys
    if os.environ.get("RNAMC_NO_TORCH_PRELOAD") == "1" or "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    path = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(path):
        try:
            C.CDLL(path, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    global _lib
    if _lib is not None:
        return _lib
    _preload_torch_hip()
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). rna_algos_amd has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    vp, u8p, u32p, u64p, f32p = C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), \
        C.POINTER(C.c_uint64), C.POINTER(C.c_float)
    L.rnamc_abi_version.restype = C.c_uint32
    L.rnamc_params_sizeof.restype = C.c_size_t
    L.rnamc_strerror.restype = C.c_char_p
    L.rnamc_strerror.argtypes = [C.c_int]
    L.rnamc_last_error.restype = C.c_char_p
    L.rnamc_bytes2seq.argtypes = [vp, C.c_uint64, vp]
    L.rnamc_bpp_len.restype = C.c_uint64
    L.rnamc_bpp_len.argtypes = [C.c_uint32]
    L.rnamc_bpp_index.restype = C.c_uint64
    L.rnamc_bpp_index.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    L.rnamc_fold_score_sets_new.argtypes = [C.c_float, vp]
    L.rnamc_fold_score_sets_accumulate.argtypes = [vp]
    L.rnamc_fold_score_sets_transfer.argtypes = [vp, vp]
    L.rnamc_params_new.argtypes = [C.c_float, vp]
    L.rnamc_params_synthetic.argtypes = [C.c_uint64, vp]
    L.rnamc_params_save.argtypes = [vp, C.c_char_p]
    L.rnamc_params_load.argtypes = [C.c_char_p, vp]
    L.rnamc_params_field.argtypes = [C.c_uint32, C.POINTER(C.c_char_p), u64p, u64p]
    L.rnamc_params_set_special_hairpins.argtypes = [vp, C.c_uint32, vp, vp, vp]
    L.rnamc_params_set_hairpin_limits.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32]
    L.rnamc_ctx_create.argtypes = [vp, C.c_int, C.c_uint64, C.POINTER(vp)]
    L.rnamc_ctx_destroy.argtypes = [vp]
    L.rnamc_ctx_destroy.restype = None
    L.rnamc_ctx_set.argtypes = [vp, C.c_char_p, C.c_int64]
    L.rnamc_ctx_set_params.argtypes = [vp, vp]
    L.rnamc_bpp_batch.argtypes = [vp, C.c_uint32, vp, vp, C.c_int, C.c_int, vp, vp, vp]
    L.rnamc_bpp_batch_device.argtypes = [vp, C.c_uint32, vp, vp, C.c_int, C.c_int, vp, vp, vp, vp]
    L.rnamc_ctx_last_stats.argtypes = [vp, C.POINTER(BatchStats)]
    L.rnamc_ctx_stats.argtypes = [vp, vp, C.c_uint64, u64p]
    L.rnamc_pool_create.argtypes = [vp, vp, C.c_uint32, C.c_uint64, C.POINTER(vp)]
    L.rnamc_pool_destroy.argtypes = [vp]
    L.rnamc_pool_destroy.restype = None
    L.rnamc_pool_size.argtypes = [vp]
    L.rnamc_pool_size.restype = C.c_uint32
    L.rnamc_pool_ctx.argtypes = [vp, C.c_uint32]
    L.rnamc_pool_ctx.restype = vp
    L.rnamc_pool_set_params.argtypes = [vp, vp]
    L.rnamc_pool_set.argtypes = [vp, C.c_char_p, C.c_int64]
    L.rnamc_bpp_batch_multi.argtypes = [vp, C.c_uint32, vp, vp, C.c_int, C.c_int, vp, vp, vp]
    L.rnamc_shard_plan.argtypes = [C.c_uint32, vp, C.c_uint32, vp]
    L.rnamc_sweep_cost.argtypes = [C.c_uint32, vp, vp]
    L.rnamc_debug_fetch.argtypes = [vp, C.c_uint32, C.c_int, vp]
    L.rnamc_debug_fetch_tree.argtypes = [vp, C.c_uint32, C.c_int, vp, C.c_uint64, u32p, u64p]
    L.rnamc_fold_scores.argtypes = [vp, vp, C.c_uint32, C.c_int, C.c_int, vp, vp, vp, vp,
                                    C.c_uint64, u64p]
    L.rnamc_centroid_fold.argtypes = [vp, C.c_uint32, C.c_float, vp, C.c_uint32, u32p, f32p]
    L.rnamc_fold_sums.argtypes = [vp, vp, C.c_uint32, C.c_int, C.c_int, vp, vp, vp, vp, vp, vp, vp]
    L.rnamc_centroid_fold_multi.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, vp, C.c_uint32, vp, vp]
    L.rnamc_align_scores_new.argtypes = [C.c_float, vp]
    L.rnamc_align_scores_transfer.argtypes = [vp]
    L.rnamc_durbin_batch.argtypes = [vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp, vp, vp, vp]
    L.rnamc_sample_batch.argtypes = [vp, C.c_uint32, vp, vp, C.c_int, C.c_int, C.c_uint32,
                                     C.c_uint64, vp, vp, vp]
    L.rnamc_structure_score.argtypes = [vp, vp, C.c_uint32, C.c_char_p, C.c_int, C.c_int,
                                        C.POINTER(C.c_double)]
    L.rnamc_mfe_batch.argtypes = [vp, C.c_uint32, vp, vp, C.c_int, C.c_int, vp, vp, vp]
    # hard constraints: (constraint strings, max_bp_span) after the offsets
    L.rnamc_bpp_batch_constrained.argtypes = [vp, C.c_uint32, vp, vp, C.c_char_p, C.c_uint32, C.c_int,
                                              C.c_int, vp, vp, vp]
    L.rnamc_bpp_batch_multi_constrained.argtypes = L.rnamc_bpp_batch_constrained.argtypes
    L.rnamc_sample_batch_constrained.argtypes = [vp, C.c_uint32, vp, vp, C.c_char_p, C.c_uint32, C.c_int,
                                                 C.c_int, C.c_uint32, C.c_uint64, vp, vp, vp]
    L.rnamc_mfe_batch_constrained.argtypes = [vp, C.c_uint32, vp, vp, C.c_char_p, C.c_uint32, C.c_int,
                                              C.c_int, vp, vp, vp]
    L.rnamc_log_partition_batch.argtypes = [vp, C.c_uint32, vp, vp, C.c_char_p, C.c_uint32, C.c_int,
                                            C.c_int, vp]
    L.rnamc_constraint_check.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_char_p,
                                         C.POINTER(C.c_int)]
    # (ctx or pool, n_seqs, bases, offsets, constraints, max_bp_span, contra, short hairpins, thresholds,
    # n_thresholds, structs, n_pairs, expect_accuracy, log_partition, bpp, out_offsets)
    L.rnamc_centroid_fold_batch.argtypes = [vp, C.c_uint32, vp, vp, C.c_char_p, C.c_uint32, C.c_int, C.c_int,
                                            vp, C.c_uint32, vp, vp, vp, vp, vp, vp]
    L.rnamc_centroid_fold_batch_multi.argtypes = L.rnamc_centroid_fold_batch.argtypes
    # (ctx or pool, n_seqs, bases, offsets, constraints, max_bp_span, contra, short hairpins, min_prob,
    # pair_start, pair_count, pair_i, pair_j, pair_prob, pairs_cap, pairs_total, paired_prob, log_partition)
    L.rnamc_bpp_batch_sparse.argtypes = [vp, C.c_uint32, vp, vp, C.c_char_p, C.c_uint32, C.c_int, C.c_int,
                                         C.c_float, vp, vp, vp, vp, vp, C.c_uint64, u64p, vp, vp]
    L.rnamc_bpp_batch_sparse_multi.argtypes = L.rnamc_bpp_batch_sparse.argtypes
    # (n, window, stride, max_bp_span, n_windows, band, starts, starts_cap)
    L.rnamc_window_plan.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, u64p, u32p, vp, C.c_uint64]
    # (ctx or pool, bases, n, constraint, window, stride, max_bp_span, contra, short hairpins, band_prob,
    # paired_prob, window_log_partition)
    L.rnamc_bpp_windowed.argtypes = [vp, vp, C.c_uint64, C.c_char_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int,
                                     C.c_int, vp, vp, vp]
    L.rnamc_bpp_windowed_multi.argtypes = L.rnamc_bpp_windowed.argtypes
    # (bases, n, positions, n_positions, n_mutants, mut_pos, mut_base, cap)
    L.rnamc_mutant_plan.argtypes = [vp, C.c_uint32, vp, C.c_uint32, u64p, vp, vp, C.c_uint64]
    # (ctx or pool, bases, n, constraint, max_bp_span, contra, short hairpins, positions, n_positions,
    # log_partition, pair_dist2_q, max_dp, max_i, max_j, paired_prob, wt_log_partition, wt_paired_prob)
    L.rnamc_mutant_scan.argtypes = [vp, vp, C.c_uint32, C.c_char_p, C.c_uint32, C.c_int, C.c_int, vp, C.c_uint32,
                                    vp, vp, vp, vp, vp, vp, vp, vp]
    L.rnamc_mutant_scan_multi.argtypes = L.rnamc_mutant_scan.argtypes
    # (ctx or pool, n_rows, n_cols, rows, max_bp_span, contra, short hairpins, thresholds, n_thresholds, bpp,
    # col_paired, structs, n_pairs, expect_accuracy, log_partition, row_len)
    L.rnamc_bpp_alignment.argtypes = [vp, C.c_uint32, C.c_uint32, vp, C.c_uint32, C.c_int, C.c_int, vp, C.c_uint32,
                                      vp, vp, vp, vp, vp, vp, vp]
    L.rnamc_bpp_alignment_multi.argtypes = L.rnamc_bpp_alignment.argtypes
    # (ctx or pool, n_seqs, bases, offsets, constraints, max_bp_span, contra, short hairpins, profile,
    # log_partition)
    L.rnamc_context_profile_batch.argtypes = [vp, C.c_uint32, vp, vp, C.c_char_p, C.c_uint32, C.c_int, C.c_int,
                                              vp, vp]
    L.rnamc_context_profile_batch_multi.argtypes = L.rnamc_context_profile_batch.argtypes
    L.rnamc_context_profile_stats.argtypes = [vp, u64p, C.POINTER(C.c_double)]
    # (ctx or pool, n_seqs, bases, offsets, n_pairs, pair_a, pair_b, contra, match_probs, out_offsets,
    # bound_a, bound_b, bound_offsets, log_partition, structs, struct_offsets, best_scores)
    L.rnamc_duplex_batch.argtypes = [vp, C.c_uint32, vp, vp, C.c_uint32, vp, vp, C.c_int, vp, vp, vp, vp, vp, vp,
                                     vp, vp, vp]
    L.rnamc_duplex_batch_multi.argtypes = L.rnamc_duplex_batch.argtypes
    # (params, a, n_a, b, n_b, n_chain, chain_i, chain_j, contra, log_weight)
    L.rnamc_duplex_score.argtypes = [vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, vp, vp, C.c_int,
                                     C.POINTER(C.c_double)]
    # (probs, n1, n2, gamma, mate, n_matched, expect_accuracy)
    L.rnamc_match_align.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_float, vp, u32p, f32p]
    # the outputs both alignment entries end on: (min_prob, gammas, n_gammas, match_i, match_j, match_prob, cap,
    # list_start, list_count, list_total, mate, mate_offsets, n_matched, expect_accuracy, matched, matched_offsets)
    match_out = [C.c_float, vp, C.c_uint32, vp, vp, vp, C.c_uint64, vp, vp, u64p, vp, vp, vp, vp, vp, vp]
    # (ctx, n_mats, n1, n2, probs, prob_offsets, ...)
    L.rnamc_match_align_mats.argtypes = [vp, C.c_uint32, vp, vp, vp, vp] + match_out
    # (ctx, scores, n_seqs, bases, offsets, n_pairs, pair_a, pair_b, ..., match_probs, out_offsets)
    L.rnamc_durbin_align_batch.argtypes = [vp, vp, C.c_uint32, vp, vp, C.c_uint32, vp, vp] + match_out + [vp, vp]
    _lib = L
    return L


def check(status):
    if status != OK:
        raise RnamcError(status, lib().rnamc_last_error().decode(errors="replace"))
