"""Every name rnamc_ctx_set accepts in a release build: its default, the summation mode it acts in and
the values the GPU suite sets it to.  tests/test_knob_table_cpu.py holds this table against
rna_algos_amd/csrc/rnamc_ctx.cpp (no name missing), against tests/test_gpu_*.py (every name set
somewhere) and against the knob paragraph of include/rnamc.h (every name documented): a knob added
without a test or without documentation fails the CPU suite.

mode: "reference" (reference-order sweep, rnamc_sweep.cpp: results are the oracle's bits whatever the
knob says), "tree" (tree-order sweep, rnamc_sweep_tree.cpp: the f64 value of the recurrences to f32
rounding), "both" (the batch plan and the mode switch itself), "entry" (a staging size of one entry
point; results do not depend on it).
default None: chosen by the library from the call (named in the comment)."""

DEFAULT_GROUP_MAX_NT = 2 << 20

# name: (default, mode, values the GPU suite exercises)
KNOBS = {
    "summation_mode": (0, "both", (0, 1)),
    "group_max_seqs": (8192, "both", (1, 2, 3, 5, 17, 512, 8192)),
    "group_max_nt": (DEFAULT_GROUP_MAX_NT, "both", (1, 500, 3000, DEFAULT_GROUP_MAX_NT)),
    "group_ws_bytes": (64 << 30, "both", (4, 1 << 21)),
    "profile": (0, "both", (0, 2)),
    # reference-order sweep
    "block_threads": (256, "reference", (64, 128, 192, 256)),
    "order_inside": (0, "reference", (0, 1, 2)),
    "order_outside": (1, "reference", (0, 1, 2, 3, 4)),
    "fuse_inside": (1, "reference", (0, 1)),
    "dual_outside": (1, "reference", (0, 1)),
    "dual_min_cells": (256 * 1024, "reference", (0, 2000, 4096, 256 * 1024)),
    "dual_max_diag": (1 << 30, "reference", (37, 90, 1 << 30)),
    "latency_mode": (1, "reference", (0, 1, 2)),
    "lat_max_cells": (32768, "reference", ("k*n", "k*n - 1", "2*k*n", "2*k*n - 1", 750, 32768)),
    "lat_inside": (2, "reference", (0, 2)),
    "lat_e_waves": (2048, "reference", (0, 64, 200, 2048)),
    "lat_pairs": (1, "reference", (0, 1)),
    "lat_merge": (1, "reference", (0, 1)),
    "lat_split": (0, "reference", (0, 1)),
    "lat_zr_ahead": (1, "reference", (0, 1)),
    # tree-order sweep
    "tree_two": (1, "tree", (0, 1)),
    "tree_tpc": (0, "tree", (0, 64, 128, 256, 1024)),
    "tree_band": (64, "tree", (0, 32, 64)),
    "tree_ahead": (1, "tree", (0, 1)),
    "tree_waves": (5120, "tree", (64, 256, 1024, 5120)),
    "tree_short": (256, "tree", (1, 32, 256)),
    "tree_ahead_waves": (16384, "tree", (0, 300, 16384)),
    "tree_xcd_rows": (0, "tree", (0, 1)),
    "tree_mid_wgs": (None, "tree", (1, 3, 7)),  # default by the longest sequence: 256 / 512 / 1024
    "tree_mid_mx": (1, "tree", (0, 1)),
    "tree_side_stream": (0, "tree", (0, 2)),
    "tree_lane": (1, "tree", (0, 1, 2)),
    "tree_lane_min_nt": (65536, "tree", ("total", "total + 1", 65536)),
    "tree_lane_band": (32, "tree", (32, 64)),
    "tree_mid_sync": (1, "tree", (0, 1)),
    "tree_gen_batch": (3, "tree", (1, 3)),
    "tree_dual": (1, "tree", (0, 1)),
    # staging sizes of single entry points
    "centroid_chunk_bytes": (0, "entry", (0, 4096, 400000)),
    "window_chunk_nt": (64 << 20, "entry", (1, 320, 448, 1000)),
    "mutant_chunk_nt": (64 << 20, "entry", (1, 600)),
}

MODES = ("reference", "tree", "both", "entry")
