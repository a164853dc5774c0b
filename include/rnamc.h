/*
 * rnamc.h — C ABI of librnamc.so: the MI355X-native McCaskill partition-function /
 * base-pairing-probability (bpp) hot path of heartsh/rna-algos.
 *
 * This is the drop-in boundary.  The reference has no FFI of its own; the entry
 * points below are what a Rust `extern "C"` block inside the crate's
 * `src/mccaskill_algo.rs` would bind so that
 *
 *     pub fn mccaskill_algo<T>(seq, uses_contra_model, allows_short_hairpins,
 *                              fold_score_sets) -> (SparseProbMat<T>, FoldScores<T>)
 *     (reference: src/mccaskill_algo.rs:247-280)
 *
 * keeps its signature while its body becomes "pack -> rnamc_bpp_batch -> unpack"
 * (binding shown in INTEGRATION.md).  Plain pointers and sizes only; no C++ or
 * torch types cross this line.  Every function returns an `int` status
 * (RNAMC_OK == 0) and never aborts or throws; the Rust shim turns a non-zero
 * status into `panic!()` to preserve the reference's error behaviour
 * (src/utils.rs:570-572, src/mccaskill_algo.rs:526).
 *
 * Scoring tables are INPUTS.  The reference takes its Turner-2004 and
 * CONTRAfold v2.02 numbers from the third-party crate `rna-ss-params = "0.1"`
 * (Cargo.toml:12, glob-imported at src/utils.rs:8-10), which is not part of the
 * reference tree; `rnamc_params` below holds every table the path reads
 *  with fixed shapes, and is filled from a table file
 * (rnamc_params_load) or from the seeded synthetic generator
 * (rnamc_params_synthetic).
 */
#ifndef RNAMC_H
#define RNAMC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: summation_mode knob (tree-order sums), rnamc_ctx_stats (sized copy), multi-device batch
 *    entry rnamc_bpp_batch_multi; rnamc_params itself is unchanged since 2.  Entries appended
 *    since, without a version change: rnamc_sample_batch, rnamc_structure_score,
 *    rnamc_mfe_batch, rnamc_bpp_batch_constrained, rnamc_bpp_batch_multi_constrained,
 *    rnamc_sample_batch_constrained, rnamc_mfe_batch_constrained, rnamc_log_partition_batch,
 *    rnamc_constraint_check, rnamc_centroid_fold_batch, rnamc_centroid_fold_batch_multi,
 *    rnamc_bpp_batch_sparse, rnamc_bpp_batch_sparse_multi, rnamc_window_plan, rnamc_bpp_windowed,
 *    rnamc_bpp_windowed_multi, rnamc_mutant_plan, rnamc_mutant_scan, rnamc_mutant_scan_multi,
 *    rnamc_bpp_alignment, rnamc_bpp_alignment_multi, rnamc_context_profile_batch,
 *    rnamc_context_profile_batch_multi, rnamc_context_profile_stats, rnamc_duplex_batch,
 *    rnamc_duplex_batch_multi, rnamc_duplex_score, rnamc_match_align, rnamc_match_align_mats,
 *    rnamc_durbin_align_batch */
#define RNAMC_ABI_VERSION 3u

/* Compile-time limits.  In the reference these are constants of rna-ss-params
 * (recalled values): NUM_BASES, MAX_2LOOP_LEN (src/utils.rs:308),
 * MAX_LOOP_LEN (src/mccaskill_algo.rs:32-34,405), MIN_SPAN_HAIRPIN_CLOSE
 * (src/mccaskill_algo.rs:290), MAX_INTERIOR_* (src/mccaskill_algo.rs:35-36,43). */
#define RNAMC_NUM_BASES 4
#define RNAMC_MAX_2LOOP_LEN 30
#define RNAMC_MAX_LOOP_LEN 30
#define RNAMC_MIN_SPAN_HAIRPIN_CLOSE 5
#define RNAMC_MAX_INTERIOR_EXPLICIT 4
#define RNAMC_MAX_INTERIOR_SYMMETRIC 15
#define RNAMC_MAX_INTERIOR_ASYMMETRIC 28
#define RNAMC_MAX_SPECIAL_HAIRPINS 64
#define RNAMC_MAX_SPECIAL_HAIRPIN_LEN 16
/* Longest sequence the reference's callers can pass (T = u16,
 * src/bin/mccaskill_algo.rs:70-90). */
#define RNAMC_MAX_SEQ_LEN 65535u

/* Base codes (bytes2seq, src/utils.rs:562-577). */
#define RNAMC_A 0
#define RNAMC_C 1
#define RNAMC_G 2
#define RNAMC_U 3

/* Status codes. */
#define RNAMC_OK 0
#define RNAMC_ERR_INVALID_ARG 1   /* null pointer, bad size, bad ABI version      */
#define RNAMC_ERR_INVALID_BASE 2  /* byte outside ACGUacgu / code outside 0..3    */
#define RNAMC_ERR_EMPTY_SEQ 3     /* n == 0 (reference panics: mccaskill_algo.rs:526) */
#define RNAMC_ERR_SEQ_TOO_LONG 4  /* n > 65535                                     */
#define RNAMC_ERR_NO_DEVICE 5     /* no HIP device / HIP runtime failure at init   */
#define RNAMC_ERR_OOM 6           /* host or device allocation failed              */
#define RNAMC_ERR_HIP 7           /* a HIP call failed (see rnamc_last_error)      */
#define RNAMC_ERR_IO 8            /* table file could not be read / written        */
#define RNAMC_ERR_FORMAT 9        /* table file has wrong magic / version / size   */

/* ------------------------------------------------------------------------- */
/* The CONTRAfold parameter set: field-for-field mirror of `FoldScoreSets`
 * (reference: src/utils.rs:91-119; constructor/accumulate/transfer at
 * src/mccaskill_algo.rs:24-211).  All f32 (`Score`). */
typedef struct rnamc_fold_score_sets {
  float hairpin_scores_len[RNAMC_MAX_LOOP_LEN + 1];
  float bulge_scores_len[RNAMC_MAX_LOOP_LEN];
  float interior_scores_len[RNAMC_MAX_LOOP_LEN - 1];
  float interior_scores_symmetric[RNAMC_MAX_INTERIOR_SYMMETRIC];
  float interior_scores_asymmetric[RNAMC_MAX_INTERIOR_ASYMMETRIC];
  float stack_scores[4][4][4][4];
  float terminal_mismatch_scores[4][4][4][4];
  float dangling_scores_left[4][4][4];
  float dangling_scores_right[4][4][4];
  float helix_close_scores[4][4];
  float basepair_scores[4][4];
  float interior_scores_explicit[RNAMC_MAX_INTERIOR_EXPLICIT][RNAMC_MAX_INTERIOR_EXPLICIT];
  float bulge_scores_0x1[4];
  float interior_scores_1x1[4][4];
  float multibranch_score_base;
  float multibranch_score_basepair;
  float multibranch_score_unpair;
  float external_score_basepair;
  float external_score_unpair;
  /* cumulative ("at least") forms, filled by rnamc_fold_score_sets_accumulate */
  float hairpin_scores_len_cumulative[RNAMC_MAX_LOOP_LEN + 1];
  float bulge_scores_len_cumulative[RNAMC_MAX_LOOP_LEN];
  float interior_scores_len_cumulative[RNAMC_MAX_LOOP_LEN - 1];
  float interior_scores_symmetric_cumulative[RNAMC_MAX_INTERIOR_SYMMETRIC];
  float interior_scores_asymmetric_cumulative[RNAMC_MAX_INTERIOR_ASYMMETRIC];
} rnamc_fold_score_sets;

/* The Turner-2004 constants the path reads straight from rna-ss-params
 * (call sites: src/utils.rs:166-411, src/mccaskill_algo.rs:364,367,594).
 * Values are scores, i.e. free energies already multiplied by -1/(kT). */
typedef struct rnamc_turner_scores {
  float hairpin_scores_init[RNAMC_MAX_LOOP_LEN + 1];           /* HAIRPIN_SCORES_INIT            */
  float terminal_mismatch_scores_hairpin[4][4][4][4];          /* TERMINAL_MISMATCH_SCORES_HAIRPIN */
  float stack_scores[4][4][4][4];                              /* STACK_SCORES                   */
  float bulge_scores_init[RNAMC_MAX_2LOOP_LEN + 1];            /* BULGE_SCORES_INIT              */
  float interior_scores_init[RNAMC_MAX_2LOOP_LEN + 1];         /* INTERIOR_SCORES_INIT           */
  float interior_scores_1x1[4][4][4][4][4][4];                 /* INTERIOR_SCORES_1X1            */
  float interior_scores_1x2[4][4][4][4][4][4][4];              /* INTERIOR_SCORES_1X2            */
  float interior_scores_2x2[4][4][4][4][4][4][4][4];           /* INTERIOR_SCORES_2X2            */
  float terminal_mismatch_scores_1xmany[4][4][4][4];
  float terminal_mismatch_scores_2x3[4][4][4][4];
  float terminal_mismatch_scores_interior[4][4][4][4];
  float terminal_mismatch_scores_multibranch[4][4][4][4];
  float dangling_scores_5prime[4][4][4];
  float dangling_scores_3prime[4][4][4];
  float helix_augu_end_penalty;
  float coeff_hairpin_len_extrapolation;
  float ninio_coeff;
  float ninio_max;
  float init_multibranch_base;
  float coeff_num_branches;
  /* HAIRPIN_SCORES_SPECIAL: (whole hairpin incl. closing pair, score), compared by
   * slice equality (src/utils.rs:198-205).  bases are codes 0..3. */
  float special_hairpin_scores[RNAMC_MAX_SPECIAL_HAIRPINS];
  uint8_t special_hairpin_seqs[RNAMC_MAX_SPECIAL_HAIRPINS][RNAMC_MAX_SPECIAL_HAIRPIN_LEN];
  uint8_t special_hairpin_lens[RNAMC_MAX_SPECIAL_HAIRPINS];
  uint32_t num_special_hairpins;
  uint32_t min_hairpin_len;                /* MIN_HAIRPIN_LEN                 (recalled: 3)  */
  uint32_t max_hairpin_len_extrapolation;  /* MAX_HAIRPIN_LEN_EXTRAPOLATION   (recalled: 9)  */
  uint32_t min_hairpin_len_extrapolation;  /* MIN_HAIRPIN_LEN_EXTRAPOLATION   (recalled: 10) */
} rnamc_turner_scores;

typedef struct rnamc_params {
  uint32_t abi_version;   /* must be RNAMC_ABI_VERSION                     */
  uint32_t struct_bytes;  /* must be sizeof(rnamc_params)                   */
  uint64_t table_id;      /* provenance tag: synthetic seed, or file hash   */
  rnamc_turner_scores turner;
  rnamc_fold_score_sets contra;
} rnamc_params;

/* ------------------------------------------------------------------------- */
/* Misc. */
uint32_t rnamc_abi_version(void);
size_t rnamc_params_sizeof(void);
const char* rnamc_strerror(int status);
/* Thread-local detail of the last failing call on this thread (HIP error text). */
const char* rnamc_last_error(void);

/* bytes2seq (src/utils.rs:562-577): ASCII ACGUacgu -> codes 0..3; any other byte
 * -> RNAMC_ERR_INVALID_BASE (the reference panics). */
int rnamc_bytes2seq(const uint8_t* ascii, uint64_t n, uint8_t* codes);

/* Number of f32 slots of one sequence's packed bpp triangle: n(n+1)/2. */
uint64_t rnamc_bpp_len(uint32_t n);
/* Index of pair (i,j), i <= j < n, in the packed triangle (diagonal-major:
 * all pairs with j-i = d are contiguous, ordered by i). */
uint64_t rnamc_bpp_index(uint32_t n, uint32_t i, uint32_t j);

/* ------------------------------------------------------------------------- */
/* Parameter plumbing. */

/* FoldScoreSets::new(init_val)  (src/mccaskill_algo.rs:25-58). */
int rnamc_fold_score_sets_new(float init_val, rnamc_fold_score_sets* out);
/* FoldScoreSets::accumulate     (src/mccaskill_algo.rs:60-86). */
int rnamc_fold_score_sets_accumulate(rnamc_fold_score_sets* fss);
/* FoldScoreSets::transfer       (src/mccaskill_algo.rs:88-210): copy the
 * "compiled" CONTRAfold tables of `src` into `dst`, skipping (leaving as they
 * are) the entries whose closing pair -- and for stack_scores also the enclosed
 * pair -- is non-canonical, then accumulate. */
int rnamc_fold_score_sets_transfer(rnamc_fold_score_sets* dst, const rnamc_fold_score_sets* src);

/* Whole parameter block with every f32 set to init_val (header filled in). */
int rnamc_params_new(float init_val, rnamc_params* out);
/* Deterministic synthetic tables for BOTH models (SplitMix64 stream seeded with
 * `seed`, Turner-like magnitudes; contra tables pass through `transfer`). */
int rnamc_params_synthetic(uint64_t seed, rnamc_params* out);
/* Binary table file: 16-byte header {"RNAMCTBL", abi u32, bytes u32} + struct. */
int rnamc_params_save(const rnamc_params* p, const char* path);
int rnamc_params_load(const char* path, rnamc_params* out);
/* Enumerate the f32 array fields of rnamc_params (for host-language mirrors):
 * returns RNAMC_ERR_INVALID_ARG when idx is past the end. */
int rnamc_params_field(uint32_t idx, const char** name, uint64_t* byte_offset, uint64_t* count);
/* The non-float members, for host languages that do not mirror the struct:
 * HAIRPIN_SCORES_SPECIAL (src/utils.rs:198-205): n entries, sequence x as len[x] base codes
 * at seqs[x * RNAMC_MAX_SPECIAL_HAIRPIN_LEN ...]; and the three hairpin length constants
 * (src/utils.rs:174-183). */
int rnamc_params_set_special_hairpins(rnamc_params* p, uint32_t n, const uint8_t* seqs,
                                      const uint8_t* lens, const float* scores);
int rnamc_params_set_hairpin_limits(rnamc_params* p, uint32_t min_hairpin_len,
                                    uint32_t max_hairpin_len_extrapolation,
                                    uint32_t min_hairpin_len_extrapolation);

/* ------------------------------------------------------------------------- */
/* Device context: owns the uploaded tables, a workspace and streams on ONE
 * GPU.  Thread-safe: calls on one ctx are serialised by an internal mutex; use
 * one ctx per host thread (or per GPU) for concurrency. */
typedef struct rnamc_ctx rnamc_ctx;

/* device < 0 selects the current HIP device.  workspace_bytes == 0 sizes the DP
 * workspace lazily from the first batch (grown on demand). */
int rnamc_ctx_create(const rnamc_params* params, int device, uint64_t workspace_bytes,
                     rnamc_ctx** out);
void rnamc_ctx_destroy(rnamc_ctx* ctx);
/* Replace the tables of a live context (waits for the context's earlier work).  The
 * reference reads `&FoldScoreSets` on every call (src/mccaskill_algo.rs:247-280) and the
 * set is trainable (src/utils.rs:91-119): a host mirror that caches a context calls this
 * whenever the contents of the caller's set differ from the ones last uploaded. */
int rnamc_ctx_set_params(rnamc_ctx* ctx, const rnamc_params* params);
/* Knobs; returns RNAMC_ERR_INVALID_ARG for unknown names or values.
 *
 * "summation_mode" selects how every logsumexp sum of the sweep is evaluated:
 *   0 (default) reference order: each fold runs in the reference's k order with its cubic
 *     ln_exp_1p / expf pieces (src/utils.rs:579-655) — bit-identical to the reference CPU path
 *     (the parity gate; north_star's <= 1e-6);
 *   1 tree order: order-free sums (every lane keeps a running max and a sum of exp, merged by
 *     wave and LDS reductions; hardware exp2 / log2), the reference's recurrences with the
 *     cell-independent Theta(n^3) loops turned into prefix recurrences
 *     (rna_algos_amd/csrc/rnamc_tree.hip).  NOT bit-comparable with the reference: the
 *     reference's fold is approximate and order-dependent, so this mode differs from it by the
 *     reference's own error (measured max |dp| 1e-3 at n = 76, 7e-3 ... 2e-2 at n = 4096; ln Z by
 *     3e-2 ... 1e-1 at n = 4096) while agreeing with the exact (f64) value of the same
 *     recurrences to f32 rounding (|dp| < 1e-4 at n = 1024).  Key sets are identical.  About
 *     ten times faster than mode 0 on a lone long sequence.  rnamc_fold_scores and
 *     rnamc_debug_fetch always use mode 0.
 * Tuning (all optional): "group_max_seqs","group_max_nt","group_ws_bytes","block_threads",
 * "fuse_inside","dual_outside","dual_min_cells","dual_max_diag","order_inside","order_outside",
 * "latency_mode","lat_max_cells","lat_inside","lat_e_waves","lat_pairs",
 * "lat_merge","lat_zr_ahead","lat_split" (latency forms of the outside sweep: probs_multibranch and
 * the multibranch half of the pair probabilities as two launches per diagonal, the 2-loop half beside
 * them on the second stream; default 0),"profile"; tree-order mode: "tree_two" (two anti-diagonals per
 * launch, default 1), "tree_tpc" (threads per cell: 64 / 128 / 256 / 1024, 0 = by diagonal size),
 * "tree_band" (width of a band of anti-diagonals whose cubic products take their mid-field from
 * the tiled kernel k_tree_mid one band ahead: 0 / 32 / 64 / 96 / 128, default 64; 0 = every launch
 * walks its sums whole), "tree_mid_wgs" (workgroups of a mid-field launch; default by length: 256 / 512 / 1024),
 * "tree_ahead" (banded sweeps: the far part of a launch's 2-loop blocks is summed by extra
 * workgroups of the previous launch, default 1), "tree_waves" (waves a tree-order launch may hold
 * at once when it picks threads per cell, default 5120), "tree_short" (sums of at most this many
 * terms take one wave per cell, default 256), "tree_ahead_waves" (waves up to which the ahead role
 * takes one wave per cell instead of one per row, default 16384), "tree_xcd_rows" (1: workgroups of a
 * sweep launch of at least 64 workgroups a sequence are dealt so that 32 neighbouring rows share an XCD,
 * grids padded to multiples of 64; default 0; same results), "tree_side_stream" (0: probe
 * whether the side stream runs beside the caller's stream and sweep unbanded if not — the default;
 * 1 / 2: take it as concurrent / serialised without probing), "tree_lane" (lane-per-cell sweeps,
 * rnamc_tree_lane.h: 0 never, 1 for calls of several sequences and at least "tree_lane_min_nt"
 * nucleotides — the default —, 2 always), "tree_mid_sync" (lane-per-cell sweeps: a band's mid-field
 * kernel runs in front of the band on the sweep's own stream, default 1), "tree_lane_band" (the band
 * width of those sweeps: 32 / 64 / 96 / 128, default 32, never wider than "tree_band"), "tree_gen_batch"
 * (diagonals whose generic 2-loop sums share a launch there: 1 .. 3, default 3), "tree_dual" (every other
 * group of such a call on a second stream with its own half of the workspace, so that two groups fill each
 * other's launch gaps: default 1; device-resident entry only), "tree_mid_mx" (the
 * mid-field products on the matrix cores, k_tree_mid_mx: exponentials per operand element, one
 * v_mfma_f32_32x32x2_f32 multiply-add per term; default 1, 0 = the VALU form k_tree_mid).
 * rnamc_centroid_fold_batch: "centroid_chunk_bytes" (bytes of (max,+) matrices one chunk of
 * (record, threshold) items may take; 0 — the default — = the workspace the context holds for the
 * group; never more than that workspace, never less than one item; results do not depend on it).
 * rnamc_bpp_windowed / rnamc_mutant_scan: "window_chunk_nt" / "mutant_chunk_nt" (nucleotides one staged
 * call of theirs takes; described with those entries below).
 * Every knob is per context. */
int rnamc_ctx_set(rnamc_ctx* ctx, const char* name, int64_t value);

/* mccaskill_algo over a batch (src/mccaskill_algo.rs:247-280 for each record, as
 * src/bin/mccaskill_algo.rs:64-93 does on its thread pool).
 *   bases        concatenated base codes 0..3, host memory
 *   offsets      n_seqs+1 prefix offsets into `bases`
 *   bpp          per sequence s the packed triangle of n_s(n_s+1)/2 f32 at
 *                bpp + out_offsets[s]; entry (i,j) at rnamc_bpp_index; a pair
 *                absent from the reference's SparseProbMat holds -1.0f
 *   log_partition  n_seqs f32: sums_external[0][n-1] (may be NULL)
 * The summation order of every logsumexp fold is the reference's unless the context's
 * "summation_mode" knob says otherwise (rnamc_ctx_set). */
int rnamc_bpp_batch(rnamc_ctx* ctx, uint32_t n_seqs, const uint8_t* bases,
                    const uint64_t* offsets, int uses_contra_model, int allows_short_hairpins,
                    float* bpp, const uint64_t* out_offsets, float* log_partition);

/* Same, with `bases`, `bpp`, `log_partition` already resident in device memory
 * of ctx's GPU; `offsets`/`out_offsets` stay host arrays.  Work is enqueued on
 * `hip_stream` (a hipStream_t, may be NULL for the default stream) and the call
 * returns without synchronising. */
int rnamc_bpp_batch_device(rnamc_ctx* ctx, uint32_t n_seqs, const uint8_t* d_bases,
                           const uint64_t* offsets, int uses_contra_model,
                           int allows_short_hairpins, float* d_bpp, const uint64_t* out_offsets,
                           float* d_log_partition, void* hip_stream);

/* ------------------------------------------------------------------------- */
/* The batch over SEVERAL devices: what the reference's binaries do with one pool task per
 * record on all cores (src/bin/mccaskill_algo.rs:58-93, src/bin/centroid_fold.rs:119-132).
 * A pool owns one device context (tables, workspace, streams) per listed device and one host
 * thread per context during a call.  The batch is cut into as many shards as there are
 * contexts — contiguous bands of the cost-sorted batch with equal total cost under the
 * measured sweep model (rnamc_shard_plan) — every shard runs through rnamc_bpp_batch of its
 * own context and writes straight into the caller's host triangles.  Sequences are never
 * split; there is no collective and no device-to-device traffic.
 *   devices / n_devices  HIP device ordinals, one context each (an ordinal may repeat: several
 *                        contexts on one GPU); n_devices == 0 = every visible device
 *   workspace_bytes      per context, as in rnamc_ctx_create */
typedef struct rnamc_pool rnamc_pool;
int rnamc_pool_create(const rnamc_params* params, const int* devices, uint32_t n_devices,
                      uint64_t workspace_bytes, rnamc_pool** out);
void rnamc_pool_destroy(rnamc_pool* pool);
uint32_t rnamc_pool_size(const rnamc_pool* pool);
/* context idx of the pool (owned by the pool), e.g. for rnamc_ctx_stats; NULL past the end */
rnamc_ctx* rnamc_pool_ctx(rnamc_pool* pool, uint32_t idx);
/* rnamc_ctx_set_params / rnamc_ctx_set on every context of the pool */
int rnamc_pool_set_params(rnamc_pool* pool, const rnamc_params* params);
int rnamc_pool_set(rnamc_pool* pool, const char* name, int64_t value);
/* Arguments as rnamc_bpp_batch.  The whole batch is validated first: a bad record fails the
 * call with its status before any device is touched.  A device-side failure of one shard is
 * returned once the other shards have finished (no buffer is left in use). */
int rnamc_bpp_batch_multi(rnamc_pool* pool, uint32_t n_seqs, const uint8_t* bases,
                          const uint64_t* offsets, int uses_contra_model,
                          int allows_short_hairpins, float* bpp, const uint64_t* out_offsets,
                          float* log_partition);
/* The partition rnamc_bpp_batch_multi uses (host only, no device needed): shard_of_seq[s] in
 * 0 .. n_shards-1.  Shard k holds a band of the batch sorted by length (longest first,
 * stable); cuts lie where the running cost a*n(n^2-1)/6 + b*n^2 reaches k/n_shards of the total. */
int rnamc_shard_plan(uint32_t n_seqs, const uint64_t* offsets, uint32_t n_shards,
                     uint32_t* shard_of_seq);
/* The cost model behind the partition, seconds of one reference-order sweep of an n-nt sequence
 * on an MI355X: RNAMC_COST_S_PER_CELL_K * n(n^2-1)/6 (the Theta(n^3) folds) +
 * RNAMC_COST_S_PER_N2 * n^2 (the 496-probe 2-loop blocks); fitted on one box (DESIGN.md section
 * 6).  THE one source of the two constants: rnamc_shard_plan, bench.py's shards and
 * rna_algos_amd.workloads.sweep_cost all evaluate rnamc_sweep_cost. */
#define RNAMC_COST_S_PER_CELL_K 3.25e-12
#define RNAMC_COST_S_PER_N2 6.6e-10
int rnamc_sweep_cost(uint32_t count, const uint64_t* lengths, double* cost_s);

/* Per-kernel accounting of the last batch call on this ctx (launch counts and
 * device time by HIP events on the launch stream; the latter only when
 * profiling was switched on with rnamc_ctx_set(ctx,"profile",1)). */
typedef struct rnamc_batch_stats {
  uint64_t n_groups;
  uint64_t launches_inside;
  uint64_t launches_outside;  /* kernels of the outside sweeps (two per diagonal on large launches) */
  uint64_t launches_other;
  double ms_inside;   /* sum of event-timed inside sweeps  */
  double ms_outside;  /* sum of event-timed outside sweeps */
  double ms_other;
  uint64_t workspace_bytes;
  /* per-kernel accounting of the outside sweep (rnamc_ctx_set(ctx,"profile",2) only; the
   * extra event records cost about 2 % of the sweep): launches and summed
   * durations (HIP events around every launch, on the stream it is launched on) of
   *   main : k_outside<.,5>  probs_multibranch + 2-loop half of the pair probabilities
   *   tail : k_outside<.,2>  multibranch half of the pair probabilities (second stream)
   *   small: k_outside<.,7>  all three roles in one kernel (launches too small to split) */
  uint64_t launches_outside_main, launches_outside_tail, launches_outside_small;
  double ms_outside_main, ms_outside_tail, ms_outside_small;
  /* tree-order mode, banded sweep: does the context's side stream (mid-field products) run BESIDE
   * the caller's stream?  0 not probed (no banded call yet), 1 yes, 2 no — the two share a
   * hardware queue (the process holds too many streams): the sweep then runs unbanded (slower on
   * long sequences, never wrong).  Probed once per context and stream, ~0.2 ms
   * (rnamc_tree.hip, tree_side_stream_probe). */
  uint64_t tree_side_stream;
  /* rnamc_bpp_windowed: the statistics above summed over the call's chunks, and the launches of its
   * own kernels (accumulate, finalise, paired; also counted in launches_other) with, when profiling
   * is on, their summed device time */
  uint64_t launches_window;
  double ms_window;
  /* rnamc_mutant_scan: the statistics above summed over the wild-type fold and the call's chunks, and
   * the launches of its own kernels (compare, paired; also counted in launches_other) with, when
   * profiling is on, their summed device time */
  uint64_t launches_mutant;
  double ms_mutant;
} rnamc_batch_stats;
int rnamc_ctx_last_stats(rnamc_ctx* ctx, rnamc_batch_stats* out);
/* The same with the caller's idea of the struct size: copies min(out_bytes, sizeof) bytes, so a
 * binding compiled against an older (shorter) rnamc_batch_stats is never overrun.  Returns the
 * library's sizeof(rnamc_batch_stats) through *lib_bytes (may be NULL). */
int rnamc_ctx_stats(rnamc_ctx* ctx, void* out, uint64_t out_bytes, uint64_t* lib_bytes);

/* Debug / test hook: copy one DP matrix of sequence `seq_idx` of the LAST group
 * of the last batch call back to the host as a dense n*n row-major f32 matrix
 * (cells outside the stored triangle = NaN).  which: 0 sums_close, 1
 * sums_accessible, 2 sums_external, 3 sums_1ormore_basepairs, 4
 * multibranch_close_scores, 5 probs_multibranch, 6 probs_multibranch2 (both -inf, the reference's
 * "no entry", on the diagonals below the shortest pair span of the call's model: the outside sweep
 * never visits them and the slot holds inside-pass data there). */
int rnamc_debug_fetch(rnamc_ctx* ctx, uint32_t seq_idx, int which, float* out_nxn);
/* The same for the tree-order mode: the raw workspace matrix `slot` (0 .. 37, enum TreeMat of
 * rna_algos_amd/csrc/rnamc_device.h; an internal layout, for tests only) of sequence `seq_idx` as the
 * last call left it, *ld (may be NULL) = its row stride.  With out = NULL only *ld and *floats (may be
 * NULL; the matrix's size) are set.  "row": cell (i, j) at [i * ld + j], "col": [j * ld + i],
 * diagonal-major: [(j - i) * ld + i].  RNAMC_ERR_INVALID_ARG unless the last batch call of the context
 * ran in summation mode 1 and made ONE group, or when out_floats is below the matrix's size. */
int rnamc_debug_fetch_tree(rnamc_ctx* ctx, uint32_t seq_idx, int slot, float* out, uint64_t out_floats,
                           uint32_t* ld, uint64_t* floats);

/* ------------------------------------------------------------------------- */
/* FoldScores<T>, the second element of mccaskill_algo's result
 * (src/mccaskill_algo.rs:14-19): the loop scores the inside pass looked up, keyed like
 * its hash maps.  The key sets depend on the DP (a pair is a key of
 * multibranch_close_scores / accessible_scores iff its sums_close is finite, :333-338 /
 * :457-462; (i,j,k,l) is a key of twoloop_scores iff (k,l) has a sums_close entry, :318-320
 * / :429-431), so the call runs the device sweep for the sequence, reads the sums_close
 * key set back and scores on the host with the functions the kernels use.
 *   hairpin_scores, multibranch_close_scores, accessible_scores: packed triangles of
 *     rnamc_bpp_len(n) floats (rnamc_bpp_index), NaN = key absent; each may be NULL.
 *   twoloop_scores: up to twoloop_cap entries, closing pair (i,j) diagonal-major, then
 *     k ascending, l descending (the reference's visiting order); *twoloop_count gets the
 *     full count.  With twoloop_scores == NULL only the count is produced; a non-NULL
 *     buffer that is too small gives RNAMC_ERR_INVALID_ARG (count still set).
 * The context keeps the key set of the last sequence it swept: the usual pair of calls
 * (count, allocate, fill) on the same sequence and flags runs ONE device sweep. */
typedef struct rnamc_twoloop_score {
  uint32_t i, j, k, l; /* (i,j) closes, (k,l) is enclosed */
  float score;
} rnamc_twoloop_score;
int rnamc_fold_scores(rnamc_ctx* ctx, const uint8_t* bases, uint32_t n, int uses_contra_model,
                      int allows_short_hairpins, float* hairpin_scores,
                      float* multibranch_close_scores, float* accessible_scores,
                      rnamc_twoloop_score* twoloop_scores, uint64_t twoloop_cap,
                      uint64_t* twoloop_count);

/* FoldSums<T> (src/mccaskill_algo.rs:3-11, 213-226): what the reference's first stage,
 * `pub fn get_fold_sums` / `get_fold_sums_contra` (src/mccaskill_algo.rs:282-378 / 380-516),
 * returns.  The inside sweep of ONE sequence on the device, always in reference order, then the
 * seven members as n x n row-major matrices like the reference's Vec<Vec<f32>> (any pointer may
 * be NULL).  Cells the reference never writes hold its initial values: sums_external 0 (lower
 * triangle and spans it skips included), the other dense matrices -inf; the two sparse maps
 * (sums_close, sums_accessible) come dense with -inf for an absent key (the reference inserts
 * finite values only, src/mccaskill_algo.rs:332-338 / 456-462).  Under Turner the reference never
 * writes sums_rightmost_basepairs_multibranch: all -inf.  The second stage (`get_basepair_probs*`)
 * is not offered alone: it reads the caller's FoldScores maps instead of the sequence; the whole
 * path is rnamc_bpp_batch. */
int rnamc_fold_sums(rnamc_ctx* ctx, const uint8_t* bases, uint32_t n, int uses_contra_model,
                    int allows_short_hairpins, float* sums_external,
                    float* sums_rightmost_basepairs_external,
                    float* sums_rightmost_basepairs_multibranch, float* sums_close,
                    float* sums_accessible, float* sums_multibranch,
                    float* sums_1ormore_basepairs);

/* ------------------------------------------------------------------------- */
/* Boltzmann sampling (stochastic traceback of the inside sweep, reference order, whatever the
 * context's "summation_mode" says): n_samples secondary structures per sequence, each drawn with
 * probability exp(score) / Z.  At every cell of the inside grammar the sampler picks one term of
 * the cell's sum with weight exp(term - max) normalised over the terms themselves (DESIGN.md
 * section 9 lists the grammar).  Randomness: Philox4x32-10 with key = seed and counter =
 * (decision index, sample t, batch index s, 0), one uniform u = (word 0 >> 8) * 2^-24 per
 * decision, so a sample is a pure function of the tables, the sequence and flags, seed, s and t
 * (not of grouping, of the other sequences of the batch, of knobs or of the device).
 *   bases, offsets  as rnamc_bpp_batch
 *   structs       per sequence s, n_samples rows of n_s bytes '(' ')' '.', at
 *                 structs + n_samples * (offsets[s] - offsets[0]); row t at + t * n_s
 *   log_weights   n_seqs * n_samples f32, [s * n_samples + t] (may be NULL): the sum of the
 *                 sample's loop scores in f32 (compare rnamc_structure_score)
 *   log_partition n_seqs f32, sums_external[0][n-1] (may be NULL)
 * n_samples == 0 writes nothing and returns RNAMC_OK. */
int rnamc_sample_batch(rnamc_ctx* ctx, uint32_t n_seqs, const uint8_t* bases,
                       const uint64_t* offsets, int uses_contra_model, int allows_short_hairpins,
                       uint32_t n_samples, uint64_t seed, uint8_t* structs, float* log_weights,
                       float* log_partition);

/* Log Boltzmann weight of one structure (host only, no device): the sum of its loop scores in
 * f64; -inf (status OK) for a well-formed structure outside the model's space (a non-canonical
 * pair, a pair of span < 5 unless CONTRAfold with allows_short_hairpins, a CONTRAfold hairpin of
 * more than 30 unpaired bases, a 2-loop of more than 30); RNAMC_ERR_INVALID_ARG for malformed
 * input (dot_bracket not of length n, characters other than "().", unbalanced brackets).
 * exp(log_weight - log Z) is the structure's probability. */
int rnamc_structure_score(const rnamc_params* params, const uint8_t* bases, uint32_t n,
                          const char* dot_bracket, int uses_contra_model,
                          int allows_short_hairpins, double* log_weight);

/* Maximum-score structure of every sequence (MFE under Turner, Viterbi parse under CONTRAfold):
 * the inside recurrences in the (max, +) semiring over the structure space that
 * rnamc_structure_score scores as finite, then an argmax traceback.
 * Ties: at every cell the first maximal candidate in the sampler's candidate order wins.  The
 * result depends only on the tables, the sequence and the two flags (not on grouping, the other
 * sequences of the batch, knobs, summation_mode or the device).
 *   bases, offsets  as rnamc_bpp_batch
 *   structs    n_s bytes '(' ')' '.' per sequence at structs + (offsets[s] - offsets[0])
 *   scores     n_seqs f32: sum of the structure's loop scores (may be NULL)
 *   dp_scores  n_seqs f32: the max-plus sweep's value (may be NULL) */
int rnamc_mfe_batch(rnamc_ctx* ctx, uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
                    int uses_contra_model, int allows_short_hairpins,
                    uint8_t* structs, float* scores, float* dp_scores);

/* ------------------------------------------------------------------------- */
/* Hard constraints: fold over a restricted structure space (RNAfold's -C without
 * --enforceConstraint, and --maxBPspan).  Every entry below takes, after
 * `offsets`,
 *   constraints   NULL = no string constraints; else sequence s's string of n_s bytes at
 *                 constraints + (offsets[s] - offsets[0]) (the layout of `bases`, no terminator)
 *                 over the characters  . x ( ) < >
 *   max_bp_span   0 = no limit; else the longest admitted span j - i + 1 of a pair (i, j)
 *                 (span as in RNAMC_MIN_SPAN_HAIRPIN_CLOSE)
 * Every rule REMOVES pairs; none forces a base to pair.  A pair (i, j), i < j, may form only if
 * the model allows it (canonical; span >= RNAMC_MIN_SPAN_HAIRPIN_CLOSE unless CONTRAfold with
 * allows_short_hairpins) and
 *   - neither i nor j is 'x';
 *   - if i or j is an end of a matched constraint pair (a, b) ('(' at a, ')' at b), (i, j) = (a, b);
 *   - (i, j) crosses no constraint pair (a, b): neither i < a < j < b nor a < i < b < j;
 *   - '<' at p: p pairs only downstream (p = i); '>' at p: p pairs only upstream (p = j);
 *   - max_bp_span L > 0: j - i + 1 <= L.
 * A constraint pair whose bases cannot pair (non-canonical, or span too short) still forbids the
 * pairs that cross it, and its two bases stay unpaired.  Enforced pairs and '|' are not offered.
 * RNAMC_ERR_INVALID_ARG, before any device work, for an unbalanced bracket or a byte outside the
 * set ('|' and a terminating NUL of a string shorter than its sequence included); the record and
 * position are in rnamc_last_error().  A NULL or all-'.' string with max_bp_span 0 or >= n is the
 * unconstrained problem: results bit-identical to the plain entries, which are these entries with
 * constraints = NULL, max_bp_span = 0.  A forbidden pair is absent from every output (bpp -1). */

/* rnamc_bpp_batch / rnamc_bpp_batch_multi over the constrained space (both summation modes);
 * exp(log_partition) is Z_c, and p(i, j) the pair probability given the constraint. */
int rnamc_bpp_batch_constrained(rnamc_ctx* ctx, uint32_t n_seqs, const uint8_t* bases,
                                const uint64_t* offsets, const char* constraints,
                                uint32_t max_bp_span, int uses_contra_model,
                                int allows_short_hairpins, float* bpp, const uint64_t* out_offsets,
                                float* log_partition);
int rnamc_bpp_batch_multi_constrained(rnamc_pool* pool, uint32_t n_seqs, const uint8_t* bases,
                                      const uint64_t* offsets, const char* constraints,
                                      uint32_t max_bp_span, int uses_contra_model,
                                      int allows_short_hairpins, float* bpp,
                                      const uint64_t* out_offsets, float* log_partition);
/* rnamc_sample_batch / rnamc_mfe_batch over the constrained space (same outputs; a sample is a pure
 * function of the tables, the sequence, its constraint, the flags, seed, s and t). */
int rnamc_sample_batch_constrained(rnamc_ctx* ctx, uint32_t n_seqs, const uint8_t* bases,
                                   const uint64_t* offsets, const char* constraints,
                                   uint32_t max_bp_span, int uses_contra_model,
                                   int allows_short_hairpins, uint32_t n_samples, uint64_t seed,
                                   uint8_t* structs, float* log_weights, float* log_partition);
int rnamc_mfe_batch_constrained(rnamc_ctx* ctx, uint32_t n_seqs, const uint8_t* bases,
                                const uint64_t* offsets, const char* constraints,
                                uint32_t max_bp_span, int uses_contra_model,
                                int allows_short_hairpins, uint8_t* structs, float* scores,
                                float* dp_scores);
/* ln Z (constrained or not) of every sequence: the reference-order inside sweep alone, whatever
 * summation_mode says (no outside sweep).  Equal bit for bit to rnamc_bpp_batch's log_partition in
 * summation_mode 0.  P(constraint) = exp(ln Z_c - ln Z); with 'x' over a region, the probability
 * that every base of it is unpaired (its accessibility).
 *   log_partition  n_seqs f32 */
int rnamc_log_partition_batch(rnamc_ctx* ctx, uint32_t n_seqs, const uint8_t* bases,
                              const uint64_t* offsets, const char* constraints,
                              uint32_t max_bp_span, int uses_contra_model,
                              int allows_short_hairpins, float* log_partition);
/* Host only: validate a constraint (a NUL-terminated string of length n; RNAMC_ERR_INVALID_ARG as
 * above, or when its length is not n) and, if dot_bracket (NUL-terminated, length n, "()." and
 * balanced; RNAMC_ERR_INVALID_ARG otherwise) is not NULL, set *compatible to 1 when every pair of
 * that structure satisfies the constraint's rules and the span limit, else 0.  The model's own
 * rules (canonical pairs, minimum span) are not part of the check. */
int rnamc_constraint_check(const char* constraint, uint32_t n, uint32_t max_bp_span,
                           const char* dot_bracket, int* compatible);

/* ------------------------------------------------------------------------- */
/* Consumers of the path's output, host side. */

/* centroid_fold (src/centroid_fold.rs:25-105) driven off a packed bpp triangle
 * as produced above.  pairs_out receives up to max_pairs (i,j) pairs in the
 * reference's push order; *n_pairs the count; *expect_accuracy the score. */
int rnamc_centroid_fold(const float* bpp_packed, uint32_t n, float centroid_threshold,
                        uint32_t* pairs_out, uint32_t max_pairs, uint32_t* n_pairs,
                        float* expect_accuracy);

/* The same fold for SEVERAL thresholds at once, the Theta(n^3) fill on ctx's GPU (the reference
 * runs it for 18 gammas per record, src/bin/centroid_fold.rs:147-161): one anti-diagonal sweep of
 * (max,+) reductions for all thresholds off one copy of the bpp triangle, then the traceback of
 * every threshold on host threads.  (max,+) is order-free in f32, so the matrices, and with them
 * pairs, push order and expect_accuracy, are bit-identical to rnamc_centroid_fold's.
 *   pairs_out        n_thresholds blocks of max_pairs (i,j) pairs (may be NULL)
 *   n_pairs          n_thresholds counts;  expect_accuracy  n_thresholds scores (may be NULL) */
int rnamc_centroid_fold_multi(rnamc_ctx* ctx, const float* bpp_packed, uint32_t n,
                              const float* centroid_thresholds, uint32_t n_thresholds,
                              uint32_t* pairs_out, uint32_t max_pairs, uint32_t* n_pairs,
                              float* expect_accuracy);

/* mccaskill_algo + centroid_fold for every record and every threshold (what the reference's
 * centroid_fold binary does, src/bin/centroid_fold.rs:119-161); the bpp triangles never leave the
 * device unless `bpp` is given.  The bpp come from the context's summation mode.  Per lock-step
 * group the (max,+) fill of every (record, threshold) and its traceback run on the device off the
 * group's triangles.
 *   bases, offsets, constraints, max_bp_span, flags   as rnamc_bpp_batch_constrained
 *   centroid_thresholds / n_thresholds               1 .. 65535 gammas, shared by all records
 *   structs          per sequence s, n_thresholds rows of n_s bytes '(' ')' '.', at
 *                    structs + n_thresholds * (offsets[s] - offsets[0]); row g at + g * n_s
 *                    (the layout of rnamc_sample_batch with thresholds in place of samples)
 *   n_pairs          n_seqs * n_thresholds u32, [s * n_thresholds + g]   (may be NULL)
 *   expect_accuracy  n_seqs * n_thresholds f32, same indexing            (may be NULL)
 *   log_partition    n_seqs f32                                          (may be NULL)
 *   bpp, out_offsets as rnamc_bpp_batch; both NULL = do not return the triangles
 * For each (s, g) the row, the count and expect_accuracy are exactly what rnamc_centroid_fold
 * returns for the triangle this same call produced: the dot-bracket string of its pairs, their
 * number, the same f32 bits.  The PUSH ORDER of the pairs is not part of this entry (the
 * reference's binary only ever prints the string, src/bin/centroid_fold.rs:197-207).  Results do
 * not depend on grouping, on the other records of the batch or on "centroid_chunk_bytes".
 * RNAMC_ERR_INVALID_ARG for n_thresholds == 0, for bpp without out_offsets or the reverse, for a
 * NULL ctx / pool; bad records and bad constraints fail before any device work. */
int rnamc_centroid_fold_batch(rnamc_ctx* ctx, uint32_t n_seqs, const uint8_t* bases,
                              const uint64_t* offsets, const char* constraints,
                              uint32_t max_bp_span, int uses_contra_model,
                              int allows_short_hairpins, const float* centroid_thresholds,
                              uint32_t n_thresholds, uint8_t* structs, uint32_t* n_pairs,
                              float* expect_accuracy, float* log_partition, float* bpp,
                              const uint64_t* out_offsets);
/* The same over the pool's devices: the shards of rnamc_bpp_batch_multi_constrained
 * (rnamc_shard_plan), each through its own context, written straight into the caller's arrays. */
int rnamc_centroid_fold_batch_multi(rnamc_pool* pool, uint32_t n_seqs, const uint8_t* bases,
                                    const uint64_t* offsets, const char* constraints,
                                    uint32_t max_bp_span, int uses_contra_model,
                                    int allows_short_hairpins, const float* centroid_thresholds,
                                    uint32_t n_thresholds, uint8_t* structs, uint32_t* n_pairs,
                                    float* expect_accuracy, float* log_partition, float* bpp,
                                    const uint64_t* out_offsets);

/* ------------------------------------------------------------------------- */
/* Durbin pair-HMM nucleotide match probabilities (SURVEY.md 8f-4;
 * reference: src/durbin_algo.rs:73-242, constants src/compiled_align_scores.rs). */

/* AlignScores (src/durbin_algo.rs:4-14).  The model they parameterise is stated in
 * tests/durbin_ref.py; insert_switch_score is a field that no term reads.
 * The domain of the scores:
 *   -inf is the way to forbid something.  The reference's logsumexp skips a term that is not
 *   finite, so a match_scores entry at -inf gives exactly 0.0 at every cell with those two bases
 *   and leaves the other cells the probabilities of the model without those matches.
 *   Very negative FINITE scores are outside the domain.  The reference's logsumexp is
 *   min + (max - min) in f32 once its two terms are more than 11.86 apart; a score far below about
 *   -1e7 makes that difference so large that adding it back to min no longer returns max (with
 *   -1e30 the sum comes out as 0), and the results are "probabilities" above 1, here as in the
 *   reference.
 *   If the scores forbid every alignment (all insert_scores at -inf and sequences of unequal
 *   lengths, for one), the total weight is 0 and every interior cell is NaN (0 / 0). */
typedef struct rnamc_align_scores {
  float match2match_score;
  float match2insert_score;
  float insert_extend_score;
  float insert_switch_score;
  float init_match_score;
  float init_insert_score;
  float insert_scores[RNAMC_NUM_BASES];
  float match_scores[RNAMC_NUM_BASES][RNAMC_NUM_BASES];
} rnamc_align_scores;

/* AlignScores::new(init_val) (src/durbin_algo.rs:26-40). */
int rnamc_align_scores_new(float init_val, rnamc_align_scores* out);
/* AlignScores::transfer (src/durbin_algo.rs:42-57): the compiled CONTRAlign constants of
 * src/compiled_align_scores.rs:2-19 (they are part of the reference tree, unlike the
 * McCaskill tables). */
int rnamc_align_scores_transfer(rnamc_align_scores* scores);

/* durbin_algo (src/durbin_algo.rs:73-77) over a batch of sequence pairs, as
 * src/bin/durbin_algo.rs:55-75 runs one pool task per pair.
 *   bases     concatenated codes of ALL sequences, each carrying PSEUDO_BASE (= 4,
 *             src/utils.rs:122) at both ends as the reference's callers build them
 *             (src/bin/durbin_algo.rs:49-51); real bases are codes 0..3
 *   offsets   n_seqs+1 prefix offsets into `bases` (every sequence has length >= 2)
 *   pair_a/b  n_pairs indices into the sequences: pair p aligns pair_a[p] with pair_b[p]
 *   match_probs  per pair p a dense row-major ProbMat of len(a) x len(b) f32 at
 *             match_probs + out_offsets[p] (border rows / columns are 0, as in the reference)
 * Each pair's forward and backward sweeps run by anti-diagonal on the GPU; every logsumexp
 * fold is the reference's, in its order. */
int rnamc_durbin_batch(rnamc_ctx* ctx, const rnamc_align_scores* scores, uint32_t n_seqs,
                       const uint8_t* bases, const uint64_t* offsets, uint32_t n_pairs,
                       const uint32_t* pair_a, const uint32_t* pair_b, float* match_probs,
                       const uint64_t* out_offsets);

/* ------------------------------------------------------------------------- */
/* Pairwise alignment off match-probability matrices: thresholded sparse
 * match probabilities, per-base marginals and gamma-centroid (maximum expected accuracy)
 * alignments, all made on the device while the matrices are there.
 *
 * The estimator, with the scoring convention of centroid_fold (src/centroid_fold.rs:49-50), for a
 * ProbMat P of n1 x n2 (border rows and columns: the pseudo bases), L1 = n1 - 2, L2 = n2 - 2:
 *     M[0][j] = M[i][0] = +0
 *     M[i][j] = max(M[i-1][j], M[i][j-1], (M[i-1][j-1] + gamma * P[i][j]) - 1)    1 <= i <= L1, 1 <= j <= L2
 * in f32; the match candidate is one rounded multiply, one rounded add and one rounded subtract, in
 * that order, never fused.  The traceback starts at (L1, L2) and runs while i > 0 and j > 0, with
 * exact float equality in this order: M[i][j] == M[i-1][j] -> i--; else M[i][j] == M[i][j-1] ->
 * j--; else the match (i, j) is recorded and i--, j--.
 *   mate             n1 values: mate[i] = the column matched with row i, or -1 (both border rows: -1)
 *   n_matched        the number of matches;  expect_accuracy  M[L1][L2] (may be NULL)
 * Host only, no device: the definition the two entries below reproduce bit for bit. */
int rnamc_match_align(const float* probs, uint32_t n1, uint32_t n2, float gamma, int* mate,
                      uint32_t* n_matched, float* expect_accuracy);

/* The stage over the caller's dense matrices (callers that transform the probabilities first: a
 * consistency transformation, an average).  Matrix m is n1[m] x n2[m] f32, row-major, at
 * probs + prob_offsets[m]; n1[m], n2[m] >= 2.
 *   min_prob      finite and >= 0.  An interior cell (i, j), 1 <= i <= L1, 1 <= j <= L2, is LISTED when
 *                 p > 0 and p >= min_prob (f32 comparisons); i and j are matrix coordinates.
 *   gammas / n_gammas   0 .. 64 finite gammas shared by all matrices; 0: lists and marginals only
 *   match_i, match_j, match_prob   parallel arrays of `cap` entries; all three or none (none: the call
 *                 only counts).  Matrix m's list is entries list_start[m] .. + list_count[m] - 1, in
 *                 row-major order (i ascending, then j ascending), match_prob with the bits of the dense
 *                 cell.  Lists of different matrices never overlap; where a list sits is unspecified.
 *   list_start, list_count   n_mats u64 (required with the three arrays; list_count may be given alone)
 *   list_total    never NULL: the number of listed cells of all matrices.  A capacity too small gives
 *                 RNAMC_ERR_INVALID_ARG with list_count and *list_total set (call again with room).
 *   mate          per matrix n_gammas rows of n1[m] values at mate + mate_offsets[m], row g at + g * n1[m]
 *   n_matched, expect_accuracy   n_mats * n_gammas values, [m * n_gammas + g]
 *   matched       per matrix n1[m] + n2[m] f32 at matched + matched_offsets[m]: row_matched[i] = the sum
 *                 of P[i][j] over j = 1 .. L2 ascending, one rounded f32 add each from +0, then
 *                 col_matched[j] likewise over i (the probability that a base is aligned to anything;
 *                 borders 0, not clamped)
 * Every output pointer may be NULL except list_total.  For each (m, g) mate, n_matched and
 * expect_accuracy are exactly what rnamc_match_align returns.  Matrices run in chunks within
 * "group_ws_bytes" (at most 65535 a chunk); results do not depend on the chunks or on the other
 * matrices.  Bad arguments fail before any device work. */
int rnamc_match_align_mats(rnamc_ctx* ctx, uint32_t n_mats, const uint32_t* n1, const uint32_t* n2,
                           const float* probs, const uint64_t* prob_offsets, float min_prob,
                           const float* gammas, uint32_t n_gammas, uint32_t* match_i,
                           uint32_t* match_j, float* match_prob, uint64_t cap,
                           uint64_t* list_start, uint64_t* list_count, uint64_t* list_total,
                           int* mate, const uint64_t* mate_offsets, uint32_t* n_matched,
                           float* expect_accuracy, float* matched,
                           const uint64_t* matched_offsets);

/* rnamc_durbin_batch followed by that stage off each chunk's device-resident ProbMats: what the
 * callers of the reference's durbin_algo binary keep of all pairs of a FASTA.  Inputs as
 * rnamc_durbin_batch, outputs as rnamc_match_align_mats with pair p in place of matrix m
 * (n1 = len(a), n2 = len(b), pseudo bases included).
 *   match_probs, out_offsets   the dense ProbMats as rnamc_durbin_batch returns them (the same bits);
 *                 both NULL = no dense matrix is copied to the host.  Both or neither.
 * Pairs run in chunks whose pair-HMM matrices, and then the stage's in their place, fit
 * "group_ws_bytes" (at most 65535 pairs a chunk). */
int rnamc_durbin_align_batch(rnamc_ctx* ctx, const rnamc_align_scores* scores, uint32_t n_seqs,
                             const uint8_t* bases, const uint64_t* offsets, uint32_t n_pairs,
                             const uint32_t* pair_a, const uint32_t* pair_b, float min_prob,
                             const float* gammas, uint32_t n_gammas, uint32_t* match_i,
                             uint32_t* match_j, float* match_prob, uint64_t cap,
                             uint64_t* list_start, uint64_t* list_count, uint64_t* list_total,
                             int* mate, const uint64_t* mate_offsets, uint32_t* n_matched,
                             float* expect_accuracy, float* matched,
                             const uint64_t* matched_offsets, float* match_probs,
                             const uint64_t* out_offsets);

/* ------------------------------------------------------------------------- */
/* Thresholded sparse pair probabilities (the reference's SparseProbMat, src/utils.rs), compacted
 * on the device: the triangles never reach the host.
 *   bases, offsets, constraints, max_bp_span, flags   as rnamc_bpp_batch_constrained
 *   min_prob      finite and >= 0.  A pair (i, j), i < j, of record s is LISTED when it is present in
 *                 the record's triangle (p > -0.5) and p >= min_prob (an f32 comparison).  0 lists
 *                 exactly the keys of the reference's SparseProbMat; values above 1 are legal.
 *   pair_i, pair_j, pair_prob   three parallel arrays of pairs_cap entries: all given, or all NULL
 *   pair_start, pair_count      n_seqs u64 each: record s's pairs are entries
 *                 [pair_start[s], pair_start[s] + pair_count[s]) of the three arrays, in packed-
 *                 triangle order (span ascending, then i ascending).  Lists of different records
 *                 never overlap; where a record's list sits is unspecified and may differ between
 *                 calls (it follows group and shard order).
 *   pairs_total   Sum of pair_count (never NULL)
 *   paired_prob   laid out like `constraints`: n_s f32 at paired_prob + (offsets[s] - offsets[0])
 *                 (may be NULL).  For base x the probability that x is paired, summed over ALL present
 *                 pairs whatever min_prob is, in this order: start from +0; for d = 1 .. n-1
 *                 ascending add p(x, x+d) if x + d < n and the pair is present, then p(x-d, x) if
 *                 x >= d and the pair is present; one rounded f32 add each.  Not clamped.
 *   log_partition n_seqs f32 (may be NULL)
 * The probabilities come from the context's summation mode exactly as rnamc_bpp_batch_constrained
 * produces them: every pair_prob has the bits of the dense triangle's cell.  Results do not depend
 * on grouping, on the other records of the batch, on knobs or on the device.
 * With the three arrays NULL the call only counts: pair_count (may then be NULL), *pairs_total,
 * paired_prob and log_partition are produced, pair_start is untouched.  With arrays and
 * pairs_cap < total: RNAMC_ERR_INVALID_ARG, pair_count and *pairs_total set, the arrays' contents
 * unspecified (the rnamc_fold_scores idiom: call again with the total).  RNAMC_ERR_INVALID_ARG also
 * for a NULL ctx / pool, a min_prob that is NaN, infinite or negative, only some of the three
 * arrays, arrays without pair_start / pair_count; bad records and bad constraints fail before any
 * device work. */
int rnamc_bpp_batch_sparse(rnamc_ctx* ctx, uint32_t n_seqs, const uint8_t* bases,
                           const uint64_t* offsets, const char* constraints, uint32_t max_bp_span,
                           int uses_contra_model, int allows_short_hairpins, float min_prob,
                           uint64_t* pair_start, uint64_t* pair_count, uint32_t* pair_i,
                           uint32_t* pair_j, float* pair_prob, uint64_t pairs_cap,
                           uint64_t* pairs_total, float* paired_prob, float* log_partition);
/* The same over the pool's devices: the shards of rnamc_bpp_batch_multi_constrained
 * (rnamc_shard_plan), each through its own context; every group of every shard claims its part of
 * the three arrays from one shared cursor, so nothing is gathered afterwards. */
int rnamc_bpp_batch_sparse_multi(rnamc_pool* pool, uint32_t n_seqs, const uint8_t* bases,
                                 const uint64_t* offsets, const char* constraints,
                                 uint32_t max_bp_span, int uses_contra_model,
                                 int allows_short_hairpins, float min_prob, uint64_t* pair_start,
                                 uint64_t* pair_count, uint32_t* pair_i, uint32_t* pair_j,
                                 float* pair_prob, uint64_t pairs_cap, uint64_t* pairs_total,
                                 float* paired_prob, float* log_partition);

/* ------------------------------------------------------------------------- */
/* Structural context profiles (CapR's profile): for every base u of every record six probabilities
 * over the Boltzmann ensemble of the model's structure space (what rnamc_structure_score scores as
 * finite, minus the pairs that constraints remove), computed on the device off the matrices of the
 * inside-outside sweep.  Rows, in CapR's order:
 *   0 bulge        u unpaired in a 2-loop with exactly one empty side
 *   1 exterior     u unpaired and enclosed by no pair
 *   2 hairpin      u unpaired, the innermost enclosing pair closes a hairpin
 *   3 internal     u unpaired in a 2-loop with both sides non-empty
 *   4 multibranch  u unpaired, the innermost enclosing pair closes a loop with >= 2 branches
 *   5 stem         u paired: rnamc_bpp_batch_sparse's paired_prob, bit for bit
 *   bases, offsets, constraints, max_bp_span, flags   as rnamc_bpp_batch_constrained
 *   profile       record s at profile + 6 * (offsets[s] - offsets[0]): six rows of n_s f32 (never NULL)
 *   log_partition n_seqs f32 (may be NULL)
 * The sweep always runs in the reference's summation order, whatever "summation_mode" says.  Rows 0,
 * 2, 3 and 4 are sums of 64-bit integers of 2^-44 (every loop's probability rounded once), so every
 * output bit is independent of grouping, the other records of the batch, knobs, devices and runs;
 * the six rows sum to 1 up to the f32 logsumexp arithmetic of the sweep (a few 1e-4).  No triangle
 * reaches the host.  RNAMC_ERR_INVALID_ARG for a NULL ctx / pool or a NULL profile; bad records and
 * bad constraints fail before any device work. */
int rnamc_context_profile_batch(rnamc_ctx* ctx, uint32_t n_seqs, const uint8_t* bases,
                                const uint64_t* offsets, const char* constraints, uint32_t max_bp_span,
                                int uses_contra_model, int allows_short_hairpins, float* profile,
                                float* log_partition);
/* The same over the pool's devices: the shards of rnamc_shard_plan, each through its own context,
 * written straight into the caller's arrays. */
int rnamc_context_profile_batch_multi(rnamc_pool* pool, uint32_t n_seqs, const uint8_t* bases,
                                      const uint64_t* offsets, const char* constraints,
                                      uint32_t max_bp_span, int uses_contra_model,
                                      int allows_short_hairpins, float* profile, float* log_partition);
/* Statistics of the context's last rnamc_context_profile_batch, beside rnamc_ctx_stats (whose block
 * keeps its size): the launches of the entry's own kernels (the copy of sums_multibranch between the
 * two sweeps, the profile kernels, the paired kernel; also counted in launches_other) and, when
 * profiling is on, the summed device time of those behind the sweep in milliseconds (0 otherwise).
 * Both 0 when the context's last call was another entry. */
int rnamc_context_profile_stats(rnamc_ctx* ctx, uint64_t* launches_context, double* ms_context);

/* ------------------------------------------------------------------------- */
/* Windowed local folding of ONE long sequence (what RNAplfold and LocalFold compute): every window
 * of `window` bases is folded with a pair-span limit, and each pair (i, j) gets the AVERAGE of its
 * probability over all windows that contain it.  The windows' triangles never reach the host; the
 * sequence may be longer than a record.
 *   bases, n      the sequence, base codes 0..3, 1 <= n < 2^31
 *   window        W, 1 .. 65535;  stride  S >= 1;  max_bp_span  0 = no limit
 *   Windows: n <= W: one window [0, n).  Otherwise the starts 0, S, 2S, ... while start + W <= n,
 *   and, if the last of these ends before n, one more window at n - W.  S > W is legal: bases that
 *   no window covers have no pairs.
 *   Band: B = min(W, n, max_bp_span if non-zero).  Every window is folded with max_bp_span = B
 *   exactly as rnamc_bpp_batch_constrained folds it (the context's summation mode).
 *   constraint    NULL or n bytes over ". x < >" only: window x gets bytes [start_x, start_x + w).
 *                 '(' ')' (brackets cannot be cut at window edges) or any other byte:
 *                 RNAMC_ERR_INVALID_ARG before any device work, the position in rnamc_last_error().
 *   band_prob     n * B f32, row-major: [i * B + d] for pair (i, i + d), 0 <= d < B
 *   paired_prob   n f32 (may be NULL)
 *   window_log_partition  n_windows f32, ln Z of every window in window order (may be NULL)
 * Accumulation is exact and order-free.  Every present cell (p > -0.5, d >= 1) of a window's triangle
 * contributes the integer q = min(rint((double)p * 2^44), 2^45) (to nearest, ties to even) to a signed
 * 64-bit sum of band cell (start + i, d), and 1 to the cell's 32-bit counter of windows in which the
 * pair was present.  Integer adds commute, and at most 65535 windows contain a cell: the sum stays
 * below 2^62.  Then, with denom(i, d) = the number of windows with start <= i and i + d < start + w,
 *   band_prob[i * B + d] = (float)((double)sum / ((double)denom * 2^44))    (int64 -> double to nearest)
 * where the counter is non-zero, and -1.0f elsewhere (d = 0, i + d >= n, never present, denom = 0).
 * The price of order-freedom is the quantum 2^-44 (5.7e-14) per window: a single-window call equals
 * the plain bpp exactly only where p >= 2^-20, and within 2^-45 absolute below that.
 * paired_prob[x], from the finished band in rnamc_bpp_batch_sparse's order: start from +0; for
 * d = 1 .. B-1 ascending add band(x, d) if present, then band(x - d, d) if x >= d and present; one
 * rounded f32 add each, not clamped.
 * Results do not depend on grouping, on the group knobs, on "window_chunk_nt" or on the number of
 * devices (in summation mode 1 the sweep picks its form per staged call, "tree_lane_min_nt", as it
 * does for rnamc_bpp_batch_constrained on the same records: there the chunk is part of the input).
 * Knob "window_chunk_nt" (rnamc_ctx_set): nucleotides of windows that go through one staged call of
 * the sweep, default 64 Mi, never less than one window: the window list is materialised chunk by
 * chunk, so host and staging memory stay bounded whatever n is.
 * RNAMC_ERR_INVALID_ARG for a NULL ctx / pool / bases / band_prob, window == 0, stride == 0,
 * window > 65535, n >= 2^31; RNAMC_ERR_EMPTY_SEQ for n == 0; RNAMC_ERR_INVALID_BASE as elsewhere;
 * all before any device work.  RNAMC_ERR_OOM when the accumulators (12 bytes per band cell) or the
 * band do not fit the device. */

/* Host only, no device: the window list and band width of a call.  *n_windows (never NULL) and
 * *band (may be NULL) are always set; starts (may be NULL) receives the n_windows window starts,
 * RNAMC_ERR_INVALID_ARG when starts_cap is too small (the count still set). */
int rnamc_window_plan(uint64_t n, uint32_t window, uint32_t stride, uint32_t max_bp_span,
                      uint64_t* n_windows, uint32_t* band, uint64_t* starts, uint64_t starts_cap);
int rnamc_bpp_windowed(rnamc_ctx* ctx, const uint8_t* bases, uint64_t n, const char* constraint,
                       uint32_t window, uint32_t stride, uint32_t max_bp_span, int uses_contra_model,
                       int allows_short_hairpins, float* band_prob, float* paired_prob,
                       float* window_log_partition);
/* The same over the pool's devices: the window list is cut into shards (rnamc_shard_plan), each
 * context accumulates its shard, the shards' integer sums and counters are added on the host, and
 * the pool's first context finalises: bit-identical to the single-context entry. */
int rnamc_bpp_windowed_multi(rnamc_pool* pool, const uint8_t* bases, uint64_t n, const char* constraint,
                             uint32_t window, uint32_t stride, uint32_t max_bp_span,
                             int uses_contra_model, int allows_short_hairpins, float* band_prob,
                             float* paired_prob, float* window_log_partition);

/* ------------------------------------------------------------------------- */
/* Point-mutation scan of ONE sequence (the riboSNitch / SNPfold / RNAsnp / RNAmute question): every
 * single-base mutant of the listed positions is folded and its pair-probability matrix compared
 * with the wild type's on the device.  No triangle reaches the host.
 *   bases, n      the wild type, base codes 0..3, 1 <= n <= 65535
 *   constraint    NULL or the wild type's n bytes over ". x ( ) < >": every record of the call has
 *                 the same length, so brackets are legal; each mutant is folded under the same string
 *   max_bp_span, flags   as rnamc_bpp_batch_constrained
 *   positions     NULL: every base 0 .. n-1 (n_positions is then ignored).  Otherwise n_positions
 *                 entries, each < n, taken as given: any order, duplicates legal (each gives its three
 *                 mutants again).
 * Mutant list: the idx-th listed position x contributes three mutants, base codes b in
 * {0,1,2,3} \ {bases[x]} ascending.  Mutant m = 3 * idx + rank, M = 3 * (number of positions).
 * Folds: the wild type as a call of one record; the mutants in chunks of records (knob
 * "mutant_chunk_nt", rnamc_ctx_set: nucleotides of mutants that go through one staged call of the
 * sweep, default 64 Mi, never less than one mutant).  Every fold runs exactly as
 * rnamc_bpp_batch_constrained folds those records with the same constraint and max_bp_span, in the
 * context's summation mode.  In mode 0 nothing depends on chunking, grouping, knobs or the number of
 * devices; in mode 1 the sweep picks its form per staged call ("tree_lane_min_nt"), as it does for
 * rnamc_bpp_batch_constrained on the same records: there the chunk is part of the input.
 * Per mutant m, against the wild type's triangle.  Both are diagonal-major packed triangles of the
 * same n: packed cell c of one is cell c of the other (rnamc_bpp_index).  Cells of span 0 (c < n)
 * are skipped.  wt[c] / mut[c]: the f32 cells, absent pairs at -1.
 *   log_partition[m]   ln Z of the mutant (never NULL)
 *   pair_dist2_q[m]    the squared Euclidean distance of the two pair-probability matrices in fixed
 *                 point, exact and order-free.  Per cell a = wt[c] > -0.5 ? (double)wt[c] : 0.0, b
 *                 likewise from mut[c]; e = a - b (one f64 subtraction);
 *                 q = min(rint(e * e * 2^44), 2^45): one correctly rounded f64 multiply e * e, fused
 *                 with nothing, an exact scaling by 2^44, rint to nearest with ties to even.  The
 *                 output is the signed 64-bit sum of q over the cells; the distance is
 *                 pair_dist2_q / 2^44.  No overflow: (a - b)^2 <= a + b for a, b in [0, 1], and each
 *                 base's pair probabilities sum to at most about 1, so the sum over the cells of
 *                 (a - b)^2 <= sum a + sum b <= n <= 65535 < 2^16: the integer sum stays below
 *                 2^61 (and a cell that rounding pushed above 1 is capped at 2^45).
 *   max_dp[m], max_i[m], max_j[m]   the pair that moved most.  Per cell t = |fa - fb| with
 *                 fa = wt[c] > -0.5 ? wt[c] : 0.0f, fb likewise (one f32 subtraction).  Only cells
 *                 with t > 0 take part; the largest t wins, ties go to the smallest packed index c;
 *                 (max_i, max_j) is that cell's pair, i < j.  No cell takes part: max_dp = 0 and
 *                 max_i = max_j = 0xffffffff.
 *   paired_prob   M rows of n f32 (may be NULL): row m is the mutant's per-base paired probability
 *                 as rnamc_bpp_batch_sparse defines paired_prob, in its summation order, bit for bit
 *   wt_log_partition   one f32, wt_paired_prob   n f32: the same two quantities of the wild type
 * Every output pointer except log_partition may be NULL.
 * Errors, all before any device work: RNAMC_ERR_INVALID_ARG for a NULL ctx / pool / bases /
 * log_partition, a position >= n, 3 * n_positions >= 2^32, a bad constraint (its position in
 * rnamc_last_error()); RNAMC_ERR_EMPTY_SEQ, RNAMC_ERR_SEQ_TOO_LONG, RNAMC_ERR_INVALID_BASE as
 * elsewhere.  n_positions == 0 with a non-NULL list writes only the wild-type outputs and returns
 * RNAMC_OK.  RNAMC_ERR_OOM when the wild type's triangle (n(n+1)/2 floats, kept for the whole call)
 * or the per-mutant buffers (16 bytes per mutant, and n floats per mutant of a chunk with
 * paired_prob) do not fit the device. */

/* Host only, no device: the mutant list of a call.  *n_mutants (never NULL) is always set to M;
 * mut_pos and mut_base (each may be NULL) receive position and base code of every mutant,
 * RNAMC_ERR_INVALID_ARG when one is given and cap < M (the count still set, nothing written).  The
 * argument checks of rnamc_mutant_scan on bases, n, positions and n_positions apply. */
int rnamc_mutant_plan(const uint8_t* bases, uint32_t n, const uint32_t* positions, uint32_t n_positions,
                      uint64_t* n_mutants, uint32_t* mut_pos, uint8_t* mut_base, uint64_t cap);
int rnamc_mutant_scan(rnamc_ctx* ctx, const uint8_t* bases, uint32_t n, const char* constraint,
                      uint32_t max_bp_span, int uses_contra_model, int allows_short_hairpins,
                      const uint32_t* positions, uint32_t n_positions, float* log_partition,
                      int64_t* pair_dist2_q, float* max_dp, uint32_t* max_i, uint32_t* max_j,
                      float* paired_prob, float* wt_log_partition, float* wt_paired_prob);
/* The same over the pool's devices: the mutant list is cut into contiguous shards
 * (rnamc_shard_plan: equal records, equal bands); every context folds the wild type itself and
 * scans its shard straight into the caller's arrays.  Nothing is summed across devices:
 * bit-identical to the single-context entry in summation mode 0. */
int rnamc_mutant_scan_multi(rnamc_pool* pool, const uint8_t* bases, uint32_t n, const char* constraint,
                            uint32_t max_bp_span, int uses_contra_model, int allows_short_hairpins,
                            const uint32_t* positions, uint32_t n_positions, float* log_partition,
                            int64_t* pair_dist2_q, float* max_dp, uint32_t* max_i, uint32_t* max_j,
                            float* paired_prob, float* wt_log_partition, float* wt_paired_prob);

/* ------------------------------------------------------------------------- */
/* Alignment folding (what CentroidAlifold, PETfold and RNAalifold -p start from): every row of a
 * multiple alignment is folded without its gaps, its pair probabilities are mapped onto alignment
 * COLUMNS and averaged over the rows, and the consensus structure is the gamma-centroid fold of the
 * averaged matrix.  The rows' triangles never reach the host.
 *   rows          n_rows rows of n_cols bytes, row-major: code 0..3 a base, 4 a gap (PSEUDO_BASE,
 *                 src/utils.rs:122: what align_char2base makes of every character outside ACGUacgu);
 *                 1 <= n_rows <= 65535, 1 <= n_cols <= 65535
 *   Records: row s without its gaps is record s, of n_s bases; map_s[k] is the column of its k-th
 *   base.  Every record is folded exactly as rnamc_bpp_batch_constrained folds this list of records
 *   with no constraint strings and the same max_bp_span (counted in the row's own bases, 0 = none),
 *   flags and summation mode.
 *   Accumulation is exact and order-free (the rule of rnamc_bpp_windowed).  Every present cell
 *   (p > -0.5, i < j) of record s contributes the integer q = min(rint((double)p * 2^44), 2^45) (to
 *   nearest, ties to even) to a signed 64-bit sum of column pair (map_s[i], map_s[j]), and 1 to that
 *   cell's 32-bit counter of rows in which the pair was present.  Integer adds commute, and at most
 *   65535 rows keep the sum below 2^61: no output bit depends on the order of rows, groups, streams
 *   or devices.
 *   bpp           one packed diagonal-major triangle of n_cols (n_cols + 1) / 2 f32, cell (ci, cj) at
 *                 rnamc_bpp_index(n_cols, ci, cj) (may be NULL):
 *                   avg = (float)((double)sum / ((double)n_rows * 2^44))   (int64 -> double to nearest)
 *                 where the counter is non-zero, -1.0f elsewhere and on the main diagonal.  The
 *                 denominator is the number of ROWS: a row with a gap in either column contributes
 *                 zero, as in the tools named above.
 *   col_paired    n_cols f32 (may be NULL): for column c the sum over the finished triangle in
 *                 rnamc_bpp_batch_sparse's order: start from +0; for d = 1 .. n_cols-1 ascending add
 *                 avg(c, c+d) if c + d < n_cols and the cell is present, then avg(c-d, c) if c >= d
 *                 and the cell is present; one rounded f32 add each, not clamped.
 *   centroid_thresholds / n_thresholds   0 .. 65535 gammas (0: no consensus folds)
 *   structs       n_thresholds rows of n_cols bytes '(' ')' '.', row g at structs + g * n_cols
 *   n_pairs, expect_accuracy   n_thresholds entries each
 *                 For each g the row, the count and expect_accuracy are exactly what rnamc_centroid_fold
 *                 returns for the averaged triangle this same call produced (whether or not `bpp` is
 *                 given); the push order of the pairs is not part of this entry.
 *   log_partition n_rows f32: ln Z of every record;  row_len  n_rows u32: n_s
 * Every output pointer may be NULL, except that structs, n_pairs or expect_accuracy with
 * n_thresholds == 0 is RNAMC_ERR_INVALID_ARG.  Also RNAMC_ERR_INVALID_ARG: a NULL ctx / pool / rows,
 * n_rows or n_cols 0 or above 65535, thresholds counted but not given.  RNAMC_ERR_INVALID_BASE for a
 * code above 4, RNAMC_ERR_EMPTY_SEQ for a row with no base (the row is named in rnamc_last_error()).
 * All of these before any device work.  RNAMC_ERR_OOM when the accumulators and the result (16 bytes
 * per column-pair cell) do not fit the device.  Results do not depend on grouping, on the group
 * knobs or on the number of devices. */
int rnamc_bpp_alignment(rnamc_ctx* ctx, uint32_t n_rows, uint32_t n_cols, const uint8_t* rows,
                        uint32_t max_bp_span, int uses_contra_model, int allows_short_hairpins,
                        const float* centroid_thresholds, uint32_t n_thresholds, float* bpp,
                        float* col_paired, uint8_t* structs, uint32_t* n_pairs, float* expect_accuracy,
                        float* log_partition, uint32_t* row_len);
/* The same over the pool's devices: the rows are cut into shards (rnamc_shard_plan over their
 * ungapped lengths), each context accumulates its shard, the shards' integer sums and counters are
 * added on the host, and the pool's first context averages and folds: bit-identical to the
 * single-context entry. */
int rnamc_bpp_alignment_multi(rnamc_pool* pool, uint32_t n_rows, uint32_t n_cols, const uint8_t* rows,
                              uint32_t max_bp_span, int uses_contra_model, int allows_short_hairpins,
                              const float* centroid_thresholds, uint32_t n_thresholds, float* bpp,
                              float* col_paired, uint8_t* structs, uint32_t* n_pairs,
                              float* expect_accuracy, float* log_partition, uint32_t* row_len);

/* ------------------------------------------------------------------------- */
/* RNA-RNA duplex folding (the RNAduplex / RNAhybrid / RNAplex question: where a short RNA binds a
 * long one, and how strongly): partition function, pair probabilities and best duplex of two
 * strands, for a batch of strand PAIRS on the device.
 *
 * The model.  Strands A (nA bases) and B (nB bases), both 5'->3', base codes 0..3.  A duplex is a
 * non-empty chain of intermolecular pairs (i_1, j_1), ..., (i_m, j_m), i in A, j in B, with
 * i_1 < i_2 < ... < i_m and j_1 > j_2 > ... > j_m, every pair canonical, and for consecutive pairs
 * a = i_{x+1} - i_x - 1, b = j_x - j_{x+1} - 1 with a + b <= RNAMC_MAX_2LOOP_LEN.  No intramolecular
 * pairs.  With S = A || B (B's index j at nA + j) and R = B || A, the log weight of a duplex is
 *   outer end   accessible(S, nA + nB, i_1, nA + j_1): reads A[i_1 - 1] and B[j_1 + 1] where they
 *               exist; under CONTRAfold it includes basepair_scores of the first pair
 *   + one 2-loop score twoloop(S, i_x, nA + j_x, i_{x+1}, nA + j_{x+1}) per consecutive pair (the
 *               scores of the folding entries: they read only bases between the two pairs)
 *   + inner end, at the pair next to the strand break: Turner accessible(R, nA + nB, j_m, nB + i_m);
 *               CONTRAfold the junction score of that call alone (helix_close and the two dangles),
 *               i.e. the same minus that pair's basepair_scores, which the chain has counted already.
 *               Reads B[j_m - 1] and A[i_m + 1] where they exist.
 * No constant initiation term is added (a caller adds their own to ln Z and to scores);
 * allows_short_hairpins, constraints and span limits do not apply.
 *   inside     F(i,j) = lse(inner_end(i,j), lse over k > i, l < j, a + b <= 30 of twoloop(i,j,k,l) + F(k,l)),
 *              -inf where (A[i], B[j]) is not canonical
 *   ln Z       lse over i, j of outer_end(i,j) + F(i,j)
 *   outside    G(k,l) = lse(outer_end(k,l), lse over i < k, j > l, a + b <= 30 of G(i,j) + twoloop(i,j,k,l))
 *   P(i,j)     exp(F + G - ln Z);   pa[i] = sum_j P(i,j);   pb[j] = sum_i P(i,j)
 *   best       the same F under (max, +), then an argmax traceback: the start pair is the smallest i,
 *              then the smallest j, among the maxima of outer_end + F; at a cell the inner end is tried
 *              first, then (a ascending, b ascending), and the first maximal candidate wins
 * The sums are order-free sums with the maximum taken out: loop scores are f32, every term's
 * exponential is one hardware exp2 of its f32 distance to the running maximum, the closing logarithm
 * one hardware log2; the log-domain values F, G and ln Z themselves are carried in f64 (a long helix
 * reaches hundreds of nats, where an f32 ulp per cell would reach the probabilities).  The order
 * per cell is FIXED, (a, b) ascending; ln Z is a fixed-shape reduction and pa / pb are sequential
 * sums in f64 rounded once, so every output bit depends on the tables, the two strands and the
 * model alone: not on the other pairs of the batch, their order, the chunking ("group_ws_bytes"),
 * the direction the sweep steps in, or the number of devices.  The max-plus sweep is f32.
 *
 *   bases, offsets   n_seqs plain records (no pseudo bases), as rnamc_bpp_batch
 *   pair_a / pair_b  n_pairs indices into the records: pair p folds A = pair_a[p] with B = pair_b[p]
 *   match_probs      per pair nA x nB f32, row-major, at match_probs + out_offsets[p]
 *   bound_a/bound_b  pa (nA f32) at bound_a + bound_offsets[p], pb (nB f32) at bound_b +
 *                    bound_offsets[p] + nA: ONE prefix array of nA + nB entries per pair for both
 *   log_partition    n_pairs f32
 *   structs          nA + nB bytes per pair at structs + struct_offsets[p]: A's bases '(' or '.', then
 *                    B's bases ')' or '.'
 *   best_scores      n_pairs f32: the max-plus value
 * Every output may be NULL and is then neither computed nor copied (a target scan passes
 * match_probs = NULL: no nA x nB matrix leaves the device; with structs and best_scores both NULL
 * the max-plus sweep is skipped).  match_probs needs out_offsets, bound_a / bound_b need
 * bound_offsets, structs needs struct_offsets.
 * A pair of strands without a canonical intermolecular pair: ln Z = -inf, probabilities 0, an
 * all-dots structure, best score -inf, status RNAMC_OK.
 * F and G (nA x nB f64 each) and the max-plus F (nA x nB f32) live in the context's workspace, each
 * only when an output needs it; pairs are chunked so that a chunk fits "group_ws_bytes"; a single
 * pair that cannot fit fails with RNAMC_ERR_OOM (and a message in rnamc_last_error) before anything
 * is launched.
 * RNAMC_ERR_INVALID_ARG for a NULL ctx / pool / offsets / pair list, a pair index >= n_seqs, an
 * output without its offsets; RNAMC_ERR_EMPTY_SEQ / RNAMC_ERR_INVALID_BASE / RNAMC_ERR_SEQ_TOO_LONG
 * for a bad record; all before any device work.  n_pairs == 0 is RNAMC_OK. */
int rnamc_duplex_batch(rnamc_ctx* ctx, uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
                       uint32_t n_pairs, const uint32_t* pair_a, const uint32_t* pair_b,
                       int uses_contra_model, float* match_probs, const uint64_t* out_offsets,
                       float* bound_a, float* bound_b, const uint64_t* bound_offsets,
                       float* log_partition, uint8_t* structs, const uint64_t* struct_offsets,
                       float* best_scores);
/* The same over the pool's devices: the pair list is cut into contiguous bands of equal total
 * nA * nB, every context gets the records its band names and writes straight into the caller's
 * arrays: bit-identical to the single-context entry. */
int rnamc_duplex_batch_multi(rnamc_pool* pool, uint32_t n_seqs, const uint8_t* bases,
                             const uint64_t* offsets, uint32_t n_pairs, const uint32_t* pair_a,
                             const uint32_t* pair_b, int uses_contra_model, float* match_probs,
                             const uint64_t* out_offsets, float* bound_a, float* bound_b,
                             const uint64_t* bound_offsets, float* log_partition, uint8_t* structs,
                             const uint64_t* struct_offsets, float* best_scores);
/* Log weight of ONE duplex (host only, no device): the sum of the three parts above in f64 over the
 * f32 loop scores (the CONTRAfold inner end as accessible(R, ...) minus basepair_scores, both in
 * f64).  chain_i / chain_j: the n_chain pairs, outer end first.  -inf (status OK) for a well-formed
 * chain outside the model (a non-canonical pair, a + b > 30); RNAMC_ERR_INVALID_ARG for an empty or
 * non-monotone chain or an index out of range; RNAMC_ERR_EMPTY_SEQ / RNAMC_ERR_INVALID_BASE for a
 * bad strand. */
int rnamc_duplex_score(const rnamc_params* params, const uint8_t* a, uint32_t n_a, const uint8_t* b,
                       uint32_t n_b, uint32_t n_chain, const uint32_t* chain_i, const uint32_t* chain_j,
                       int uses_contra_model, double* log_weight);

#ifdef __cplusplus
}
#endif
#endif /* RNAMC_H */
