// rnamc_device.h — host<->kernel contract of librnamc.so (internal).
#ifndef RNAMC_DEVICE_H
#define RNAMC_DEVICE_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "rnamc_internal.h"

namespace rnamc {

// One lock-step group of sequences as the kernels see it (passed by value).
struct DeviceBatch {
  const SeqDesc* seqs;      // descriptors of this group, longest sequence first
  const uint8_t* bases;     // base codes of the whole batch
  float* workspace;         // DP matrices
  float* out;               // packed bpp triangles of the whole batch
  float* log_partition;     // may be null
  const rnamc_params* params;
  const float* hp_init;     // Turner hairpin initiation by loop length (host-built)
  int allows_short_hairpins;
  int order_inside, order_outside;  // order in which a launch's role blocks are dispatched
  // hard constraints (rnamc_scoring.h, pair_allowed): two words per base, laid out like `bases`;
  // null = unconstrained.  max_span: the longest admitted pair span j - i + 1 where cons is set.
  const int32_t* cons;
  uint32_t max_span;
};

void launch_init(const DeviceBatch& b, uint32_t nseq, uint32_t max_n, hipStream_t st);
// folds of diagonal d (do_sums) and closing-pair block of diagonal d+1 (do_pair)
void launch_inside(const DeviceBatch& b, bool contra, uint32_t d, uint32_t max_n, uint32_t nseq,
                   uint32_t block, bool do_sums, bool do_pair, hipStream_t st);
// Two-diagonal schedule: folds of diagonals d and d+1 (pair blocks of d and d+1 done; for
// CONTRAfold also launch_inside_zr2 of the same d) beside the early part of the pair
// blocks of d+2 and d+3 (do_head)
void launch_inside2(const DeviceBatch& b, bool contra, uint32_t d, uint32_t max_n, uint32_t nseq,
                    uint32_t block, bool do_sums, bool do_head, hipStream_t st);
// CONTRAfold: sums_rightmost_basepairs_{external,multibranch} of diagonals d and d+1
void launch_inside_zr2(const DeviceBatch& b, uint32_t d, uint32_t max_n, uint32_t nseq,
                       uint32_t block, hipStream_t st);
// last (multibranch) term of the parked pair blocks of diagonals d0 .. d0+nd-1
void launch_pair_tail(const DeviceBatch& b, bool contra, uint32_t d0, uint32_t nd, uint32_t max_n,
                      uint32_t nseq, uint32_t block, hipStream_t st);
// roles: 7 = all three roles in one kernel; 5 = probs_multibranch + pair head; 2 = pair tail;
// 4 = pair head alone
void launch_outside(const DeviceBatch& b, bool contra, uint32_t d, uint32_t max_n, uint32_t nseq,
                    uint32_t block, bool do_mb, bool do_tail, bool do_head, int roles,
                    hipStream_t st);
// Latency forms for groups too small to fill the chip (rnamc_latency.h): one wave per fold
// chain.  A group that uses them uses them on EVERY diagonal (they keep W dense, and complete
// sums_1ormore_basepairs of diagonal d-1 in the launch of diagonal d).
// pair_d != 0: the closing-pair blocks of diagonal pair_d in the same launch; head: the 2-loop
// half of the pair probabilities of diagonal d - 1 in the same launch
void launch_inside_lat(const DeviceBatch& b, bool contra, uint32_t d, uint32_t max_n, uint32_t nseq,
                       int form, bool do_combine, uint32_t pair_d, hipStream_t st);
void launch_outside_lat(const DeviceBatch& b, bool contra, uint32_t d, uint32_t max_n, uint32_t nseq,
                        bool do_mb, bool do_tail, bool head, hipStream_t st);
// closing-pair block (inside) / 2-loop half of the pair probabilities (outside) of diagonal d
void launch_pair_lat(const DeviceBatch& b, bool contra, bool outside, uint32_t d, uint32_t max_n,
                     uint32_t nseq, hipStream_t st);
// Durbin pair-HMM (src/durbin_algo.rs:79-242): one pair of sequences
struct DurbinPair {
  uint32_t n1, n2;   // lengths including the two pseudo bases
  uint64_t a_off, b_off;  // offsets of the two sequences in the bases buffer
  uint64_t ws_off;   // float offset of this pair's six n1 x n2 matrices in the workspace
  uint64_t out_off;  // float offset of this pair's ProbMat in the output
};
void launch_durbin(const DurbinPair* d_pairs, uint32_t n_pairs, uint32_t max_cells,
                   const uint8_t* d_bases, float* ws, float* d_out, const rnamc_align_scores& sc,
                   hipStream_t st);
void launch_finalize(const DeviceBatch& b, uint32_t nseq, uint32_t max_n, uint32_t dmin_out,
                     hipStream_t st);

// Boltzmann sampling (rnamc_sample.hip): one wave per (sequence, sample) of a group whose
// reference-order inside sweep is in the workspace
struct SampleBatch {
  const SeqDesc* seqs;      // descriptors of this group
  const uint8_t* bases;     // base codes of the whole batch
  const float* workspace;   // DP matrices
  const rnamc_params* params;
  const float* hp_init;
  const uint64_t* row_off;  // per descriptor: byte offset of its n_samples rows of n bytes in `rows`
  uint8_t* rows;            // '(' ')' '.'
  float* log_weights;       // [descriptor * n_samples + sample]
  uint64_t* stack;          // n_waves slices of stack_cap pending cells
  uint32_t stack_cap, nseq, n_samples;
  uint64_t seed;
  float* dp_scores;         // maximum-score traceback: [descriptor] sums_external[0][n-1] (may be null)
};
// n_waves a multiple of 4 (256-thread blocks)
void launch_sample(const SampleBatch& a, bool contra, uint32_t n_waves, hipStream_t st);

// Maximum-score (MFE / Viterbi) structure (rnamc_mfe.hip).  The max-plus inside sweep writes the
// matrices the walker reads (rnamc_walk.h) into the group's workspace, k_init's initial values
// serving as they are: one launch per diagonal d holds the sums of diagonal d (d_sums < max_n) and
// the closing-pair cells of diagonal d_pair (< max_n), either may be absent.  Needs launch_init.
void launch_mfe_inside(const DeviceBatch& b, bool contra, uint32_t d_sums, uint32_t d_pair,
                       uint32_t max_n, uint32_t nseq, hipStream_t st);
// argmax traceback of a group whose max-plus sweep is in the workspace: one wave per sequence
// (a.n_samples = 1; a.log_weights receives the structure's score, a.dp_scores the sweep's value)
void launch_mfe_trace(const SampleBatch& a, bool contra, uint32_t n_waves, hipStream_t st);

// gamma-centroid fold (rnamc_centroid.hip): per threshold g two dense n x n matrices of msz
// floats at m + g * 2 * msz (row-major, then column-major), row stride ld, zero-initialised
struct CentroidBatch {
  const float* bpp;     // packed diagonal-major triangle, absent pairs negative (device)
  float* m;
  const float* gammas;  // device
  uint32_t n, ld;
  uint64_t msz;
};
void launch_centroid(const CentroidBatch& a, uint32_t d, uint32_t n_gammas, hipStream_t st);

// gamma-centroid folds of a batch (rnamc_centroid_batch.hip).  An item is one (sequence, threshold)
// pair; its (max,+) matrix is ONE packed diagonal-major triangle laid out like the bpp triangle
// (cell (i, j) at d*n - d(d-1)/2 + i, d = j - i; the main diagonal holds zeros), so the cells of a
// diagonal on consecutive rows read consecutive floats for both factors of every bifurcation.
struct CentroidItem {
  uint64_t m_off;    // float offset of the item's triangle in `m` (mpad floats, see centroid_item_floats)
  uint64_t bpp_off;  // float offset of its sequence's bpp triangle in `bpp`
  uint64_t row_off;  // byte offset of its n bytes '(' ')' '.' in `rows`
  uint32_t n;
  float gamma;
};
struct CentroidChunk {
  const CentroidItem* items;  // device; longest sequence first (items with n > d are a prefix)
  const float* bpp;           // the group's packed triangles, absent pairs negative
  float* m;
  uint8_t* rows;
  uint32_t* n_pairs;          // [item]; 0xffffffff = the traceback's stack overflowed (nothing written)
  float* expect_accuracy;     // [item] M(0, n-1)
  uint64_t* stack;            // n_waves slices of stack_cap pending intervals
  uint32_t n_items, stack_cap;
};
inline uint64_t centroid_item_floats(uint32_t n) {
  return ((static_cast<uint64_t>(n) * (n + 1ull) / 2ull) + 63ull) & ~63ull;
}
// out[x] = the largest entry of sequence x's bpp triangle (seqs[x].bpp_off, seqs[x].n; -1 when no pair is present)
void launch_centroid_pmax(const CentroidItem* seqs, const float* bpp, float* out, uint32_t nseq, hipStream_t st);
// zeros on the main diagonal of every item's triangle
void launch_centroid_batch_init(const CentroidChunk& a, uint32_t max_n, hipStream_t st);
// diagonal d (1 <= d < max_n) of the first n_active items (those with n > d; at most 65535)
void launch_centroid_batch(const CentroidChunk& a, uint32_t d, uint32_t n_active, uint32_t max_n,
                           hipStream_t st);
// traceback of every item: one wave per item; n_waves a multiple of 4 (256-thread blocks)
void launch_centroid_trace(const CentroidChunk& a, uint32_t n_waves, hipStream_t st);

// thresholded sparse pair probabilities of a group (rnamc_sparse.hip).  A
// record's packed triangle is cut into blocks of 256 consecutive cells; a cell is listed when it is
// present (p > -0.5) and p >= min_prob.
struct SparseItem {
  uint64_t bpp_off;   // float offset of the record's bpp triangle in `bpp`
  uint64_t blk_off;   // offset of its n_blocks block counts / bases in `blocks`
  uint64_t out_off;   // offset of its list in the group's staged i / j / p arrays (fill)
  uint64_t pp_off;    // offset of its n paired probabilities in the group's staged array
  uint32_t n;
  uint32_t n_blocks;  // ceil(n(n+1)/2 / 256)
};
// at most 65535 items a launch; max_blocks / max_n: the largest of the launch's items
void launch_sparse_count(const SparseItem* items, uint32_t n_items, uint32_t max_blocks, const float* bpp,
                         uint32_t* blocks, float min_prob, hipStream_t st);
// block counts -> exclusive block bases in place; totals[x] = listed cells of item x (any number of items)
void launch_sparse_scan(const SparseItem* items, uint32_t n_items, uint32_t* blocks, uint32_t* totals,
                        hipStream_t st);
void launch_sparse_fill(const SparseItem* items, uint32_t n_items, uint32_t max_blocks, const float* bpp,
                        const uint32_t* blocks, float min_prob, uint32_t* out_i, uint32_t* out_j, float* out_p,
                        hipStream_t st);
void launch_sparse_paired(const SparseItem* items, uint32_t n_items, uint32_t max_n, const float* bpp,
                          float* paired, hipStream_t st);

// pairwise alignment off device-resident match-probability matrices (rnamc_match.hip, DESIGN.md
// section 20).  A matrix is a dense row-major n1 x n2 ProbMat (border rows / columns: the pseudo
// bases); L1 = n1 - 2, L2 = n2 - 2.  Its part of the workspace holds, in this order, the block
// counts of the compaction, the spilled diagonals of the fill (where L1 + 1 > kMatchDiagLds) and the
// direction bytes of every gamma.
constexpr uint32_t kMatchDiagLds = 1024u;  // cells of a live diagonal that stay in LDS
struct MatchMat {
  uint64_t p_off;      // float offset of the matrix in `probs`
  uint64_t blk_off;    // u32 offset of its n_blocks block counts / bases in the workspace
  uint64_t spill_off;  // float offset of its n_gammas * 3 * (L1 + 1) spilled diagonal cells
  uint64_t dir_off;    // byte offset of its n_gammas * match_dir_bytes(n1, n2) direction bytes
  uint64_t out_off;    // offset of its list in the chunk's staged i / j / p arrays (fill)
  uint64_t mate_off;   // i32 offset of its n_gammas rows of n1 mates in the chunk's staged array
  uint64_t marg_off;   // float offset of its n1 + n2 marginals in the chunk's staged array
  uint32_t n1, n2;
  uint32_t n_blocks;   // ceil(n1 * n2 / 256)
  uint32_t pad;
};
// direction bytes of one (matrix, gamma): row s = i + j of L1 + 1 bytes, for s = 0 .. L1 + L2
__host__ __device__ inline uint64_t match_dir_bytes(uint32_t n1, uint32_t n2) {
  const uint64_t l1 = n1 - 2u, l2 = n2 - 2u;
  return l1 && l2 ? (l1 + l2 + 1u) * (l1 + 1u) : 0u;
}
// at most 65535 matrices a launch (count, fill, marginals); max_blocks / max_side: the largest of
// the launch's matrices
void launch_match_count(const MatchMat* mats, uint32_t n_mats, uint32_t max_blocks, const float* probs,
                        uint32_t* blocks, float min_prob, hipStream_t st);
void launch_match_scan(const MatchMat* mats, uint32_t n_mats, uint32_t* blocks, uint32_t* totals, hipStream_t st);
void launch_match_list(const MatchMat* mats, uint32_t n_mats, uint32_t max_blocks, const float* probs,
                       const uint32_t* blocks, float min_prob, uint32_t* out_i, uint32_t* out_j, float* out_p,
                       hipStream_t st);
void launch_match_marginals(const MatchMat* mats, uint32_t n_mats, uint32_t max_side, const float* probs,
                            float* matched, hipStream_t st);
// fill and traceback of every (matrix, gamma): one workgroup per item, item = matrix * n_gammas + g
// (any number of items); n_matched and accuracy are indexed by item
void launch_match_align(const MatchMat* mats, uint32_t n_mats, const float* probs, const float* gammas,
                        uint32_t n_gammas, float* ws, int32_t* mate, uint32_t* n_matched, float* accuracy,
                        hipStream_t st);

// windowed local folding (rnamc_window.hip): the triangles of a group of
// windows, all of length w, summed as integers into the band accumulators of the whole sequence
struct WindowItem {
  uint64_t bpp_off;  // float offset of the window's bpp triangle in `bpp`
  uint64_t start;    // its first base in the sequence
};
// the call's window list: n_grid windows at 0, stride, 2 stride, ..., and with has_last one more
// at n - w (off the grid); sum and cnt hold [d * n + i], the band [i * band + d]
struct WindowGeom {
  uint64_t n, n_grid;
  uint32_t w, stride, band, has_last;
};
// at most 65535 items a launch
void launch_window_accumulate(const WindowItem* items, uint32_t n_items, const float* bpp, uint32_t w, uint32_t band,
                              uint64_t n_total, int64_t* sum, uint32_t* cnt, hipStream_t st);
void launch_window_finalize(const WindowGeom& g, const int64_t* sum, const uint32_t* cnt, float* band_out,
                            hipStream_t st);
void launch_window_paired(const WindowGeom& g, const int64_t* sum, const uint32_t* cnt, float* paired,
                          hipStream_t st);

// alignment folding (rnamc_align.hip): the triangles of a group of alignment
// rows, each of its own length, summed as integers into the column-pair accumulators of the call
struct AlignItem {
  uint64_t bpp_off;  // float offset of the row's bpp triangle in `bpp`
  uint64_t map_off;  // offset of its column map (u32 per base: the column of base k) in `maps`
  uint32_t n;        // its bases
  uint32_t pad_;
};
// at most 65535 items a launch; max_n: the longest of the launch's items.  sum, cnt and the result
// are packed diagonal-major triangles over the n_cols columns (rnamc_bpp_index)
void launch_align_accumulate(const AlignItem* items, uint32_t n_items, uint32_t max_n, const float* bpp,
                             const uint32_t* maps, uint32_t n_cols, int64_t* sum, uint32_t* cnt, hipStream_t st);
void launch_align_finalize(uint32_t n_cols, uint32_t n_rows, const int64_t* sum, const uint32_t* cnt, float* out,
                           hipStream_t st);
void launch_align_paired(uint32_t n_cols, uint32_t n_rows, const int64_t* sum, const uint32_t* cnt, float* paired,
                         hipStream_t st);

// point-mutation scan (rnamc_mutant.hip): the triangles of a group of mutants, all
// of length n, against the wild type's resident triangle
struct MutantItem {
  uint64_t bpp_off;  // float offset of the mutant's bpp triangle in `bpp`
  uint64_t slot;     // its entry in the call's accumulators
};
// Cells of a strip (one workgroup each) for triangles of `len` cells: 4096 while at most 64 of them
// cover the triangle, beyond that a 64th of it rounded up to whole workgroup steps of 256 cells -- a
// mutant takes at most 64 atomics of either kind however long it is.
constexpr uint32_t kMutantMinStrip = 4096u, kMutantMaxStrips = 64u;
inline uint32_t mutant_strip_of(uint64_t len) {
  const uint64_t per = (len + kMutantMaxStrips - 1u) / kMutantMaxStrips;
  const uint64_t strip = (per + 255u) / 256u * 256u;
  return static_cast<uint32_t>(strip < kMutantMinStrip ? kMutantMinStrip : strip);
}
// at most 65535 items a launch; sum[slot] += the fixed-point squared distance of item and wild type,
// key[slot] = max(key[slot], (bits(|dp|) << 32) | (0xffffffff - cell)) over the cells that moved
void launch_mutant_compare(const MutantItem* items, uint32_t n_items, const float* wt, const float* bpp, uint32_t n,
                           int64_t* sum, uint64_t* key, hipStream_t st);

// structural context profiles (rnamc_context.hip): per-base loop-type
// probabilities off the workspace of a reference-order group.  Rows of a record's profile in CapR's
// order, and the rows of its 64-bit integer accumulators (n + 1 entries each, units of 2^-44: bulge,
// hairpin and internal as difference arrays, multibranch as per-base sums)
enum : int { CTX_ROW_BULGE = 0, CTX_ROW_EXTERIOR = 1, CTX_ROW_HAIRPIN = 2, CTX_ROW_INTERNAL = 3, CTX_ROW_MULTI = 4,
             CTX_ROW_STEM = 5, CTX_ROWS = 6 };
enum : int { CTX_ACC_BULGE = 0, CTX_ACC_HAIRPIN = 1, CTX_ACC_INTERNAL = 2, CTX_ACC_MULTI = 3, CTX_ACC_ROWS = 4 };
struct ContextItem {
  uint64_t qm_off;   // float offset of the record's copy of sums_multibranch in `qm` (tri_pad floats)
  uint64_t acc_off;  // offset of its CTX_ACC_ROWS * (n + 1) accumulators in `acc`
  uint64_t out_off;  // float offset of its CTX_ROWS * n profile in `out`
};
struct ContextBatch {
  const SeqDesc* seqs;       // descriptors of the launch's records, longest first
  const ContextItem* items;  // one per descriptor
  const uint8_t* bases;
  float* workspace;
  const float* bpp;          // the group's finished triangles (SeqDesc::out_off; absent pairs negative)
  const rnamc_params* params;
  const float* hp_init;
  float* qm;
  unsigned long long* acc;   // zeroed by the caller
  float* out;
};
// at most 65535 records a launch; max_n: the longest of them
// M_QM of every record into its copy: between the inside and the outside sweep
void launch_context_save(const ContextBatch& b, uint32_t n_items, uint32_t max_n, hipStream_t st);
// rows 0 .. 4 of every record's profile: behind the group's finalize kernel -> the number of launches
uint32_t launch_context_profile(const ContextBatch& b, bool contra, uint32_t n_items, uint32_t max_n,
                                hipStream_t st);

// RNA-RNA duplex folding (rnamc_duplex.hip): one pair of strands A, B.  Its
// matrices F (inside) and G (outside), nA x nB f64 each (at even float offsets of the workspace), and
// M (max-plus inside), nA x nB f32, are stored LINE-major
// in the direction the chunk steps in: stepping along A (by_col = 0) cell (i, j) sits at
// [i * nB + j], stepping along B (by_col = 1) at [j * nA + i] -- a step's lanes read and write
// consecutive floats either way.
struct DuplexPair {
  uint64_t a_off, b_off;  // offsets of the two strands in the bases buffer
  uint64_t f_off, g_off, m_off;  // float offsets of the three matrices in the workspace (unused ones: 0)
  uint64_t prob_off;      // float offset of the nA x nB probabilities in `probs` (row-major)
  uint64_t bound_off;     // float offset of the nA + nB bound probabilities in `bound`
  uint64_t struct_off;    // byte offset of the nA + nB structure bytes in `structs`
  uint32_t na, nb;
};
struct DuplexRes {
  double log_z;                // ln Z
  float best;                  // max over the cells of outer_end + M
  uint32_t start_i, start_j;   // the cell of `best`: smallest i, then smallest j (0xffffffff: none)
  uint32_t pad_;
};
struct DuplexChunk {
  const DuplexPair* pairs;  // device
  const uint8_t* bases;
  float* ws;
  const rnamc_params* params;
  DuplexRes* res;           // [pair]
  float* probs;             // may be null
  float* bound;             // may be null
  uint8_t* structs;         // may be null
  uint32_t n_pairs;         // at most 65535
  uint32_t by_col;          // 0: steps along A, 1: steps along B
  uint32_t contra;
};
// One step of a sweep: line s of every pair of the chunk in the sweep's own direction (a pair with
// fewer lines idles).  what: 0 inside (F), 1 outside (G), 2 max-plus inside (M).  max_lane: the
// longest line of the chunk.
void launch_duplex_step(const DuplexChunk& c, int what, uint32_t step, uint32_t max_lane, hipStream_t st);
// ln Z (what = 0, from F) or best score and start cell (what = 2, from M): one workgroup per pair
void launch_duplex_reduce(const DuplexChunk& c, int what, hipStream_t st);
// match probabilities (c.probs) and / or bound probabilities (c.bound) from F, G and ln Z
void launch_duplex_probs(const DuplexChunk& c, uint64_t max_cells, uint32_t max_bases, hipStream_t st);
// argmax traceback from the start cell: the nA + nB structure bytes of every pair
void launch_duplex_trace(const DuplexChunk& c, hipStream_t st);

// ---- tree-order summation mode (rnamc_tree.hip) ----
// Dense n x n matrices with row stride ld (>= n + 32, a multiple of 32 floats), msz floats
// each; "row" = [i * ld + j], "col" = [j * ld + i].  The outside sweep reuses four slots.
enum TreeMat : int {
  T_QB = 0,   // sums_close                                   row
  T_QA = 1,   // sums_accessible                              row
  T_Q1R = 2,  // sums_1ormore_basepairs                       row
  T_Q1C = 3,  // sums_1ormore_basepairs                       col
  T_ZRE = 4,  // sums_rightmost_basepairs_external            col | outside: W = (P + mbclose) - Qb, row
  T_ZRM = 5,  // sums_rightmost_basepairs_multibranch         col | outside: R = Pm (+) Pm2, col
  T_QM = 6,   // sums_multibranch                             row | outside: probs_multibranch2, row
  T_U = 7,    // column prefix of Zr_mb (first fold of L_c)   col | outside: column prefix of Pm, col
  T_HP = 8,    // hairpin score of the pair (static)                        row
  T_MBC = 9,   // multibranch_close score; -inf = (i,j) may not pair (static) row
  T_X4 = 10,   // four planes (one per 2-loop class), row: inside QbX4 = sums_close + IN4[class],
               // outside PX4 = (log bpp - sums_close) + CS4[class]: a probe reads the plane of its class
  T_ACCS = 14, // accessible score (static)                                  row
  T_CS4 = 15,  // float4 per cell, row: the pair as CLOSING pair of a generic 2-loop, by class (static)
  T_IN4 = 19,  // float4 per cell, row: the pair as ENCLOSED pair (static)
  T_NEAR4 = 23,  // float4 per cell, row: scores of the explicit small 2-loops this pair CLOSES, slots 0..3 of
                 // Special<>::slot: enclosed pair (i+1,j-1), (i+1,j-2), (i+2,j-1), (i+2,j-2) (static)
  T_NEAR8 = 27,  // float4 per cell, row: slots 4..6 (Turner: 1x2, 2x1, 2x2; .w unused) (static)
  // lane-per-cell sweeps (rnamc_tree_lane.h), DIAGONAL-major: cell (i, j) at [(j - i) * ld + i], so that
  // the 64 consecutive rows a wave holds read and write consecutive floats.  In those sweeps the four
  // T_X4 planes are diagonal-major too (their only readers are the sweeps' own 2-loop sums).
  T_QB_D = 31,   // sums_close
  T_Q1_D = 32,   // sums_1ormore_basepairs
  T_ZRM_D = 33,  // sums_rightmost_basepairs_multibranch | outside: R
  T_W_D = 34,    // outside: W
  T_LIST = 35,   // u32 per entry: row d holds the rows i of the cells (i, i + d) that may pair, in order; the
                 // count in the row's last entry (k_tlane_list; the 2-loop sums run a lane per LISTED cell)
  T_GEN_D = 36,  // float2 per cell over two slots: {max, sum} of a listed cell's generic 2-loop terms (k_tlane_gen,
                 // three diagonals a launch; as ONE f32 logarithm it cost an ulp of a ~300-nat value per cell and
                 // diagonal: 2.6e-4 in the probabilities at n = 257, measured)
  T_COUNT = 38,
  // ... and in those sweeps these slots hold diagonal-major data as well:
  T_ZRE_D = T_QB,  // sums_rightmost_basepairs_external (the row-major sums_close has no reader there)
  T_QA_D = T_W_D,  // sums_accessible until the band is spread into T_QA (inside sweep)
  T_P2_D = T_QB     // outside sweep: float2 per cell over the slots T_QB and T_QA (both free once the inside sweep
                    // and its sums_external are through): {max, sum} of the pair's enclosing 2-loop terms
  // T_QM, T_U: sums_multibranch / the column prefix (inside), probs_multibranch2 / the column prefix of
  // probs_multibranch (outside); the statics (T_HP .. T_NEAR8): cell (i, j) at [(j - i) * ld + i] too
};
// Length-dependent part of a generic 2-loop score per probe slot (rnamc_tree.hip, probe_slot),
// derived from rnamc_params on the host (rnamc_sweep_tree.cpp, build_tree_tabs).  Model index 0 Turner,
// 1 CONTRAfold.
struct TreeTabs {
  float len[2][512];
  // lane-per-cell sweeps: the generic slots by class, inside a class in order of a + b (a prefix of the
  // class's list is what a cell of a given span can enclose): a | (a + b) << 8, the slot's length term;
  // class c's list starts at gstart[c] (a multiple of 8; lists padded to multiples of 8 with their
  // last slot), gcount[c][s] of its slots have a + b <= s
  uint32_t gslot[2][544];
  float glen[2][544];
  uint32_t gstart[2][4];
  uint32_t gcount[2][4][32];
  // ... and class 3 (both unpaired stretches >= 2 bases: three quarters of the slots) once more in runs: on a
  // level a + b = s its slots are CONSECUTIVE a, i.e. consecutive floats of one diagonal row, so four of them
  // are one 16-byte load.  Group g: first a | s << 8, the four length terms (-inf beyond the level's run);
  // g4count[s] of the groups have a + b <= s; the list is padded with eight empty groups.
  uint32_t g4slot[2][128];
  float g4len[2][128][4];
  uint32_t g4count[2][32];
  // ... and classes 0 and 1 (bulges, 1 x many) by LEVEL a + b = s: their slots are (0, s), (s, 0), (1, s - 1),
  // (s - 1, 1) — the row's first and last two positions — so a level is four loads whose offsets are the level's
  // row plus 0, s, 1, s - 1: no slot list at all.  elen[s] = the four length terms (-inf: not a generic slot).
  float elen[2][32][4];
};
struct TreeSeq {
  uint32_t n, ld;
  uint64_t msz;       // floats per matrix
  uint64_t seq_off;   // first base in the bases buffer
  uint64_t ws_off;    // float offset of the first matrix; after the T_COUNT matrices come the
                      // vectors Z(0,.) and Z(.,n-1), n + 64 floats each
  uint64_t out_off;   // float offset of the packed bpp triangle in the output
  uint64_t pk_off;    // float offset of the 2-bit packed copy of the bases (pk_words words)
  uint32_t pk_words;
  uint32_t batch_idx;
  uint64_t mid_off;   // float offset of the banded mid-field ring: three products x `ring`
                      // diagonals x (n + 64 rounded up to 64) cells x {max, sum} (rnamc_tree.hip)
};
struct TreeBatch {
  const TreeSeq* seqs;  // descriptors of the group (device memory)
  TreeSeq one;          // the descriptor itself when the group is a single sequence (use_one):
  uint32_t use_one;     // saves the dependent descriptor load in front of every launch
  const uint8_t* bases;
  float* workspace;
  float* out;
  float* log_partition;
  const rnamc_params* params;
  const TreeTabs* tabs;
  const float* hp_init;
  int allows_short_hairpins;
  int debug;  // timing experiments (builds with -DRNAMC_DEBUG_KNOBS only; 0 otherwise)
  uint32_t ring;  // diagonals the mid-field ring holds (twice the band width; 0: no banding)
  uint32_t lane;  // != 0: both sweeps run lane-per-cell (rnamc_tree_lane.h: statics and sweep matrices diagonal-major)
  const int32_t* cons;  // hard constraints, as DeviceBatch (read by k_tree_static alone)
  uint32_t max_span;
};
// Launch-shape policy of the tree-order sweep, per context (rnamc_ctx_set "tree_waves",
// "tree_short", "tree_ahead_waves", "tree_mid_wgs"): passed to every launch, no process globals.
struct TreePolicy {
  uint64_t waves = 5120;            // waves a launch may hold at once (5 per SIMD at ~88 VGPRs)
  uint32_t short_terms = 256;       // sums up to this many terms take one wave per cell
  uint64_t ahead_waves = 16384;    // waves up to which the ahead role takes one wave per CELL (a lone sequence;
                                    // beyond — batches — one per row: 8 % faster there, profiles/r04_tree_on_batches.txt)
  uint32_t xcd_rows = 0;            // != 0: workgroup ids of a sweep launch are dealt so that runs of 8 workgroups
                                    // (32 rows of a sequence) share an XCD, rotated by sequence (see xcd_chunk)
  uint32_t mid_wgs = 0;             // workgroups of a k_tree_mid launch; 0: by the longest sequence (256 below
                                    // 6 144 nt, 512 below 12 288, 1 024 beyond: from ~8 000 nt on the mid-field
                                    // products, not the launch chain, set the sweep's time: profiles/r04_tree_long.txt)
  uint32_t mid_mx = 1;              // != 0: the mid-field products on the matrix cores (k_tree_mid_mx, rnamc_tree_mx.h:
                                    // factors 2^(x log2 e - E) per operand element, v_mfma_f32_32x32x2_f32 per term)
};
// what = 0: everything before the inside sweep; 1: the four reused slots before the outside sweep
void launch_tree_init(const TreeBatch& b, uint32_t nseq, uint32_t max_n, bool contra, int what,
                      hipStream_t st);
// tpc_knob: threads per cell (64, 256, 1024), anything else = chosen by the diagonal's cells;
// two: diagonals d and d+1 in one launch (inside: d then d+1; outside: d+1 then d)
// thr: banded mid-field threshold of the launch's band (0: none; the launch's sums run whole)
// use_far: the far parts of this launch's 2-loop blocks were written by the previous launch's
// ahead role; nd0, nd_count: the diagonals of the NEXT launch, whose far parts this launch's extra
// workgroups write (nd_count = 0: none).  Needs the far ring of a banded workspace (ring != 0).
void launch_tree_inside(const TreeBatch& b, bool contra, uint32_t d, uint32_t max_n, uint32_t nseq,
                        int64_t tpc_knob, bool two, uint32_t thr, bool use_far, uint32_t nd0,
                        uint32_t nd_count, const TreePolicy& pol, hipStream_t st);
void launch_tree_outside(const TreeBatch& b, bool contra, uint32_t d, uint32_t max_n, uint32_t nseq,
                         int64_t tpc_knob, bool two, uint32_t thr, bool use_far, uint32_t nd0,
                         uint32_t nd_count, const TreePolicy& pol, hipStream_t st);
// Mid-field of the cubic products for the cells of diagonals [dlo, dhi] (one band), threshold thr:
// inside (outside = false) sums_multibranch, outside probs_multibranch and the Q1 x R part of L_e
void launch_tree_mid(const TreeBatch& b, bool outside, uint32_t dlo, uint32_t dhi, uint32_t thr,
                     uint32_t max_n, uint32_t nseq, const TreePolicy& pol, hipStream_t st);
// sums_external's first row and last column of a banded sweep, diagonals [dlo, dhi] (in order)
void launch_tree_ext(const TreeBatch& b, bool contra, uint32_t dlo, uint32_t dhi, uint32_t max_n,
                     uint32_t nseq, hipStream_t st);
// Does `side` run beside `main`?  A bounded spin (~120 us of s_memtime ticks, every wave exits) on
// `side`, a trivial kernel on `main` behind it in submission order, events around the latter: if
// the trivial kernel only ends when the spin does, the two streams share a hardware queue.
// Returns 1 (concurrent), 2 (serialised), 0 on any HIP error.  Synchronises both streams.
int tree_side_stream_probe(hipStream_t main, hipStream_t side);
// per-cell statics (hairpin / multibranch-close / accessible scores, 2-loop sides), once per group
void launch_tree_static(const TreeBatch& b, bool contra, uint32_t nseq, uint32_t max_n, hipStream_t st);
// lane-per-cell sweeps of a batch (rnamc_tree_lane.h): one diagonal per launch, a lane per cell
// d: the diagonal whose cells take their sums and recurrences (a lane per row); d_b: the diagonal whose LISTED
// cells (the ones that may pair) take their 2-loop sums in the same launch — one diagonal ahead of d in the
// sweep's direction (either >= max_n: that role is absent)
void launch_tlane_inside(const TreeBatch& b, bool contra, uint32_t d, uint32_t d_b, uint32_t max_n, uint32_t nseq,
                         uint32_t thr, hipStream_t st);
void launch_tlane_outside(const TreeBatch& b, bool contra, uint32_t d, uint32_t d_b, uint32_t max_n, uint32_t nseq,
                          uint32_t thr, hipStream_t st);
// generic 2-loop sums of the listed cells of `count` (<= 3) diagonals from g0 on (inside upwards, outside downwards)
void launch_tlane_gen(const TreeBatch& b, bool contra, bool outside, uint32_t g0, uint32_t count, uint32_t max_n,
                      uint32_t nseq, hipStream_t st);
// the rows of the cells that may pair, diagonal by diagonal (after launch_tree_static)
void launch_tlane_list(const TreeBatch& b, uint32_t max_n, uint32_t nseq, hipStream_t st);
// the finished band [dlo, dhi] into the row- / column-major copies k_tree_mid and k_tree_ext read
void launch_tlane_spread(const TreeBatch& b, bool outside, uint32_t dlo, uint32_t dhi, uint32_t max_n, uint32_t nseq,
                         hipStream_t st);
void launch_tree_finalize(const TreeBatch& b, uint32_t nseq, uint32_t max_n, hipStream_t st);

}  // namespace rnamc

#endif
