// rnamc_internal.h — declarations shared by the host and device translation
// units of librnamc.so.  Not part of the public ABI.
#ifndef RNAMC_INTERNAL_H
#define RNAMC_INTERNAL_H

#include <atomic>
#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rnamc.h"

namespace rnamc {

void set_last_error(const std::string& msg);
bool is_canonical(int a, int b);
// Turner hairpin initiation by loop length 0 .. len-1, extrapolated past
// max_hairpin_len_extrapolation (src/utils.rs:174-183): the `hp_init` table of the Turner scorer
void hp_init_table(const rnamc_turner_scores& t, uint32_t len, float* out);
// Hard constraints (include/rnamc.h): the n bytes of a constraint string over
// ". x ( ) < >" into the 2n words pair_allowed reads (rnamc_scoring.h).  RNAMC_ERR_INVALID_ARG for a
// byte outside the set or an unbalanced bracket, with its position in *bad_pos and the reason in *why.
int compile_constraint(const char* str, uint32_t n, int32_t* words, uint32_t* bad_pos, const char** why);

// Where the records of a batch core write in the caller's arrays.  The three cores below serve a
// context entry, whose records are the caller's (the identity: both pointers NULL), and a pool's
// shard, whose record s is the caller's record res_idx[s] and starts base_off[s] bases into the
// caller's batch (RecordShards, rnamc_shards.h).  Per-record results go to index idx(s), per-base
// results to a multiple of base(s, offsets) that the core knows.
struct Place {
  const uint32_t* res_idx = nullptr;
  const uint64_t* base_off = nullptr;
  uint32_t idx(uint32_t s) const { return res_idx ? res_idx[s] : s; }
  uint64_t base(uint32_t s, const uint64_t* offsets) const { return base_off ? base_off[s] : offsets[s] - offsets[0]; }
};

// rnamc_centroid_fold_batch behind its two entries (rnamc_entries_centroid.cpp): the arguments of the entry after
// centroid_fold_batch_check, plus where sequence s writes — its rows at structs + n_thresholds * base(s),
// its per-threshold results at index idx(s) * n_thresholds, its log partition at idx(s)
int centroid_fold_batch_check(uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
                              const float* gammas, uint32_t ng, const uint8_t* structs, const float* bpp,
                              const uint64_t* out_offsets);
int centroid_fold_batch_core(rnamc_ctx* c, uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
                             const char* constraints, uint32_t max_bp_span, int uses_contra_model,
                             int allows_short_hairpins, const float* gammas, uint32_t ng, uint8_t* structs,
                             const Place& place, uint32_t* n_pairs, float* expect_accuracy,
                             float* log_partition, float* bpp, const uint64_t* out_offsets);

// rnamc_bpp_batch_sparse behind its two entries (rnamc_entries_sparse.cpp): the arguments of the entry after
// bpp_batch_sparse_check, plus where sequence s writes — count, start and log partition at index
// idx(s), paired probabilities at paired_prob + base(s) — and the cursor from which every
// group claims its part of the three list arrays (shared by the shards of a pool)
int bpp_batch_sparse_check(uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets, float min_prob,
                           const uint64_t* pair_start, const uint64_t* pair_count, const uint32_t* pair_i,
                           const uint32_t* pair_j, const float* pair_prob, const uint64_t* pairs_total);
int bpp_batch_sparse_core(rnamc_ctx* c, uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
                          const char* constraints, uint32_t max_bp_span, int uses_contra_model,
                          int allows_short_hairpins, float min_prob, const Place& place, uint64_t* pair_start,
                          uint64_t* pair_count, uint32_t* pair_i, uint32_t* pair_j, float* pair_prob,
                          uint64_t pairs_cap, std::atomic<uint64_t>* cursor, float* paired_prob,
                          float* log_partition);
int bpp_batch_sparse_finish(uint64_t total, bool wants_lists, uint64_t pairs_cap, uint64_t* pairs_total);

// rnamc_context_profile_batch behind its two entries (rnamc_entries_context.cpp): the arguments of
// the entry after context_profile_check, plus where sequence s writes — its six rows at profile +
// 6 * base(s), its log partition at index idx(s)
int context_profile_check(uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets, const float* profile);
int context_profile_core(rnamc_ctx* c, uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
                         const char* constraints, uint32_t max_bp_span, int uses_contra_model,
                         int allows_short_hairpins, const Place& place, float* profile, float* log_partition);

// rnamc_bpp_windowed behind its two entries (rnamc_entries_window.cpp).  The window list of a call:
// n_grid windows at 0, stride, 2 stride, ..., and with has_last one more at n - w.
struct WindowPlan {
  uint64_t n = 0, n_windows = 0, n_grid = 0;
  uint32_t w = 0, stride = 0, band = 0, has_last = 0;
  uint64_t start(uint64_t x) const { return x < n_grid ? x * stride : n - w; }
};
// the plan of (n, window, stride, max_bp_span): RNAMC_ERR_EMPTY_SEQ / RNAMC_ERR_INVALID_ARG as the entry
int window_plan_of(uint64_t n, uint32_t window, uint32_t stride, uint32_t max_bp_span, WindowPlan* out);
// every check of the entry that needs no context: pointers, the plan, bases, the constraint's bytes
int bpp_windowed_check(const uint8_t* bases, uint64_t n, const char* constraint, uint32_t window, uint32_t stride,
                       uint32_t max_bp_span, const float* band_prob, WindowPlan* out);
// The three below run with c->mu HELD by the caller and the context's device current (the
// accumulators live in the context from the first of them to the last).
// zero the context's accumulators and add windows [first, first + count) into them, chunk by chunk;
// window_log_partition (may be NULL) is the call's whole array
int bpp_windowed_accumulate(rnamc_ctx* c, const WindowPlan& wp, const uint8_t* bases, const char* constraint,
                            uint64_t first, uint64_t count, int uses_contra_model, int allows_short_hairpins,
                            float* window_log_partition);
// the context's accumulators to the host (band * n entries each, [d * n + i])
int bpp_windowed_fetch(rnamc_ctx* c, const WindowPlan& wp, int64_t* sum, uint32_t* cnt);
// finalise and paired kernels and the copies to the host; sum / cnt: host totals to upload first
// (both NULL: the context's own accumulators as bpp_windowed_accumulate left them)
int bpp_windowed_finish(rnamc_ctx* c, const WindowPlan& wp, const int64_t* sum, const uint32_t* cnt,
                        float* band_prob, float* paired_prob);

// rnamc_bpp_alignment behind its two entries (rnamc_entries_align.cpp).  Rows of an alignment cut into
// records: row row_idx[s] without its gaps is record s, bases [offsets[s], offsets[s + 1]) (offsets[0]
// = 0); maps is laid out like bases and holds the column of every base.  The single-context entry
// holds all rows in order, a pool's shard some of them.
struct AlignRows {
  uint32_t n_cols = 0;
  std::vector<uint8_t> bases;
  std::vector<uint64_t> offsets;
  std::vector<uint32_t> maps;
  std::vector<uint32_t> row_idx;
};
// every check of the entry that needs no context: pointers, sizes, the codes of every row (the bad
// row named in rnamc_last_error); *out = all rows
int bpp_alignment_check(uint32_t n_rows, uint32_t n_cols, const uint8_t* rows, const float* gammas, uint32_t ng,
                        const uint8_t* structs, const uint32_t* n_pairs, const float* expect_accuracy,
                        AlignRows* out);
// The three below run with c->mu HELD by the caller and the context's device current (the
// accumulators live in the context from the first of them to the last).
// zero the context's accumulators and add the rows of `ar` into them group by group;
// log_partition (may be NULL) is the call's whole array, indexed by row
int bpp_alignment_accumulate(rnamc_ctx* c, const AlignRows& ar, uint32_t max_bp_span, int uses_contra_model,
                             int allows_short_hairpins, float* log_partition);
// the context's accumulators to the host (n_cols (n_cols + 1) / 2 entries each, rnamc_bpp_index)
int bpp_alignment_fetch(rnamc_ctx* c, uint32_t n_cols, int64_t* sum, uint32_t* cnt);
// average, column profile and consensus folds, and the copies to the host; sum / cnt: host totals to
// upload first (both NULL: the context's own accumulators as bpp_alignment_accumulate left them)
int bpp_alignment_finish(rnamc_ctx* c, uint32_t n_rows, uint32_t n_cols, const int64_t* sum, const uint32_t* cnt,
                         const float* gammas, uint32_t ng, float* bpp, float* col_paired, uint8_t* structs,
                         uint32_t* n_pairs, float* expect_accuracy);

// rnamc_mutant_scan behind its two entries (rnamc_entries_mutant.cpp).
// base code of the rank-th (0 .. 2) mutant of a position whose wild-type base is wt: {0,1,2,3} \ {wt} ascending
inline uint8_t mutant_base_of(uint8_t wt, uint32_t rank) { return static_cast<uint8_t>(rank + (rank >= wt ? 1u : 0u)); }
// every check of the entry that needs no context: pointers, the record, the position list, the
// constraint; *n_mutants = 3 * (number of positions)
int mutant_scan_check(const uint8_t* bases, uint32_t n, const char* constraint, const uint32_t* positions,
                      uint32_t n_positions, const float* log_partition, uint64_t* n_mutants);
// Runs with c->mu HELD by the caller and the context's device current: folds the wild type, then
// mutants [first, first + count) of the list chunk by chunk.  The per-mutant outputs are the call's
// whole arrays (indexed by m); the wild-type outputs may be NULL (a pool's later shards).
int mutant_scan_core(rnamc_ctx* c, const uint8_t* bases, uint32_t n, const char* constraint, uint32_t max_bp_span,
                     int uses_contra_model, int allows_short_hairpins, const uint32_t* positions, uint64_t first,
                     uint64_t count, float* log_partition, int64_t* pair_dist2_q, float* max_dp, uint32_t* max_i,
                     uint32_t* max_j, float* paired_prob, float* wt_log_partition, float* wt_paired_prob);

// rnamc_duplex_batch behind its two entries (rnamc_entries_duplex.cpp).
// every check of the entry that needs no context: pointers, outputs and their offsets, the records,
// the pair indices
int duplex_batch_check(uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets, uint32_t n_pairs,
                       const uint32_t* pair_a, const uint32_t* pair_b, const float* match_probs,
                       const uint64_t* out_offsets, const float* bound_a, const float* bound_b,
                       const uint64_t* bound_offsets, const uint8_t* structs, const uint64_t* struct_offsets);
// pairs [first, first + count) of the caller's list on one context: only the records they name are
// uploaded; every output is the call's whole array, written at the caller's offsets and pair indices
int duplex_batch_core(rnamc_ctx* c, const uint8_t* bases, const uint64_t* offsets, uint32_t first,
                      uint32_t count, const uint32_t* pair_a, const uint32_t* pair_b, int uses_contra_model,
                      float* match_probs, const uint64_t* out_offsets, float* bound_a, float* bound_b,
                      const uint64_t* bound_offsets, float* log_partition, uint8_t* structs,
                      const uint64_t* struct_offsets, float* best_scores);

// DP matrices of one sequence inside the workspace.  Every matrix is a packed
// upper triangle of n(n+1)/2 f32 (padded to a multiple of 64 floats):
//  - "diag-major": cell (i,j) at  d*n - d(d-1)/2 + i  with d = j-i.  A lane that
//    owns row i of a diagonal sweep then reads consecutive addresses next to its
//    neighbours' for every k of the reference's inner loops.
//  - "row-major":  cell (r,c) at  r*n - r(r-1)/2 + (c-r).
enum Mat : int {
  M_QB = 0,   // sums_close                          diag-major
  M_QA = 1,   // sums_accessible                     diag-major
  M_MBC = 2,  // multibranch_close_scores            diag-major
  M_Z = 3,    // sums_external                       diag-major
  M_Q1D = 4,  // sums_1ormore_basepairs              diag-major
  M_Q1C = 5,  // sums_1ormore_basepairs              column-major, shifted one row (see col_off)
  M_ZRE = 6,  // sums_rightmost_basepairs_external   diag-major (inside pass)
  M_PM = 6,   // probs_multibranch                   column-major (outside pass, same slot)
  M_QM = 7,   // sums_multibranch                    diag-major (inside pass)
  M_PM2 = 7,  // probs_multibranch2                  column-major (outside pass, same slot)
  M_W = 8,    // (P + mbclose) - Qb of a pair        diag-major (outside pass)
  M_ZRM = 9,  // sums_rightmost_basepairs_multibranch diag-major (CONTRAfold, inside pass)
  M_P = 9,    // log basepair_probs                  diag-major (outside pass, same slot)
  M_PQ = 10,  // {log basepair_prob, sums_close} of a FINISHED pair, interleaved (float2, two
              // slots), diag-major: the enclosing-pair probes read both with one 8-byte gather
  M_COUNT = 12
};

struct SeqDesc {
  uint32_t n;
  uint32_t tri_pad;   // padded floats per matrix
  uint64_t seq_off;   // offset of the first base in the bases buffer
  uint64_t ws_off;    // float offset of this sequence's matrices in the workspace
  uint64_t out_off;   // float offset of this sequence's bpp triangle in the output
  uint32_t batch_idx; // position in the caller's batch (for log_partition)
  uint32_t pk_words;  // 32-bit words of the 2-bit packed sequence copy
  uint64_t pk_off;    // float offset of that copy in the workspace
  uint64_t cidx_off;  // float offset of the u16 lists of canonical cells (one per diagonal)
  uint64_t ccnt_off;  // float offset of the u32 list lengths (one per diagonal)
  uint64_t c64_off;   // float offset of the u32 table: canonical cells before position 64*w
                      // of diagonal D at [w * (n + 64) + D]
};

// Traceback of the gamma-centroid fold (src/centroid_fold.rs:64-102): exact float equality
// tests in the order left-skip, right-skip, pair, first bifurcation k.  M(r, c) reads the filled
// matrix (0 below and on the main diagonal), prob(i, j) the bpp entry (negative = absent).
template <class MatFn, class ProbFn>
inline uint32_t centroid_traceback(uint32_t n, float centroid_threshold, MatFn&& M, ProbFn&& prob,
                                   uint32_t* pairs_out, uint32_t max_pairs) {
  uint32_t np = 0;
  std::vector<std::pair<uint32_t, uint32_t>> stack;
  stack.emplace_back(0u, n - 1);
  while (!stack.empty()) {
    auto [i, j] = stack.back();
    stack.pop_back();
    if (j <= i) continue;
    const float best = M(i, j);
    if (best == 0.f) continue;
    if (best == M(i + 1, j)) {
      stack.emplace_back(i + 1, j);
    } else if (best == M(i, j - 1)) {
      stack.emplace_back(i, j - 1);
    } else if (prob(i, j) >= -0.5f &&
               best == M(i + 1, j - 1) + centroid_threshold * prob(i, j) - 1.f) {
      stack.emplace_back(i + 1, j - 1);
      if (pairs_out && np < max_pairs) {
        pairs_out[2 * np] = i;
        pairs_out[2 * np + 1] = j;
      }
      np++;
    } else {
      for (uint32_t k = i + 1; k < j; k++) {
        if (best == M(i, k) + M(k + 1, j)) {
          stack.emplace_back(i, k);
          stack.emplace_back(k + 1, j);
          break;
        }
      }
    }
  }
  return np;
}

}  // namespace rnamc

#endif
