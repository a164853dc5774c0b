// rnamc_pool.cpp — the batch entry over SEVERAL devices behind the C ABI.
//
// The reference fans a FASTA out over all cores inside the binary, one pool task per record
// (src/bin/mccaskill_algo.rs:58-93, src/bin/centroid_fold.rs:119-132).  The drop-in's
// equivalent is one device context + one host thread per GPU: the batch is cut into as many
// shards as there are contexts, every shard runs through rnamc_bpp_batch of its own context
// (H2D, sweeps, D2H on that device's streams) and writes straight into the caller's host
// triangles.  Sequences are independent and never split: there is no
// collective and no device-to-device traffic.
//
// Shards are contiguous bands of the cost-sorted batch with equal total cost under the
// measured model of one sweep (a * n(n^2-1)/6 + b * n^2: the Theta(n^3) folds plus the
// Theta(496 n^2) 2-loop blocks), so every device's lock-step groups hold
// sequences of similar length and stay large on every diagonal.
//
// Every _multi entry below reads as the same steps: the argument checks of its context entry (nothing
// of the pool is read before they pass), the shards (RecordShards or list_shards, rnamc_shards.h),
// run_shards with what one context does with one shard, and for the two averaging entries the sum of
// the shards' integer accumulators, finished on the pool's first context.
#include "rnamc_entries.h"

using namespace rnamc;

struct rnamc_pool {
  std::vector<rnamc_ctx*> ctxs;
  std::vector<int> devices;
  std::mutex mu;  // one batch at a time per pool
  uint32_t size() const { return static_cast<uint32_t>(ctxs.size()); }
};

namespace {

// One context's part of an entry whose cores run with c->mu held (windows, alignment rows, mutants):
// the context's lock and device around `work`, own_stream drained when it fails.
int on_ctx(rnamc_ctx* c, const std::function<int()>& work) {
  std::unique_lock<std::mutex> ctx_lock(c->mu);
  DeviceGuard guard(c->device);
  if (!guard.ok) return RNAMC_ERR_NO_DEVICE;
  const int rc = work();
  if (rc) (void)hipStreamSynchronize(c->own_stream);
  return rc;
}

}  // namespace

extern "C" {

int rnamc_sweep_cost(uint32_t count, const uint64_t* lengths, double* cost_s) {
  if (count && (!lengths || !cost_s)) return RNAMC_ERR_INVALID_ARG;
  for (uint32_t x = 0; x < count; x++) cost_s[x] = sweep_cost(lengths[x]);
  return RNAMC_OK;
}

int rnamc_shard_plan(uint32_t n_seqs, const uint64_t* offsets, uint32_t n_shards,
                     uint32_t* shard_of_seq) {
  if (!offsets || !shard_of_seq || n_shards == 0) return RNAMC_ERR_INVALID_ARG;
  for (uint32_t s = 0; s < n_seqs; s++)
    if (offsets[s + 1] < offsets[s]) return RNAMC_ERR_INVALID_ARG;
  if (n_seqs) plan(n_seqs, offsets, n_shards, shard_of_seq, nullptr);
  return RNAMC_OK;
}

int rnamc_pool_create(const rnamc_params* params, const int* devices, uint32_t n_devices,
                      uint64_t workspace_bytes, rnamc_pool** out) {
  if (!params || !out || (n_devices && !devices)) return RNAMC_ERR_INVALID_ARG;
  *out = nullptr;
  std::vector<int> devs;
  if (n_devices == 0) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
      rnamc::set_last_error("no HIP device visible: librnamc has no CPU fallback");
      return RNAMC_ERR_NO_DEVICE;
    }
    for (int d = 0; d < count; d++) devs.push_back(d);
  } else {
    devs.assign(devices, devices + n_devices);
  }
  rnamc_pool* p = new (std::nothrow) rnamc_pool();
  if (!p) return RNAMC_ERR_OOM;
  for (int d : devs) {
    rnamc_ctx* c = nullptr;
    const int rc = rnamc_ctx_create(params, d, workspace_bytes, &c);
    if (rc) {
      rnamc_pool_destroy(p);
      return rc;
    }
    p->ctxs.push_back(c);
    p->devices.push_back(d);
  }
  *out = p;
  return RNAMC_OK;
}

void rnamc_pool_destroy(rnamc_pool* p) {
  if (!p) return;
  for (rnamc_ctx* c : p->ctxs) rnamc_ctx_destroy(c);
  delete p;
}

uint32_t rnamc_pool_size(const rnamc_pool* p) { return p ? static_cast<uint32_t>(p->ctxs.size()) : 0u; }

rnamc_ctx* rnamc_pool_ctx(rnamc_pool* p, uint32_t idx) {
  return (p && idx < p->ctxs.size()) ? p->ctxs[idx] : nullptr;
}

int rnamc_pool_set_params(rnamc_pool* p, const rnamc_params* params) {
  if (!p || !params) return RNAMC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(p->mu);
  for (rnamc_ctx* c : p->ctxs)
    if (int rc = rnamc_ctx_set_params(c, params)) return rc;
  return RNAMC_OK;
}

int rnamc_pool_set(rnamc_pool* p, const char* name, int64_t value) {
  if (!p || !name) return RNAMC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(p->mu);
  for (rnamc_ctx* c : p->ctxs)
    if (int rc = rnamc_ctx_set(c, name, value)) return rc;
  return RNAMC_OK;
}

int rnamc_bpp_batch_multi(rnamc_pool* p, uint32_t n_seqs, const uint8_t* bases,
                          const uint64_t* offsets, int uses_contra_model,
                          int allows_short_hairpins, float* bpp, const uint64_t* out_offsets,
                          float* log_partition) {
  return rnamc_bpp_batch_multi_constrained(p, n_seqs, bases, offsets, nullptr, 0, uses_contra_model,
                                           allows_short_hairpins, bpp, out_offsets, log_partition);
}

// rnamc_bpp_batch_constrained over the pool.  The whole batch is validated before any device sees a
// part of it: one bad record fails the call with its status and nothing is computed (the reference
// panics before its pool starts for bad bytes, src/bin/mccaskill_algo.rs:50-56).  The context entry
// has no core with a placement, so every shard takes its members' triangle offsets gathered — the
// triangles go straight into the caller's — and its log partitions are scattered afterwards.
int rnamc_bpp_batch_multi_constrained(rnamc_pool* p, uint32_t n_seqs, const uint8_t* bases,
                                      const uint64_t* offsets, const char* constraints,
                                      uint32_t max_bp_span, int uses_contra_model,
                                      int allows_short_hairpins, float* bpp,
                                      const uint64_t* out_offsets, float* log_partition) {
  const char* who = "rnamc_bpp_batch_multi";
  if (!p || !offsets || !out_offsets || (n_seqs && (!bases || !bpp))) return RNAMC_ERR_INVALID_ARG;
  if (n_seqs == 0) return RNAMC_OK;
  if (int rc = check_records(n_seqs, bases, offsets)) return rc;
  if (int rc = check_constraints(n_seqs, offsets, constraints)) return rc;
  if (p->ctxs.empty()) return RNAMC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(p->mu);
  RecordShards rs;
  if (int rc = rs.build(who, n_seqs, bases, offsets, constraints, p->size(), out_offsets)) return rc;
  const uint32_t n_shards = static_cast<uint32_t>(rs.shards.size());
  std::vector<std::vector<float>> logz;
  try {  // nothing may throw across the C boundary
    logz.resize(n_shards);
    for (uint32_t k = 0; k < n_shards; k++) logz[k].resize(rs.shards[k].count());
  } catch (const std::exception&) {
    return no_host_memory(who);
  }
  if (int rc = run_shards(who, n_shards, [&](uint32_t k) {
        const RecordShards::Shard& sh = rs.shards[k];
        return rnamc_bpp_batch_constrained(p->ctxs[k], sh.count(), sh.bases.data(), sh.offsets.data(),
                                           sh.constraints(), max_bp_span, uses_contra_model, allows_short_hairpins,
                                           bpp, sh.out_offsets.data(), log_partition ? logz[k].data() : nullptr);
      }))
    return rc;
  if (log_partition)
    for (uint32_t k = 0; k < n_shards; k++)
      for (uint32_t x = 0; x < rs.shards[k].count(); x++) log_partition[rs.shards[k].members[x]] = logz[k][x];
  return RNAMC_OK;
}

// rnamc_centroid_fold_batch over the pool: the shards of rnamc_bpp_batch_multi_constrained, each through
// its own context, rows, counts, accuracies, log partitions and triangles written straight into the
// caller's arrays.
int rnamc_centroid_fold_batch_multi(rnamc_pool* p, uint32_t n_seqs, const uint8_t* bases,
                                    const uint64_t* offsets, const char* constraints, uint32_t max_bp_span,
                                    int uses_contra_model, int allows_short_hairpins,
                                    const float* centroid_thresholds, uint32_t n_thresholds, uint8_t* structs,
                                    uint32_t* n_pairs, float* expect_accuracy, float* log_partition, float* bpp,
                                    const uint64_t* out_offsets) {
  const char* who = "rnamc_centroid_fold_batch_multi";
  if (!p) return RNAMC_ERR_INVALID_ARG;
  if (int rc = centroid_fold_batch_check(n_seqs, bases, offsets, centroid_thresholds, n_thresholds, structs, bpp,
                                         out_offsets))
    return rc;
  if (n_seqs == 0) return RNAMC_OK;
  if (int rc = check_constraints(n_seqs, offsets, constraints)) return rc;
  if (p->ctxs.empty()) return RNAMC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(p->mu);
  RecordShards rs;
  if (int rc = rs.build(who, n_seqs, bases, offsets, constraints, p->size(), out_offsets)) return rc;
  return run_shards(who, static_cast<uint32_t>(rs.shards.size()), [&](uint32_t k) {
    const RecordShards::Shard& sh = rs.shards[k];
    return centroid_fold_batch_core(p->ctxs[k], sh.count(), sh.bases.data(), sh.offsets.data(), sh.constraints(),
                                    max_bp_span, uses_contra_model, allows_short_hairpins, centroid_thresholds,
                                    n_thresholds, structs, sh.place(), n_pairs, expect_accuracy, log_partition, bpp,
                                    bpp ? sh.out_offsets.data() : nullptr);
  });
}

// rnamc_bpp_batch_sparse over the pool: the same shards, each through its own context; counts, starts,
// paired probabilities and log partitions go straight into the caller's arrays, and every group of
// every shard claims its part of the three list arrays from one cursor, so nothing is gathered.
int rnamc_bpp_batch_sparse_multi(rnamc_pool* p, uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
                                 const char* constraints, uint32_t max_bp_span, int uses_contra_model,
                                 int allows_short_hairpins, float min_prob, uint64_t* pair_start,
                                 uint64_t* pair_count, uint32_t* pair_i, uint32_t* pair_j, float* pair_prob,
                                 uint64_t pairs_cap, uint64_t* pairs_total, float* paired_prob,
                                 float* log_partition) {
  const char* who = "rnamc_bpp_batch_sparse_multi";
  if (!p) return RNAMC_ERR_INVALID_ARG;
  if (int rc = bpp_batch_sparse_check(n_seqs, bases, offsets, min_prob, pair_start, pair_count, pair_i, pair_j,
                                      pair_prob, pairs_total))
    return rc;
  *pairs_total = 0;
  if (n_seqs == 0) return RNAMC_OK;
  if (int rc = check_constraints(n_seqs, offsets, constraints)) return rc;
  if (p->ctxs.empty()) return RNAMC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(p->mu);
  RecordShards rs;
  if (int rc = rs.build(who, n_seqs, bases, offsets, constraints, p->size())) return rc;
  std::atomic<uint64_t> cursor{0};
  if (int rc = run_shards(who, static_cast<uint32_t>(rs.shards.size()), [&](uint32_t k) {
        const RecordShards::Shard& sh = rs.shards[k];
        return bpp_batch_sparse_core(p->ctxs[k], sh.count(), sh.bases.data(), sh.offsets.data(), sh.constraints(),
                                     max_bp_span, uses_contra_model, allows_short_hairpins, min_prob, sh.place(),
                                     pair_start, pair_count, pair_i, pair_j, pair_prob, pairs_cap, &cursor,
                                     paired_prob, log_partition);
      }))
    return rc;
  return bpp_batch_sparse_finish(cursor.load(), pair_i != nullptr, pairs_cap, pairs_total);
}

// rnamc_context_profile_batch over the pool: the same shards, each through its own context; profiles
// and log partitions go straight into the caller's arrays.
int rnamc_context_profile_batch_multi(rnamc_pool* p, uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
                                      const char* constraints, uint32_t max_bp_span, int uses_contra_model,
                                      int allows_short_hairpins, float* profile, float* log_partition) {
  const char* who = "rnamc_context_profile_batch_multi";
  if (!p) return RNAMC_ERR_INVALID_ARG;
  if (int rc = context_profile_check(n_seqs, bases, offsets, profile)) return rc;
  if (n_seqs == 0) return RNAMC_OK;
  if (int rc = check_constraints(n_seqs, offsets, constraints)) return rc;
  if (p->ctxs.empty()) return RNAMC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(p->mu);
  RecordShards rs;
  if (int rc = rs.build(who, n_seqs, bases, offsets, constraints, p->size())) return rc;
  return run_shards(who, static_cast<uint32_t>(rs.shards.size()), [&](uint32_t k) {
    const RecordShards::Shard& sh = rs.shards[k];
    return context_profile_core(p->ctxs[k], sh.count(), sh.bases.data(), sh.offsets.data(), sh.constraints(),
                                max_bp_span, uses_contra_model, allows_short_hairpins, sh.place(), profile,
                                log_partition);
  });
}

// rnamc_bpp_windowed over the pool: the window list cut into shards (equal windows: contiguous bands of
// equal size), each context accumulating its shard into its own integer sums and counters; these are added
// on the host — integer adds, any order — and the pool's first context finalises the totals: the bits of
// the single-context entry.
int rnamc_bpp_windowed_multi(rnamc_pool* p, const uint8_t* bases, uint64_t n, const char* constraint,
                             uint32_t window, uint32_t stride, uint32_t max_bp_span, int uses_contra_model,
                             int allows_short_hairpins, float* band_prob, float* paired_prob,
                             float* window_log_partition) {
  const char* who = "rnamc_bpp_windowed_multi";
  if (!p) return RNAMC_ERR_INVALID_ARG;
  WindowPlan wp;
  if (int rc = bpp_windowed_check(bases, n, constraint, window, stride, max_bp_span, band_prob, &wp)) return rc;
  if (p->ctxs.empty()) return RNAMC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(p->mu);
  std::vector<ListBand> bands;
  ShardSums sums;
  // (n < 2^31: the number of windows fits)
  if (int rc = list_shards(who, static_cast<uint32_t>(wp.n_windows), wp.w, p->size(), &bands)) return rc;
  const uint32_t n_shards = static_cast<uint32_t>(bands.size());
  if (int rc = sums.init(who, n_shards, static_cast<uint64_t>(wp.band) * wp.n)) return rc;
  if (int rc = run_shards(who, n_shards, [&](uint32_t k) {
        rnamc_ctx* c = p->ctxs[k];
        return on_ctx(c, [&] {
          const int rc = bpp_windowed_accumulate(c, wp, bases, constraint, bands[k].first, bands[k].count,
                                                 uses_contra_model, allows_short_hairpins, window_log_partition);
          return rc || n_shards == 1 ? rc : bpp_windowed_fetch(c, wp, sums.sum_of(k), sums.cnt_of(k));
        });
      }))
    return rc;
  sums.reduce();
  rnamc_ctx* c = p->ctxs[0];
  return on_ctx(c, [&] { return bpp_windowed_finish(c, wp, sums.total_sum(), sums.total_cnt(), band_prob, paired_prob); });
}

// rnamc_bpp_alignment over the pool: the rows cut into shards by the plan of rnamc_shard_plan over their
// ungapped lengths, each context accumulating its shard into its own integer sums and counters; these
// are added on the host — integer adds, any order — and the pool's first context averages the totals
// and folds them: the bits of the single-context entry.
int rnamc_bpp_alignment_multi(rnamc_pool* p, uint32_t n_rows, uint32_t n_cols, const uint8_t* rows,
                              uint32_t max_bp_span, int uses_contra_model, int allows_short_hairpins,
                              const float* centroid_thresholds, uint32_t n_thresholds, float* bpp,
                              float* col_paired, uint8_t* structs, uint32_t* n_pairs, float* expect_accuracy,
                              float* log_partition, uint32_t* row_len) {
  const char* who = "rnamc_bpp_alignment_multi";
  if (!p) return RNAMC_ERR_INVALID_ARG;
  AlignRows all;
  if (int rc = bpp_alignment_check(n_rows, n_cols, rows, centroid_thresholds, n_thresholds, structs, n_pairs,
                                   expect_accuracy, &all))
    return rc;
  if (p->ctxs.empty()) return RNAMC_ERR_INVALID_ARG;
  if (row_len)
    for (uint32_t s = 0; s < n_rows; s++) row_len[s] = static_cast<uint32_t>(all.offsets[s + 1] - all.offsets[s]);
  std::lock_guard<std::mutex> lock(p->mu);
  const uint32_t n_shards = std::min(p->size(), n_rows);
  std::vector<AlignRows> parts;  // the rows of every shard, longest first (one shard: `all` as it is)
  ShardSums sums;
  if (int rc = sums.init(who, n_shards, rnamc_bpp_len(n_cols))) return rc;
  try {  // nothing may throw across the C boundary
    if (n_shards > 1) {
      std::vector<uint32_t> shard_of(n_rows), order;
      plan(n_rows, all.offsets.data(), n_shards, shard_of.data(), &order);
      parts.resize(n_shards);
      for (AlignRows& r : parts) {
        r.n_cols = n_cols;
        r.offsets.assign(1, 0);
      }
      for (uint32_t x = 0; x < n_rows; x++) {
        const uint32_t s = order[x];
        AlignRows& r = parts[shard_of[s]];
        r.bases.insert(r.bases.end(), all.bases.begin() + all.offsets[s], all.bases.begin() + all.offsets[s + 1]);
        r.maps.insert(r.maps.end(), all.maps.begin() + all.offsets[s], all.maps.begin() + all.offsets[s + 1]);
        r.offsets.push_back(r.bases.size());
        r.row_idx.push_back(s);
      }
    }
  } catch (const std::exception&) {
    return no_host_memory(who);
  }
  if (int rc = run_shards(who, n_shards, [&](uint32_t k) {
        rnamc_ctx* c = p->ctxs[k];
        return on_ctx(c, [&] {
          const int rc = bpp_alignment_accumulate(c, n_shards > 1 ? parts[k] : all, max_bp_span, uses_contra_model,
                                                  allows_short_hairpins, log_partition);
          return rc || n_shards == 1 ? rc : bpp_alignment_fetch(c, n_cols, sums.sum_of(k), sums.cnt_of(k));
        });
      }))
    return rc;
  sums.reduce();
  rnamc_ctx* c = p->ctxs[0];
  return on_ctx(c, [&] {
    return bpp_alignment_finish(c, n_rows, n_cols, sums.total_sum(), sums.total_cnt(), centroid_thresholds,
                                n_thresholds, bpp, col_paired, structs, n_pairs, expect_accuracy);
  });
}

// rnamc_mutant_scan over the pool: the mutant list cut into shards (equal records: contiguous bands of
// equal size); every context folds the wild type itself and scans its shard straight into the caller's
// arrays.  Per-mutant integers, nothing summed across devices: the bits of the single-context entry.
int rnamc_mutant_scan_multi(rnamc_pool* p, const uint8_t* bases, uint32_t n, const char* constraint,
                            uint32_t max_bp_span, int uses_contra_model, int allows_short_hairpins,
                            const uint32_t* positions, uint32_t n_positions, float* log_partition,
                            int64_t* pair_dist2_q, float* max_dp, uint32_t* max_i, uint32_t* max_j,
                            float* paired_prob, float* wt_log_partition, float* wt_paired_prob) {
  const char* who = "rnamc_mutant_scan_multi";
  if (!p) return RNAMC_ERR_INVALID_ARG;
  uint64_t total = 0;
  if (int rc = mutant_scan_check(bases, n, constraint, positions, n_positions, log_partition, &total)) return rc;
  if (p->ctxs.empty()) return RNAMC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(p->mu);
  std::vector<ListBand> bands;  // (an empty list: one empty band, whose context folds the wild type)
  // (the number of mutants is below 2^32: checked)
  if (int rc = list_shards(who, static_cast<uint32_t>(total), n, p->size(), &bands)) return rc;
  return run_shards(who, static_cast<uint32_t>(bands.size()), [&](uint32_t k) {
    rnamc_ctx* c = p->ctxs[k];
    // (the wild type's outputs come from the first shard alone: every context computes the same bits)
    return on_ctx(c, [&] {
      return mutant_scan_core(c, bases, n, constraint, max_bp_span, uses_contra_model, allows_short_hairpins,
                              positions, bands[k].first, bands[k].count, log_partition, pair_dist2_q, max_dp, max_i,
                              max_j, paired_prob, k == 0 ? wt_log_partition : nullptr,
                              k == 0 ? wt_paired_prob : nullptr);
    });
  });
}

// The pair list is cut into contiguous bands of equal total cost nA * nB (a pair's sweeps visit every
// cell a fixed number of times): cut k lies at the first pair where the running cost reaches
// k / n_shards of the total, no band empty while there are pairs to give.  Every context uploads the
// records its band names and writes its pairs straight into the caller's arrays; every output of a
// pair is a function of the pair alone: the bits of the single-context entry.
int rnamc_duplex_batch_multi(rnamc_pool* p, uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
                             uint32_t n_pairs, const uint32_t* pair_a, const uint32_t* pair_b,
                             int uses_contra_model, float* match_probs, const uint64_t* out_offsets,
                             float* bound_a, float* bound_b, const uint64_t* bound_offsets, float* log_partition,
                             uint8_t* structs, const uint64_t* struct_offsets, float* best_scores) {
  const char* who = "rnamc_duplex_batch_multi";
  if (!p) return RNAMC_ERR_INVALID_ARG;
  if (int rc = duplex_batch_check(n_seqs, bases, offsets, n_pairs, pair_a, pair_b, match_probs, out_offsets,
                                  bound_a, bound_b, bound_offsets, structs, struct_offsets))
    return rc;
  if (p->ctxs.empty()) return RNAMC_ERR_INVALID_ARG;
  if (n_pairs == 0) return RNAMC_OK;
  std::lock_guard<std::mutex> lock(p->mu);
  const uint32_t n_shards = std::min(p->size(), n_pairs);
  std::vector<ListBand> bands;
  try {  // nothing may throw across the C boundary
    std::vector<double> csum(n_pairs);
    double run = 0.0;
    for (uint32_t x = 0; x < n_pairs; x++) {
      run += static_cast<double>(offsets[pair_a[x] + 1] - offsets[pair_a[x]]) *
             static_cast<double>(offsets[pair_b[x] + 1] - offsets[pair_b[x]]);
      csum[x] = run;
    }
    bands.assign(n_shards, ListBand());
    uint32_t lo = 0;
    for (uint32_t k = 0; k < n_shards; k++) {
      uint32_t hi = n_pairs;
      if (k + 1 < n_shards) {
        hi = static_cast<uint32_t>(std::lower_bound(csum.begin(), csum.end(), run * (k + 1.0) / n_shards) -
                                   csum.begin());
        hi = std::min(std::max(hi, lo + 1u), n_pairs - (n_shards - 1u - k));
      }
      bands[k].first = lo;
      bands[k].count = hi - lo;
      lo = hi;
    }
  } catch (const std::exception&) {
    return no_host_memory(who);
  }
  return run_shards(who, n_shards, [&](uint32_t k) {
    return duplex_batch_core(p->ctxs[k], bases, offsets, static_cast<uint32_t>(bands[k].first),
                             static_cast<uint32_t>(bands[k].count), pair_a, pair_b, uses_contra_model, match_probs,
                             out_offsets, bound_a, bound_b, bound_offsets, log_partition, structs, struct_offsets,
                             best_scores);
  });
}

}  // extern "C"
