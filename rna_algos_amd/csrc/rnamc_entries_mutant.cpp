// rnamc_entries_mutant.cpp — rnamc_mutant_plan and rnamc_mutant_scan: the wild type of one sequence
// folded once and its triangle parked on the device, then every single-base mutant through the bpp
// sweep chunk by chunk and group by group, and per group the comparison of its device-resident
// triangles with the wild type's (rnamc_mutant.hip).
#include "rnamc_entries.h"

using namespace rnamc;

namespace rnamc {

int mutant_scan_check(const uint8_t* bases, uint32_t n, const char* constraint, const uint32_t* positions,
                      uint32_t n_positions, const float* log_partition, uint64_t* n_mutants) {
  if (!bases || !log_partition) return RNAMC_ERR_INVALID_ARG;
  if (n == 0) return RNAMC_ERR_EMPTY_SEQ;
  if (n > RNAMC_MAX_SEQ_LEN) return RNAMC_ERR_SEQ_TOO_LONG;
  for (uint32_t x = 0; x < n; x++)
    if (bases[x] > 3) return RNAMC_ERR_INVALID_BASE;
  const uint64_t n_pos = positions ? n_positions : n;
  if (3ull * n_pos >= (1ull << 32)) {
    set_last_error("rnamc_mutant_scan: 3 * n_positions must be below 2^32");
    return RNAMC_ERR_INVALID_ARG;
  }
  if (positions)
    for (uint64_t k = 0; k < n_pos; k++)
      if (positions[k] >= n) {
        set_last_error("rnamc_mutant_scan: positions[" + std::to_string(k) + "] = " + std::to_string(positions[k]) +
                       " is outside the sequence of " + std::to_string(n) + " bases");
        return RNAMC_ERR_INVALID_ARG;
      }
  if (constraint) {
    uint32_t bad = 0;
    const char* why = "";
    int rc = RNAMC_OK;
    try {  // nothing may throw across the C boundary
      std::vector<int32_t> words(2ull * n);
      rc = compile_constraint(constraint, n, words.data(), &bad, &why);
    } catch (const std::exception&) {
      set_last_error("rnamc_mutant_scan: no host memory");
      return RNAMC_ERR_OOM;
    }
    if (rc) {
      set_last_error("rnamc_mutant_scan: constraint position " + std::to_string(bad) + ": " + why);
      return rc;
    }
  }
  *n_mutants = 3ull * n_pos;
  return RNAMC_OK;
}

namespace {

// pair (i, j) of packed cell c: the largest d with tri_off(d) <= c, by bisection in integers
void cell_pair(uint32_t n, uint64_t c, uint32_t* i, uint32_t* j) {
  auto tri_off = [n](uint64_t d) { return d * n - ((d * (d - 1ull)) >> 1); };
  uint32_t lo = 0u, hi = n - 1u;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (tri_off(mid) <= c) lo = mid; else hi = mid - 1u;
  }
  *i = static_cast<uint32_t>(c - tri_off(lo));
  *j = *i + lo;
}

// one record's descriptor for k_sparse_paired: its triangle and where its n sums go
SparseItem paired_item(uint64_t bpp_off, uint64_t pp_off, uint32_t n) {
  SparseItem it{};
  it.bpp_off = bpp_off;
  it.pp_off = pp_off;
  it.n = n;
  it.n_blocks = static_cast<uint32_t>((rnamc_bpp_len(n) + 255ull) / 256ull);
  return it;
}

}  // namespace

int mutant_scan_core(rnamc_ctx* c, const uint8_t* bases, uint32_t n, const char* constraint, uint32_t max_bp_span,
                     int uses_contra_model, int allows_short_hairpins, const uint32_t* positions, uint64_t first,
                     uint64_t count, float* log_partition, int64_t* pair_dist2_q, float* max_dp, uint32_t* max_i,
                     uint32_t* max_j, float* paired_prob, float* wt_log_partition, float* wt_paired_prob) {
  hipStream_t st = c->own_stream;  // (a call with hooks never takes the two-stream route of the tree order)
  const uint64_t len = rnamc_bpp_len(n);
  const bool prof = c->profile != 0;
  const bool wants_paired = paired_prob != nullptr && count != 0;
  rnamc_batch_stats total{};

  // ---- the wild type: a call of one record, its triangle parked where no later group writes ----
  {
    const uint64_t offs[2] = {0, n};
    ConsCall cons;
    if (int rc = cons.prepare(1, offs, constraint, max_bp_span)) return rc;
    StagedCall sc(c, true);
    if (int rc = sc.stage(c, "rnamc_mutant_scan", 1, bases, offs, cons)) return rc;
    const SparseItem wt_item = paired_item(0, 0, n);  // (lives until sc.finish has drained the stream)
    uint64_t launches = 0;  // (run_batch* resets the context's statistics when it starts)
    size_t ev_pairs = 0;
    GroupHooks hooks;
    hooks.before = [&](size_t, float** out_base) -> int {
      HIPCHK(c->mt_wt.grow(len));
      *out_base = c->mt_wt;
      return RNAMC_OK;
    };
    hooks.after = [&](size_t, uint32_t, uint32_t) -> int {
      if (!wt_paired_prob) return RNAMC_OK;
      HIPCHK(c->mt_wt_paired.grow(n));
      HIPCHK(c->mt_pitems.upload(&wt_item, 1, st));
      if (prof) {
        HIPCHK(c->mt_events.pairs(1));
        HIPCHK(hipEventRecord(c->mt_events[0], st));
      }
      launch_sparse_paired(c->mt_pitems, 1, n, c->mt_wt, c->mt_wt_paired, st);
      launches++;
      HIPCHK(hipGetLastError());
      if (prof) {
        HIPCHK(hipEventRecord(c->mt_events[1], st));
        ev_pairs = 1;
      }
      HIPCHK(hipMemcpyAsync(wt_paired_prob, c->mt_wt_paired, n * sizeof(float), hipMemcpyDeviceToHost, st));
      return RNAMC_OK;
    };
    int rc = run_batch_mode(c, 1, c->st_bases, sc.doff.data(), uses_contra_model != 0, allows_short_hairpins != 0,
                            nullptr, nullptr, c->st_logz, st, sc.opts, &hooks);
    rc = sc.finish(c, rc, 1, wt_log_partition);
    if (rc) return rc;
    if (int rc2 = fold_call_stats(c, &total, launches, c->mt_events, ev_pairs, &rnamc_batch_stats::launches_mutant,
                                  &rnamc_batch_stats::ms_mutant))
      return rc2;
  }
  if (count == 0) {
    c->stats = total;
    return RNAMC_OK;
  }

  // ---- the mutants ----
  HIPCHK(c->mt_sum.grow(count));
  HIPCHK(c->mt_key.grow(count));
  // once per call, not per chunk
  HIPCHK(hipMemsetAsync(c->mt_sum, 0, count * sizeof(int64_t), st));
  HIPCHK(hipMemsetAsync(c->mt_key, 0, count * sizeof(uint64_t), st));
  ChunkScan s{};
  s.who = "rnamc_mutant_scan";
  s.what = "mutants";
  s.rec_len = n;
  s.count = count;
  // mutants of a chunk: mutant_chunk_nt nucleotides, one mutant at least
  s.per_chunk = std::min<uint64_t>(std::max<uint64_t>(static_cast<uint64_t>(c->mutant_chunk_nt) / n, 1), count);
  s.with_constraint = constraint != nullptr;
  s.max_bp_span = max_bp_span;
  s.contra = uses_contra_model != 0;
  s.allows_short = allows_short_hairpins != 0;
  s.log_partition = log_partition + first;
  s.events = &c->mt_events;
  s.launches_own = &rnamc_batch_stats::launches_mutant;
  s.ms_own = &rnamc_batch_stats::ms_mutant;
  std::vector<uint64_t> h_key;
  std::vector<MutantItem> items;  // (the host copies live until the chunk's stream is drained)
  std::vector<SparseItem> pitems;
  try {  // nothing may throw across the C boundary
    items.resize(s.per_chunk);
    if (wants_paired) pitems.resize(s.per_chunk);
    if (max_dp || max_i || max_j) h_key.resize(count);
  } catch (const std::exception&) {
    set_last_error("rnamc_mutant_scan: no host memory for a chunk of mutants");
    return RNAMC_ERR_OOM;
  }
  if (wants_paired) HIPCHK(c->mt_paired.grow(s.per_chunk * n));
  // a mutant as an ordinary record: the wild type with one byte changed
  s.cut = [&](uint64_t x, uint8_t* rec, char* cons) {
    const uint64_t mu = first + x, idx = mu / 3;
    const uint32_t pos = positions ? positions[idx] : static_cast<uint32_t>(idx);
    std::memcpy(rec, bases, n);
    rec[pos] = mutant_base_of(bases[pos], static_cast<uint32_t>(mu % 3));
    if (cons) std::memcpy(cons, constraint, n);
  };
  s.upload_items = [&](uint64_t x0, uint32_t m) -> int {
    for (size_t x = 0; x < c->descs.size(); x++) {
      const SeqDesc& sd = c->descs[x];
      items[x].bpp_off = sd.out_off;
      items[x].slot = x0 + sd.batch_idx;
      if (wants_paired) pitems[x] = paired_item(sd.out_off, static_cast<uint64_t>(sd.batch_idx) * n, n);
    }
    HIPCHK(c->mt_items.upload(items.data(), m, st));
    if (wants_paired) HIPCHK(c->mt_pitems.upload(pitems.data(), m, st));
    return RNAMC_OK;
  };
  s.launch = [&](uint32_t first_desc, uint32_t k) -> uint64_t {
    launch_mutant_compare(c->mt_items + first_desc, k, c->mt_wt, c->st_out[0], n, c->mt_sum, c->mt_key, st);
    if (!wants_paired) return 1;
    launch_sparse_paired(c->mt_pitems + first_desc, k, n, c->st_out[0], c->mt_paired, st);
    return 2;
  };
  if (wants_paired)
    s.after_sweep = [&](uint64_t x0, uint32_t m) -> int {
      if (hipMemcpyAsync(paired_prob + (first + x0) * n, c->mt_paired, static_cast<uint64_t>(m) * n * sizeof(float),
                         hipMemcpyDeviceToHost, st) == hipSuccess)
        return RNAMC_OK;
      set_last_error("rnamc_mutant_scan: copying a chunk's paired probabilities failed");
      (void)hipGetLastError();
      return RNAMC_ERR_HIP;
    };
  if (int rc = scan_chunks(c, s, &total)) return rc;
  c->stats = total;
  // the accumulators, after the last chunk
  if (pair_dist2_q)
    HIPCHK(hipMemcpyAsync(pair_dist2_q + first, c->mt_sum, count * sizeof(int64_t), hipMemcpyDeviceToHost, st));
  if (!h_key.empty())
    HIPCHK(hipMemcpyAsync(h_key.data(), c->mt_key, count * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  for (uint64_t x = 0; x < h_key.size(); x++) {
    const uint64_t k = h_key[x];
    float t = 0.f;
    uint32_t i = 0xffffffffu, j = 0xffffffffu;
    if (k != 0) {  // (a cell that moved has t > 0)
      const uint32_t bits = static_cast<uint32_t>(k >> 32);
      std::memcpy(&t, &bits, sizeof(t));
      cell_pair(n, 0xffffffffu - static_cast<uint32_t>(k), &i, &j);
    }
    if (max_dp) max_dp[first + x] = t;
    if (max_i) max_i[first + x] = i;
    if (max_j) max_j[first + x] = j;
  }
  return RNAMC_OK;
}

}  // namespace rnamc

extern "C" {

int rnamc_mutant_plan(const uint8_t* bases, uint32_t n, const uint32_t* positions, uint32_t n_positions,
                      uint64_t* n_mutants, uint32_t* mut_pos, uint8_t* mut_base, uint64_t cap) {
  if (!n_mutants) return RNAMC_ERR_INVALID_ARG;
  *n_mutants = 0;
  const float unused = 0.f;  // (the scan's own check wants its log_partition)
  uint64_t total = 0;
  if (int rc = mutant_scan_check(bases, n, nullptr, positions, n_positions, &unused, &total)) return rc;
  *n_mutants = total;
  if (!mut_pos && !mut_base) return RNAMC_OK;
  if (cap < total) {
    set_last_error("rnamc_mutant_plan: " + std::to_string(total) + " mutants, cap " + std::to_string(cap));
    return RNAMC_ERR_INVALID_ARG;
  }
  for (uint64_t m = 0; m < total; m++) {
    const uint32_t pos = positions ? positions[m / 3] : static_cast<uint32_t>(m / 3);
    if (mut_pos) mut_pos[m] = pos;
    if (mut_base) mut_base[m] = mutant_base_of(bases[pos], static_cast<uint32_t>(m % 3));
  }
  return RNAMC_OK;
}

int rnamc_mutant_scan(rnamc_ctx* c, const uint8_t* bases, uint32_t n, const char* constraint, uint32_t max_bp_span,
                      int uses_contra_model, int allows_short_hairpins, const uint32_t* positions,
                      uint32_t n_positions, float* log_partition, int64_t* pair_dist2_q, float* max_dp,
                      uint32_t* max_i, uint32_t* max_j, float* paired_prob, float* wt_log_partition,
                      float* wt_paired_prob) {
  if (!c) return RNAMC_ERR_INVALID_ARG;
  uint64_t total = 0;
  if (int rc = mutant_scan_check(bases, n, constraint, positions, n_positions, log_partition, &total)) return rc;
  std::unique_lock<std::mutex> lock(c->mu);
  DeviceGuard guard(c->device);
  if (!guard.ok) return RNAMC_ERR_NO_DEVICE;
  const int rc = mutant_scan_core(c, bases, n, constraint, max_bp_span, uses_contra_model, allows_short_hairpins,
                                  positions, 0, total, log_partition, pair_dist2_q, max_dp, max_i, max_j, paired_prob,
                                  wt_log_partition, wt_paired_prob);
  if (rc) (void)hipStreamSynchronize(c->own_stream);
  return rc;
}

}  // extern "C"
