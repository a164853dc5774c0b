// rnamc_entries_sparse.cpp — rnamc_bpp_batch_sparse: the bpp sweep group by group, and per group
// the compaction of its device-resident triangles into thresholded pair lists and per-base paired
// probabilities (rnamc_sparse.hip).
#include "rnamc_entries.h"

using namespace rnamc;

namespace rnamc {

// argument checks shared by rnamc_bpp_batch_sparse and rnamc_bpp_batch_sparse_multi: nothing of the
// context or pool is read before they pass
int bpp_batch_sparse_check(uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets, float min_prob,
                           const uint64_t* pair_start, const uint64_t* pair_count, const uint32_t* pair_i,
                           const uint32_t* pair_j, const float* pair_prob, const uint64_t* pairs_total) {
  if (!offsets || !pairs_total || (n_seqs && !bases)) return RNAMC_ERR_INVALID_ARG;
  if (!std::isfinite(min_prob) || min_prob < 0.f) {
    set_last_error("rnamc_bpp_batch_sparse: min_prob must be finite and >= 0");
    return RNAMC_ERR_INVALID_ARG;
  }
  const int given = (pair_i != nullptr) + (pair_j != nullptr) + (pair_prob != nullptr);
  if (given != 0 && given != 3) {
    set_last_error("rnamc_bpp_batch_sparse: pair_i, pair_j and pair_prob go together");
    return RNAMC_ERR_INVALID_ARG;
  }
  if (given == 3 && n_seqs && (!pair_start || !pair_count)) return RNAMC_ERR_INVALID_ARG;
  return check_records(n_seqs, bases, offsets);
}

// rnamc_bpp_batch_sparse behind both of its entries.  Sequence s writes its count (and start) at
// index place.idx(s), its log partition there too, its paired probabilities at paired_prob +
// place.base(s); a group claims its part of the caller's three arrays from `cursor`, which the shards
// of a pool share.  A group that does not fit (or a counting call) is counted only; the cursor ends
// at the total either way and the entry compares it with pairs_cap.
int bpp_batch_sparse_core(rnamc_ctx* c, uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
                          const char* constraints, uint32_t max_bp_span, int uses_contra_model,
                          int allows_short_hairpins, float min_prob, const Place& place, uint64_t* pair_start,
                          uint64_t* pair_count, uint32_t* pair_i, uint32_t* pair_j, float* pair_prob,
                          uint64_t pairs_cap, std::atomic<uint64_t>* cursor, float* paired_prob,
                          float* log_partition) {
  ConsCall cons;
  if (int rc = cons.prepare(n_seqs, offsets, constraints, max_bp_span)) return rc;
  StagedCall sc(c, false);
  if (int rc = sc.stage(c, "rnamc_bpp_batch_sparse", n_seqs, bases, offsets, cons)) return rc;
  std::vector<SparseItem> items;
  std::vector<uint32_t> h_totals;
  std::vector<float> h_paired, h_logz;
  try {  // nothing may throw across the C boundary
    h_logz.resize(n_seqs);
  } catch (const std::exception&) {
    set_last_error("rnamc_bpp_batch_sparse: no host memory");
    return RNAMC_ERR_OOM;
  }
  hipStream_t st = c->own_stream;  // (a call with hooks never takes the two-stream route of the tree order)
  uint64_t launches = 0;  // (run_batch* resets the context's statistics when it starts)
  GroupHooks hooks;
  // (the group's triangles stay on the device, at group-local offsets)
  hooks.before = [&](size_t g, float** out_base) -> int { return group_triangles(c, g, out_base); };
  hooks.after = [&](size_t, uint32_t first, uint32_t count) -> int {
    // the group's sweep and finalize kernel are enqueued on `st`: its DP workspace is dead, the
    // block counts of the group's records live there
    uint64_t n_blocks = 0, nt = 0;
    try {
      items.clear();
      for (uint32_t x = first; x < first + count; x++) {
        const SeqDesc& sd = c->descs[x];
        SparseItem it{};
        it.bpp_off = sd.out_off;
        it.blk_off = n_blocks;
        it.pp_off = nt;
        it.n = sd.n;
        it.n_blocks = static_cast<uint32_t>((rnamc_bpp_len(sd.n) + 255ull) / 256ull);
        items.push_back(it);
        n_blocks += it.n_blocks;
        nt += sd.n;
      }
      h_totals.resize(count);
      if (paired_prob) h_paired.resize(nt);
    } catch (const std::exception&) {
      set_last_error("rnamc_bpp_batch_sparse: no host memory for a group");
      return RNAMC_ERR_OOM;
    }
    if (n_blocks > c->ws_floats) {  // (a record's DP state is a multiple of its triangle: never)
      set_last_error("rnamc_bpp_batch_sparse: the workspace cannot hold the block counts");
      return RNAMC_ERR_HIP;
    }
    uint32_t* d_blocks = reinterpret_cast<uint32_t*>(c->d_ws.get());
    HIPCHK(c->sp_totals.grow(count));
    HIPCHK(c->sp_items.upload(items.data(), count, st));
    // records longest first: the first item of a launch has the most blocks
    for (uint32_t x = 0; x < count; x += 65535u) {
      launch_sparse_count(c->sp_items + x, std::min(count - x, 65535u), items[x].n_blocks, c->st_out[0], d_blocks,
                          min_prob, st);
      launches++;
    }
    launch_sparse_scan(c->sp_items, count, d_blocks, c->sp_totals, st);
    launches++;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_totals.data(), c->sp_totals, count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    uint64_t group_total = 0;
    for (uint32_t x = 0; x < count; x++) {
      items[x].out_off = group_total;
      group_total += h_totals[x];
    }
    const uint64_t start = cursor->fetch_add(group_total);
    const bool fill = pair_i != nullptr && start + group_total <= pairs_cap;
    for (uint32_t x = 0; x < count; x++) {
      const uint32_t r = place.idx(c->descs[first + x].batch_idx);
      if (pair_count) pair_count[r] = h_totals[x];
      if (fill) pair_start[r] = start + items[x].out_off;
    }
    if (fill && group_total) {
      HIPCHK(c->sp_i.grow(group_total));
      HIPCHK(c->sp_j.grow(group_total));
      HIPCHK(c->sp_p.grow(group_total));
      HIPCHK(hipMemcpyAsync(c->sp_items, items.data(), count * sizeof(SparseItem), hipMemcpyHostToDevice, st));
      for (uint32_t x = 0; x < count; x += 65535u) {
        launch_sparse_fill(c->sp_items + x, std::min(count - x, 65535u), items[x].n_blocks, c->st_out[0], d_blocks,
                           min_prob, c->sp_i, c->sp_j, c->sp_p, st);
        launches++;
      }
      HIPCHK(hipGetLastError());
      // the group's lists are contiguous in the caller's arrays: one copy per array
      HIPCHK(hipMemcpyAsync(pair_i + start, c->sp_i, group_total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(pair_j + start, c->sp_j, group_total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(pair_prob + start, c->sp_p, group_total * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    if (paired_prob) {
      HIPCHK(c->sp_paired.grow(nt));
      for (uint32_t x = 0; x < count; x += 65535u) {
        launch_sparse_paired(c->sp_items + x, std::min(count - x, 65535u), items[x].n, c->st_out[0], c->sp_paired,
                             st);
        launches++;
      }
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(h_paired.data(), c->sp_paired, nt * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    // (the next group's sweep reuses the workspace and the triangles: everything above is done first)
    HIPCHK(hipStreamSynchronize(st));
    if (paired_prob)
      for (uint32_t x = 0; x < count; x++) {
        const SeqDesc& sd = c->descs[first + x];
        std::memcpy(paired_prob + place.base(sd.batch_idx, offsets), h_paired.data() + items[x].pp_off,
                    sd.n * sizeof(float));
      }
    return RNAMC_OK;
  };
  int rc = run_batch_mode(c, n_seqs, c->st_bases, sc.doff.data(), uses_contra_model != 0,
                          allows_short_hairpins != 0, nullptr, nullptr, c->st_logz, st, sc.opts, &hooks);
  c->stats.launches_other += launches;
  rc = sc.finish(c, rc, n_seqs, log_partition ? h_logz.data() : nullptr);
  if (rc) return rc;
  if (log_partition)
    for (uint32_t s = 0; s < n_seqs; s++) log_partition[place.idx(s)] = h_logz[s];
  return RNAMC_OK;
}

// the end both entries share: the total, and the status of a call whose arrays were too small
int bpp_batch_sparse_finish(uint64_t total, bool wants_lists, uint64_t pairs_cap, uint64_t* pairs_total) {
  *pairs_total = total;
  if (wants_lists && total > pairs_cap) {
    set_last_error("rnamc_bpp_batch_sparse: " + std::to_string(total) + " pairs, pairs_cap " +
                   std::to_string(pairs_cap));
    return RNAMC_ERR_INVALID_ARG;
  }
  return RNAMC_OK;
}

}  // namespace rnamc

extern "C" {

int rnamc_bpp_batch_sparse(rnamc_ctx* c, uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
                           const char* constraints, uint32_t max_bp_span, int uses_contra_model,
                           int allows_short_hairpins, float min_prob, uint64_t* pair_start, uint64_t* pair_count,
                           uint32_t* pair_i, uint32_t* pair_j, float* pair_prob, uint64_t pairs_cap,
                           uint64_t* pairs_total, float* paired_prob, float* log_partition) {
  if (!c) return RNAMC_ERR_INVALID_ARG;
  if (int rc = bpp_batch_sparse_check(n_seqs, bases, offsets, min_prob, pair_start, pair_count, pair_i, pair_j,
                                      pair_prob, pairs_total))
    return rc;
  *pairs_total = 0;
  if (n_seqs == 0) return RNAMC_OK;
  std::atomic<uint64_t> cursor{0};
  if (int rc = bpp_batch_sparse_core(c, n_seqs, bases, offsets, constraints, max_bp_span, uses_contra_model,
                                     allows_short_hairpins, min_prob, Place(), pair_start, pair_count, pair_i,
                                     pair_j, pair_prob, pairs_cap, &cursor, paired_prob, log_partition))
    return rc;
  return bpp_batch_sparse_finish(cursor.load(), pair_i != nullptr, pairs_cap, pairs_total);
}

}  // extern "C"
