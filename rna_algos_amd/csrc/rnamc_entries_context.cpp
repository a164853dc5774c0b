// rnamc_entries_context.cpp — rnamc_context_profile_batch: the reference-order sweep group by group,
// sums_multibranch copied aside between a group's two sweeps, and behind its finalize kernel the
// per-base loop-type probabilities off the group's workspace (rnamc_context.hip).
#include "rnamc_entries.h"

using namespace rnamc;

namespace rnamc {

// argument checks shared by rnamc_context_profile_batch and rnamc_context_profile_batch_multi: nothing
// of the context or pool is read before they pass
int context_profile_check(uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets, const float* profile) {
  if (!offsets || (n_seqs && (!bases || !profile))) return RNAMC_ERR_INVALID_ARG;
  return check_records(n_seqs, bases, offsets);
}

// rnamc_context_profile_batch behind both of its entries.  Sequence s writes its six rows at
// profile + CTX_ROWS * place.base(s) and its log partition at index place.idx(s).
int context_profile_core(rnamc_ctx* c, uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
                         const char* constraints, uint32_t max_bp_span, int uses_contra_model,
                         int allows_short_hairpins, const Place& place, float* profile, float* log_partition) {
  ConsCall cons;
  if (int rc = cons.prepare(n_seqs, offsets, constraints, max_bp_span)) return rc;
  StagedCall sc(c, false);
  if (int rc = sc.stage(c, "rnamc_context_profile_batch", n_seqs, bases, offsets, cons)) return rc;
  std::vector<ContextItem> items;
  std::vector<SparseItem> pitems;
  std::vector<float> h_prof, h_logz;
  try {  // nothing may throw across the C boundary
    h_logz.resize(n_seqs);
  } catch (const std::exception&) {
    set_last_error("rnamc_context_profile_batch: no host memory");
    return RNAMC_ERR_OOM;
  }
  hipStream_t st = c->own_stream;
  const bool prof = c->profile != 0, contra = uses_contra_model != 0;
  uint64_t launches = 0;  // (run_batch resets the context's statistics when it starts)
  size_t ev_pairs = 0;
  uint64_t acc_words = 0, nt = 0;
  auto batch_of = [&](uint32_t first, uint32_t x) {
    ContextBatch b{};
    b.seqs = c->d_seqs + first + x;
    b.items = c->cx_items + x;
    b.bases = c->st_bases;
    b.workspace = c->d_ws;
    b.bpp = c->st_out[0];
    b.params = c->d_params;
    b.hp_init = c->d_hp_init;
    b.qm = c->cx_qm;
    b.acc = c->cx_acc;
    b.out = c->cx_out;
    return b;
  };
  GroupHooks hooks;
  // (the group's triangles stay on the device, at group-local offsets)
  hooks.before = [&](size_t g, float** out_base) -> int {
    if (g == 0 && prof) HIPCHK(c->cx_events.pairs(c->group_begin.size() - 1));
    return group_triangles(c, g, out_base);
  };
  hooks.mid = [&](size_t, uint32_t first, uint32_t count) -> int {
    // the group's inside sweep is enqueued on `st`: sums_multibranch is whole and its slot not yet
    // reused.  The group before is drained (its after-hook), so the buffers may grow.
    uint64_t qm_floats = 0;
    acc_words = nt = 0;
    try {
      items.clear();
      for (uint32_t x = first; x < first + count; x++) {
        const SeqDesc& sd = c->descs[x];
        ContextItem it{};
        it.qm_off = qm_floats;
        it.acc_off = acc_words;
        it.out_off = static_cast<uint64_t>(CTX_ROWS) * nt;
        items.push_back(it);
        qm_floats += sd.tri_pad;
        acc_words += static_cast<uint64_t>(CTX_ACC_ROWS) * (sd.n + 1ull);
        nt += sd.n;
      }
    } catch (const std::exception&) {
      set_last_error("rnamc_context_profile_batch: no host memory for a group");
      return RNAMC_ERR_OOM;
    }
    HIPCHK(c->cx_qm.grow(qm_floats));
    HIPCHK(c->cx_items.upload(items.data(), count, st));
    // records longest first: the first item of a launch is its longest
    for (uint32_t x = 0; x < count; x += 65535u) {
      launch_context_save(batch_of(first, x), std::min(count - x, 65535u), c->descs[first + x].n, st);
      launches++;
    }
    HIPCHK(hipGetLastError());
    return RNAMC_OK;
  };
  hooks.after = [&](size_t g, uint32_t first, uint32_t count) -> int {
    // the group's sweep and finalize kernel are enqueued on `st`: the workspace holds what the
    // outside sweep left, st_out[0] the group's triangles
    try {
      pitems.clear();
      for (uint32_t x = 0; x < count; x++) {
        const SeqDesc& sd = c->descs[first + x];
        SparseItem it{};
        it.bpp_off = sd.out_off;
        it.pp_off = items[x].out_off + static_cast<uint64_t>(CTX_ROW_STEM) * sd.n;  // row 5 in place
        it.n = sd.n;
        pitems.push_back(it);
      }
      h_prof.resize(static_cast<uint64_t>(CTX_ROWS) * nt);
    } catch (const std::exception&) {
      set_last_error("rnamc_context_profile_batch: no host memory for a group");
      return RNAMC_ERR_OOM;
    }
    HIPCHK(c->cx_acc.grow(acc_words));
    HIPCHK(c->cx_out.grow(static_cast<uint64_t>(CTX_ROWS) * nt));
    HIPCHK(c->sp_items.upload(pitems.data(), count, st));
    if (prof) HIPCHK(hipEventRecord(c->cx_events[2 * g], st));
    HIPCHK(hipMemsetAsync(c->cx_acc, 0, acc_words * sizeof(unsigned long long), st));
    for (uint32_t x = 0; x < count; x += 65535u) {
      const uint32_t k = std::min(count - x, 65535u), max_n = c->descs[first + x].n;
      launches += launch_context_profile(batch_of(first, x), contra, k, max_n, st);
      // row 5 by the kernel of rnamc_bpp_batch_sparse's paired_prob: the same bits
      launch_sparse_paired(c->sp_items + x, k, max_n, c->st_out[0], c->cx_out, st);
      launches++;
    }
    HIPCHK(hipGetLastError());
    if (prof) {
      HIPCHK(hipEventRecord(c->cx_events[2 * g + 1], st));
      ev_pairs = g + 1;
    }
    HIPCHK(hipMemcpyAsync(h_prof.data(), c->cx_out, h_prof.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    // (the next group's sweep reuses the workspace and the triangles: everything above is done first)
    HIPCHK(hipStreamSynchronize(st));
    for (uint32_t x = 0; x < count; x++) {
      const SeqDesc& sd = c->descs[first + x];
      std::memcpy(profile + static_cast<uint64_t>(CTX_ROWS) * place.base(sd.batch_idx, offsets),
                  h_prof.data() + items[x].out_off,
                  static_cast<uint64_t>(CTX_ROWS) * sd.n * sizeof(float));
    }
    return RNAMC_OK;
  };
  // the reference-order sweep whatever summation_mode says: the kernels read its workspace layout
  int rc = run_batch(c, n_seqs, c->st_bases, sc.doff.data(), contra, allows_short_hairpins != 0, nullptr, nullptr,
                     c->st_logz, st, sc.opts, &hooks);
  c->stats.launches_other += launches;
  c->cx_launches = launches;
  c->cx_ms = 0.0;
  if (rc == RNAMC_OK && prof) {
    if (hipError_t e = c->cx_events.pairs_ms(ev_pairs, &c->cx_ms)) {
      set_last_error(std::string("rnamc_context_profile_batch: ") + hipGetErrorString(e));
      rc = RNAMC_ERR_HIP;
    }
  }
  rc = sc.finish(c, rc, n_seqs, log_partition ? h_logz.data() : nullptr);
  if (rc) return rc;
  if (log_partition)
    for (uint32_t s = 0; s < n_seqs; s++) log_partition[place.idx(s)] = h_logz[s];
  return RNAMC_OK;
}

}  // namespace rnamc

extern "C" {

int rnamc_context_profile_batch(rnamc_ctx* c, uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
                                const char* constraints, uint32_t max_bp_span, int uses_contra_model,
                                int allows_short_hairpins, float* profile, float* log_partition) {
  if (!c) return RNAMC_ERR_INVALID_ARG;
  if (int rc = context_profile_check(n_seqs, bases, offsets, profile)) return rc;
  if (n_seqs == 0) return RNAMC_OK;
  return context_profile_core(c, n_seqs, bases, offsets, constraints, max_bp_span, uses_contra_model,
                              allows_short_hairpins, Place(), profile, log_partition);
}

int rnamc_context_profile_stats(rnamc_ctx* c, uint64_t* launches_context, double* ms_context) {
  if (!c || !launches_context || !ms_context) return RNAMC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(c->mu);
  *launches_context = c->cx_launches;
  *ms_context = c->cx_ms;
  return RNAMC_OK;
}

}  // extern "C"
