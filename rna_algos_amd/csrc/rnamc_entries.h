// rnamc_entries.h — what the host-buffer entries share before and around their sweep: the record
// check, the compiled constraints of a call, the staging prologue.
#ifndef RNAMC_ENTRIES_H
#define RNAMC_ENTRIES_H

#include "rnamc_ctx.h"

namespace rnamc {

// Hard constraints of one batch call (include/rnamc.h).  prepare() validates
// and compiles every record on the host, before any device work and before the context's lock: two
// words per base, laid out like the staged bases (rnamc_scoring.h, pair_allowed).  A call with
// nothing to constrain (no string or only '.', no span limit below the longest record) is not
// active: it runs exactly the unconstrained sweep.
struct ConsCall {
  std::vector<int32_t> words;
  uint32_t max_span = 0xffffffffu;
  bool active = false;

  int prepare(uint32_t n_seqs, const uint64_t* offsets, const char* strings, uint32_t max_bp_span) {
    uint64_t max_n = 0;
    for (uint32_t s = 0; s < n_seqs; s++) max_n = std::max<uint64_t>(max_n, offsets[s + 1] - offsets[s]);
    if (max_bp_span != 0 && max_bp_span < max_n) {
      active = true;
      max_span = max_bp_span;
    }
    const uint64_t lo = offsets[0], total = offsets[n_seqs] - lo;
    if (strings)
      for (uint64_t x = 0; x < total && !active; x++) active = strings[x] != '.';
    if (!active) return RNAMC_OK;
    try {  // nothing may throw across the C boundary
      words.assign(2 * total, -1);  // (no string: every base free, outside every constraint pair)
    } catch (const std::exception&) {
      set_last_error("constraints: no host memory");
      return RNAMC_ERR_OOM;
    }
    if (!strings) return RNAMC_OK;
    for (uint32_t s = 0; s < n_seqs; s++) {
      const uint64_t off = offsets[s] - lo;
      uint32_t bad = 0;
      const char* why = "";
      int rc = RNAMC_OK;
      try {
        rc = compile_constraint(strings + off, static_cast<uint32_t>(offsets[s + 1] - offsets[s]),
                                words.data() + 2 * off, &bad, &why);
      } catch (const std::exception&) {
        set_last_error("constraints: no host memory");
        return RNAMC_ERR_OOM;
      }
      if (rc) {
        set_last_error("constraint of record " + std::to_string(s) + ", position " + std::to_string(bad) +
                       ": " + why);
        return rc;
      }
    }
    return RNAMC_OK;
  }
};

// Record checks of every host-buffer entry, before the context is touched: offsets monotone, no
// empty record, none above the length limit (decided from the offsets alone), every base 0 .. 3.
// `ends`: pseudo bases at either end of a record (rnamc_durbin_batch: 1), never scored, any value.
inline int check_records(uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets, uint32_t ends = 0) {
  for (uint32_t s = 0; s < n_seqs; s++) {
    if (offsets[s + 1] < offsets[s]) return RNAMC_ERR_INVALID_ARG;
    const uint64_t n = offsets[s + 1] - offsets[s];
    // (the reference's Durbin indexes [seq_len - 2]: a sequence is at least its two pseudo bases)
    if (n < std::max(1u, 2u * ends)) return RNAMC_ERR_EMPTY_SEQ;
    if (n > RNAMC_MAX_SEQ_LEN + 2ull * ends) return RNAMC_ERR_SEQ_TOO_LONG;
    for (uint64_t x = offsets[s] + ends; x + ends < offsets[s + 1]; x++)
      if (bases[x] > 3) return RNAMC_ERR_INVALID_BASE;
  }
  return RNAMC_OK;
}

// The prologue of a host-buffer entry whose arguments passed (everything before it runs without the
// context): the context's lock and device, the record offsets rebased to the staged bases, the
// context's earlier work finished, the bases and -- after them -- the constraint words uploaded on
// own_stream.  `opts` carries the staged constraints to the sweep.
struct StagedCall {
  std::unique_lock<std::mutex> lock;  // (none where the caller holds c->mu: rnamc_fold_scores, rnamc_fold_sums)
  DeviceGuard guard;
  std::vector<uint64_t> doff;
  SweepOpts opts;

  StagedCall(rnamc_ctx* c, bool locked)
      : lock(locked ? std::unique_lock<std::mutex>() : std::unique_lock<std::mutex>(c->mu)), guard(c->device) {}

  // Staging buffers live in the context and only grow (a caller that folds one record after
  // another, like the reference's binaries, would otherwise pay hipMalloc/hipFree per call).
  int stage(rnamc_ctx* c, const char* who, uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
            const ConsCall& cons, bool with_logz = true) {
    if (!guard.ok) return RNAMC_ERR_NO_DEVICE;
    try {  // nothing may throw across the C boundary
      doff.resize(n_seqs + 1);
    } catch (const std::exception&) {
      set_last_error(std::string(who) + ": no host memory");
      return RNAMC_ERR_OOM;
    }
    const uint64_t base_lo = offsets[0], base_hi = offsets[n_seqs];
    for (uint32_t s = 0; s <= n_seqs; s++) doff[s] = offsets[s] - base_lo;
    HIPCHK(hipStreamSynchronize(c->own_stream));
    HIPCHK(grow_device(reinterpret_cast<void**>(&c->st_bases), &c->st_bases_cap, base_hi - base_lo));
    if (with_logz)
      HIPCHK(grow_device(reinterpret_cast<void**>(&c->st_logz), &c->st_logz_cap,
                         static_cast<uint64_t>(n_seqs) * sizeof(float)));
    HIPCHK(hipMemcpyAsync(c->st_bases, bases + base_lo, base_hi - base_lo, hipMemcpyHostToDevice,
                          c->own_stream));
    if (!cons.active) return RNAMC_OK;
    HIPCHK(grow_device(reinterpret_cast<void**>(&c->st_cons), &c->st_cons_cap, cons.words.size() * sizeof(int32_t)));
    HIPCHK(hipMemcpyAsync(c->st_cons, cons.words.data(), cons.words.size() * sizeof(int32_t), hipMemcpyHostToDevice,
                          c->own_stream));
    opts.cons = c->st_cons;
    opts.max_span = cons.max_span;
    return RNAMC_OK;
  }

  // the end of the call: own_stream drained either way, the log partitions copied out after a sweep that ran
  int finish(rnamc_ctx* c, int rc, uint32_t n_seqs, float* log_partition) {
    if (rc) {
      (void)hipStreamSynchronize(c->own_stream);
      return rc;
    }
    if (log_partition)
      HIPCHK(hipMemcpyAsync(log_partition, c->st_logz, n_seqs * sizeof(float), hipMemcpyDeviceToHost,
                            c->own_stream));
    HIPCHK(hipStreamSynchronize(c->own_stream));
    return RNAMC_OK;
  }
};

// before-hook of the entries that take no triangles to the host: the finalize kernel writes the
// group's triangles somewhere, at group-local offsets -- one device buffer for all groups
inline int group_triangles(rnamc_ctx* c, size_t g, float** out_base) {
  const uint64_t need = std::max<uint64_t>(c->group_out_floats[g], 1) * sizeof(float);
  HIPCHK(grow_device(reinterpret_cast<void**>(&c->st_out[0]), &c->st_out_cap[0], need));
  *out_base = c->st_out[0];
  return RNAMC_OK;
}

// Entries that run the sweep several times in one call (chunks of windows, of mutants): the sweep's
// statistics of one staged call added to the call's (run_batch* resets the context's when it starts)
inline void add_sweep_stats(rnamc_batch_stats* to, const rnamc_batch_stats& s) {
  to->n_groups += s.n_groups;
  to->launches_inside += s.launches_inside;
  to->launches_outside += s.launches_outside;
  to->launches_other += s.launches_other;
  to->ms_inside += s.ms_inside;
  to->ms_outside += s.ms_outside;
  to->ms_other += s.ms_other;
  to->workspace_bytes = std::max(to->workspace_bytes, s.workspace_bytes);
  to->launches_outside_main += s.launches_outside_main;
  to->launches_outside_tail += s.launches_outside_tail;
  to->launches_outside_small += s.launches_outside_small;
  to->ms_outside_main += s.ms_outside_main;
  to->ms_outside_tail += s.ms_outside_tail;
  to->ms_outside_small += s.ms_outside_small;
  to->tree_side_stream = s.tree_side_stream;
}

// profiling: event pairs around an entry's own kernels (pair p = events 2p, 2p + 1 of a grow-only
// ring of the context), read once their stream is drained
inline int event_pairs(std::vector<hipEvent_t>* ring, size_t pairs) {
  while (ring->size() < 2 * pairs) {
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    ring->push_back(e);
  }
  return RNAMC_OK;
}
inline int event_pairs_ms(const std::vector<hipEvent_t>& ring, size_t pairs, double* ms) {
  for (size_t p = 0; p < pairs; p++) {
    float t = 0.f;
    HIPCHK(hipEventElapsedTime(&t, ring[2 * p], ring[2 * p + 1]));
    *ms += t;
  }
  return RNAMC_OK;
}

// Waves of a walk kernel (sampling, tracebacks), one item each while they last: enough to fill the
// chip, no more than the items, within 1 GB of stacks (the longest n + 1 pending cells per wave).
inline uint32_t waves_of(int cus, uint64_t items, uint32_t gmax) {
  uint64_t w = std::min<uint64_t>(items, static_cast<uint64_t>(std::max(cus, 1)) * 16);
  w = std::min<uint64_t>(w, std::max<uint64_t>((1ull << 30) / ((gmax + 1ull) * 8ull), 4));
  return static_cast<uint32_t>((w + 3) / 4 * 4);
}

}  // namespace rnamc

#endif
