// rnamc_entries.h — what the host-buffer entries share before and around their sweep: the record
// check, the compiled constraints of a call, the staging prologue, and the chunk scan of the entries
// that put derived records of one sequence through the sweep (windows, mutants).
#ifndef RNAMC_ENTRIES_H
#define RNAMC_ENTRIES_H

#include "rnamc_ctx.h"
#include "rnamc_shards.h"

namespace rnamc {

// Hard constraints of one batch call (include/rnamc.h).  prepare() validates
// and compiles every record on the host, before any device work and before the context's lock: two
// words per base, laid out like the staged bases (rnamc_scoring.h, pair_allowed), by the record loop
// the pool's pre-validation runs too (compile_constraints, rnamc_shards.h).  A call with
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
      return no_host_memory("constraints");
    }
    return strings ? compile_constraints(n_seqs, offsets, strings, words.data()) : RNAMC_OK;
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

  // Staging buffers are DevBufs of the context and only grow (a caller that folds one record after
  // another, like the reference's binaries, would otherwise pay an allocation and a free per call).
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
    HIPCHK(c->st_bases.grow(base_hi - base_lo));
    if (with_logz) HIPCHK(c->st_logz.grow(n_seqs));
    HIPCHK(hipMemcpyAsync(c->st_bases, bases + base_lo, base_hi - base_lo, hipMemcpyHostToDevice,
                          c->own_stream));
    if (!cons.active) return RNAMC_OK;
    HIPCHK(c->st_cons.upload(cons.words.data(), cons.words.size(), c->own_stream));
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
  HIPCHK(c->st_out[0].grow(std::max<uint64_t>(c->group_out_floats[g], 1)));
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

// The end of one staged call of an entry that runs the sweep several times: its own launches and the
// milliseconds of its event pairs (EventRing::pairs) into the two statistics fields that are the
// entry's, then the call's statistics added to `total`.
inline int fold_call_stats(rnamc_ctx* c, rnamc_batch_stats* total, uint64_t launches, const EventRing& ring,
                           size_t ev_pairs, uint64_t rnamc_batch_stats::*launches_own,
                           double rnamc_batch_stats::*ms_own) {
  c->stats.launches_other += launches;
  c->stats.*launches_own = launches;
  c->stats.*ms_own = 0.0;
  if (c->profile != 0) HIPCHK(ring.pairs_ms(ev_pairs, &(c->stats.*ms_own)));
  add_sweep_stats(total, c->stats);
  total->*launches_own += c->stats.*launches_own;
  total->*ms_own += c->stats.*ms_own;
  return RNAMC_OK;
}

// One chunk scan: `count` derived records of one fixed length, cut out of one sequence, through the
// bpp sweep chunk by chunk (`per_chunk` records a staged call) and group by group.  A group's
// triangles stay on the device (st_out[0], group-local offsets) and the caller's kernels run behind
// its finalize kernel in stream order, without a host round-trip.  The caller says how a record is
// cut, what an item holds, which kernels a slice of descriptors launches and which statistics
// fields are its own; the scan owns everything else.
struct ChunkScan {
  const char* who;   // the entry's name, and the noun of its records ("windows") for the messages
  const char* what;
  uint32_t rec_len;
  uint64_t count, per_chunk;
  bool with_constraint;
  uint32_t max_bp_span;
  bool contra, allows_short;
  float* log_partition;  // of record 0 of the scan, or null
  EventRing* events;     // profiling: a pair around every group's launches
  uint64_t rnamc_batch_stats::*launches_own;
  double rnamc_batch_stats::*ms_own;
  // record x of the scan (and its constraint, where there is one) written to rec / cons
  std::function<void(uint64_t x, uint8_t* rec, char* cons)> cut;
  // the chunk starting at record x0 is planned (c->descs, m of them): fill and upload its items
  std::function<int(uint64_t x0, uint32_t m)> upload_items;
  // the kernels of descriptors [first_desc, first_desc + k), k <= 65 535 -> the number of launches
  std::function<uint64_t(uint32_t first_desc, uint32_t k)> launch;
  // optional: after the chunk's sweep is enqueued, before its stream is drained
  std::function<int(uint64_t x0, uint32_t m)> after_sweep;
};

inline int scan_chunks(rnamc_ctx* c, const ChunkScan& s, rnamc_batch_stats* total) {
  hipStream_t st = c->own_stream;  // (a call with hooks never takes the two-stream route of the tree order)
  const uint32_t w = s.rec_len;
  std::vector<uint8_t> cb;
  std::vector<char> cc;
  std::vector<uint64_t> offs;
  try {  // nothing may throw across the C boundary
    cb.resize(s.per_chunk * w);
    if (s.with_constraint) cc.resize(s.per_chunk * w);
    offs.resize(s.per_chunk + 1);
  } catch (const std::exception&) {
    set_last_error(std::string(s.who) + ": no host memory for a chunk of " + s.what);
    return RNAMC_ERR_OOM;
  }
  const bool prof = c->profile != 0;
  for (uint64_t x0 = 0; x0 < s.count; x0 += s.per_chunk) {
    const uint32_t m = static_cast<uint32_t>(std::min<uint64_t>(s.per_chunk, s.count - x0));
    // the chunk's records as ordinary records (they may overlap in the sequence; the record checks
    // want monotone offsets)
    for (uint32_t x = 0; x <= m; x++) offs[x] = static_cast<uint64_t>(x) * w;
    for (uint32_t x = 0; x < m; x++)
      s.cut(x0 + x, cb.data() + offs[x], s.with_constraint ? cc.data() + offs[x] : nullptr);
    ConsCall cons;
    if (int rc = cons.prepare(m, offs.data(), s.with_constraint ? cc.data() : nullptr, s.max_bp_span)) return rc;
    StagedCall sc(c, true);
    if (int rc = sc.stage(c, s.who, m, cb.data(), offs.data(), cons)) return rc;
    uint64_t launches = 0;  // (run_batch* resets the context's statistics when it starts)
    size_t ev_pairs = 0;
    GroupHooks hooks;
    hooks.before = [&](size_t g, float** out_base) -> int {
      if (g == 0) {
        // the plan of the chunk is cut: one item per record for all its groups, uploaded once
        if (int rc = s.upload_items(x0, m)) return rc;
        if (prof) HIPCHK(s.events->pairs(c->group_begin.size() - 1));
      }
      return group_triangles(c, g, out_base);
    };
    hooks.after = [&](size_t g, uint32_t first_desc, uint32_t n_desc) -> int {
      // the group's finalize kernel is enqueued on `st`; the next group's writes st_out[0] behind
      // these launches in stream order
      if (prof) HIPCHK(hipEventRecord((*s.events)[2 * g], st));
      for (uint32_t x = 0; x < n_desc; x += 65535u) launches += s.launch(first_desc + x, std::min(n_desc - x, 65535u));
      HIPCHK(hipGetLastError());
      if (prof) {
        HIPCHK(hipEventRecord((*s.events)[2 * g + 1], st));
        ev_pairs = g + 1;
      }
      return RNAMC_OK;
    };
    int rc = run_batch_mode(c, m, c->st_bases, sc.doff.data(), s.contra, s.allows_short, nullptr, nullptr,
                            c->st_logz, st, sc.opts, &hooks);
    if (rc == RNAMC_OK && s.after_sweep) rc = s.after_sweep(x0, m);
    rc = sc.finish(c, rc, m, s.log_partition ? s.log_partition + x0 : nullptr);
    if (rc) return rc;
    if (int rc2 = fold_call_stats(c, total, launches, *s.events, ev_pairs, s.launches_own, s.ms_own)) return rc2;
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

// The centroid stage of rnamc_centroid_fold_batch and rnamc_bpp_alignment (rnamc_entries_centroid.cpp):
// the gamma-centroid folds of `count` device-resident triangles (longest first) for every threshold,
// the (max,+) fill and the traceback on the device in chunks of "centroid_chunk_bytes" of the
// context's workspace.  Runs on own_stream and drains it.  emit(x, g, row, n_pairs, accuracy) is
// called once per (sequence x, threshold g) from the calling thread; row == nullptr: the empty fold
// (every byte '.').  The host scratch lives in the stage and is reused from group to group.
struct CentroidSeq {
  uint64_t bpp_off;  // float offset of the sequence's triangle in `d_bpp`
  uint32_t n;
};
using CentroidEmit = std::function<void(uint32_t x, uint32_t g, const uint8_t* row, uint32_t n_pairs, float accuracy)>;
struct CentroidStage {
  const char* who = "";
  int cus = 0;
  uint64_t launches = 0;  // of all runs so far
  int init(rnamc_ctx* c, const char* entry);
  int run(rnamc_ctx* c, const float* d_bpp, const CentroidSeq* seqs, uint32_t count, const float* gammas,
          uint32_t ng, const CentroidEmit& emit);

 private:
  std::vector<CentroidItem> items;
  std::vector<uint32_t> item_seq;  // sequence of every item of the running chunk
  std::vector<uint64_t> ids;       // the items that need the fill: sequence * ng + threshold
  std::vector<uint8_t> h_rows;
  std::vector<uint32_t> h_np;
  std::vector<float> h_acc;
};

}  // namespace rnamc

#endif
