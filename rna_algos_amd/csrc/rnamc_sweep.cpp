// rnamc_sweep.cpp — batch orchestration behind the C ABI: the batch plan and the reference-order sweep.
//
// A batch of independent sequences (the reference runs one thread-pool task per
// record: src/bin/mccaskill_algo.rs:64-93) is sorted by length and cut into
// lock-step groups; each group sweeps the anti-diagonals of all its sequences
// together, one kernel launch per diagonal and pass, on one HIP stream.  The DP
// state of a whole group lives in HBM (ten packed triangles per sequence); the
// 288 GB of an MI355X hold thousands of sequences at once.
#include "rnamc_ctx.h"
#include "rnamc_schedule.h"

using namespace rnamc;

namespace {

uint64_t tri_pad_of(uint32_t n) {
  // + 64 floats: kernels read up to one wave past a diagonal's end (values masked).
  // Column-major slots pad every column to 16 floats: 16 (m+1)(8m + r) floats for n columns.
  uint64_t t = static_cast<uint64_t>(n) * (n + 1ull) / 2ull;
  const uint64_t m = n >> 4, r = n & 15ull;
  t = std::max<uint64_t>(t, 16ull * (m + 1ull) * (8ull * m + r));
  return ((t + 63ull) & ~63ull) + 64ull;
}

int ensure_hp_init(rnamc_ctx* c, uint32_t max_n) {
  if (c->hp_init_len >= max_n + 1 && c->d_hp_init) return RNAMC_OK;
  uint32_t len = std::max<uint32_t>(max_n + 1, 64);
  std::vector<float> hp(len);
  hp_init_table(c->host_params.turner, len, hp.data());
  c->hp_init_len = 0;
  HIPCHK(c->d_hp_init.replace_exact(len));
  HIPCHK(hipMemcpy(c->d_hp_init, hp.data(), sizeof(float) * len, hipMemcpyHostToDevice));
  c->hp_init_len = len;
  c->h_hp_init = std::move(hp);
  return RNAMC_OK;
}

}  // namespace

namespace rnamc {

int BatchPlan::begin(rnamc_ctx* ctx, uint32_t n_seqs, const uint64_t* offsets) {
  c = ctx;
  c->stats = rnamc_batch_stats{};
  c->cx_launches = 0;
  c->cx_ms = 0.0;
  c->kev_class.clear();
  c->descs.clear();
  c->group_begin.clear();
  c->group_out_floats.clear();
  c->h_tseqs.clear();  // (the tree-order sweep fills it: rnamc_debug_fetch_tree tells by it which mode ran last)
  if (n_seqs == 0) return RNAMC_OK;
  for (uint32_t s = 0; s < n_seqs; s++) {
    if (offsets[s + 1] < offsets[s]) return RNAMC_ERR_INVALID_ARG;
    const uint64_t n = offsets[s + 1] - offsets[s];
    if (n == 0) return RNAMC_ERR_EMPTY_SEQ;
    if (n > RNAMC_MAX_SEQ_LEN) return RNAMC_ERR_SEQ_TOO_LONG;
    max_n = std::max<uint32_t>(max_n, static_cast<uint32_t>(n));
  }
  if (int rc = ensure_hp_init(c, max_n)) return rc;
  // longest first: within a group the sequences active on diagonal d are a prefix
  order.resize(n_seqs);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    return (offsets[a + 1] - offsets[a]) > (offsets[b + 1] - offsets[b]);
  });
  return RNAMC_OK;
}

void BatchPlan::cut(const uint64_t* offsets, const uint64_t* out_offsets, uint64_t ws_cap_floats,
                    const std::function<uint64_t(uint32_t)>& need_of, const std::function<void(SeqDesc&)>& place) {
  uint64_t cur = 0, cur_nt = 0, cur_out = 0;
  uint32_t cnt = 0;
  for (const uint32_t s : order) {
    const uint32_t n = static_cast<uint32_t>(offsets[s + 1] - offsets[s]);
    const uint64_t need = need_of(n);
    // a launch should carry enough cells to fill the chip: short sequences go into
    // larger groups (bounded by nucleotides, sequences and workspace bytes)
    if (cnt > 0 && (cnt >= static_cast<uint32_t>(c->group_max_seqs) ||
                    cur_nt + n > static_cast<uint64_t>(c->group_max_nt) ||
                    cur + need > ws_cap_floats)) {
      max_group_floats = std::max(max_group_floats, cur);
      c->group_out_floats.push_back(cur_out);
      cur = cur_nt = cur_out = 0;
      cnt = 0;
    }
    if (cnt == 0) c->group_begin.push_back(static_cast<uint32_t>(c->descs.size()));
    SeqDesc sd{};
    sd.n = n;
    sd.seq_off = offsets[s];
    sd.ws_off = cur;
    sd.out_off = out_offsets ? out_offsets[s] : cur_out;
    sd.batch_idx = s;
    place(sd);
    c->descs.push_back(sd);
    cur += need;
    cur_nt += n;
    cur_out += rnamc_bpp_len(n);
    cnt++;
  }
  max_group_floats = std::max(max_group_floats, cur);
  c->group_out_floats.push_back(cur_out);
  c->group_begin.push_back(static_cast<uint32_t>(c->descs.size()));
}

uint32_t BatchPlan::active(size_t g, uint32_t d) const {
  const uint32_t gb = c->group_begin[g];
  uint32_t lo = 0, hi = c->group_begin[g + 1] - gb;  // first index with n <= d
  while (lo < hi) {
    const uint32_t mid = (lo + hi) / 2;
    if (c->descs[gb + mid].n > d) lo = mid + 1; else hi = mid;
  }
  return lo;
}

int BatchPlan::create_events() {
  if (c->profile != 0) HIPCHK(c->events.grow(n_groups() * 4));
  return RNAMC_OK;
}

int BatchPlan::finish(hipStream_t st) {
  c->stats.n_groups = n_groups();
  c->stats.workspace_bytes = c->ws_floats * sizeof(float);
  if (c->profile == 0) return RNAMC_OK;
  HIPCHK(hipStreamSynchronize(st));
  const hipEvent_t* const gev = c->events.data();
  for (size_t g = 0; g < n_groups(); g++) {
    float a = 0, bms = 0, cc = 0;
    HIPCHK(hipEventElapsedTime(&a, gev[4 * g + 0], gev[4 * g + 1]));
    HIPCHK(hipEventElapsedTime(&bms, gev[4 * g + 1], gev[4 * g + 2]));
    HIPCHK(hipEventElapsedTime(&cc, gev[4 * g + 2], gev[4 * g + 3]));
    c->stats.ms_inside += a;
    c->stats.ms_outside += bms;
    c->stats.ms_other += cc;
  }
  return RNAMC_OK;
}

namespace {

// The sink that enqueues what the schedule (rnamc_schedule.h) decides: every method is the one HIP
// call or launch_* call it names, on the stream of the lane it is given.  A group's sink holds
// plain handles; the launches report nothing (hipGetLastError after the group does).
struct HipSink {
  const DeviceBatch& b;
  hipStream_t lane[2];      // kMain: the sweep's stream, kAux: the context's second stream
  const hipEvent_t* ev[2];  // kRingA, kRingB
  bool contra;
  uint32_t block, gmax;
  rnamc_batch_stats& stats;
  // profiling (profile >= 2): a pair of events around every outside kernel, on its stream
  bool time_kernels;
  EventRing& kev;
  std::vector<uint8_t>& kev_class;

  int record(Ring r, uint32_t slot, Lane l) {
    HIPCHK(hipEventRecord(ev[r][slot], lane[l]));
    return 0;
  }
  int wait(Lane l, Ring r, uint32_t slot) {
    HIPCHK(hipStreamWaitEvent(lane[l], ev[r][slot], 0));
    return 0;
  }
  int count_inside(uint32_t n) {
    stats.launches_inside += n;
    return 0;
  }
  int count_outside(uint32_t n) {
    stats.launches_outside += n;
    return 0;
  }

  int mfe_inside(uint32_t d_sums, uint32_t d_pair, uint32_t nseq) {
    launch_mfe_inside(b, contra, d_sums, d_pair, gmax, nseq, lane[kMain]);
    return 0;
  }
  int inside(Lane l, uint32_t d, uint32_t nseq, bool do_sums, bool do_pair) {
    launch_inside(b, contra, d, gmax, nseq, block, do_sums, do_pair, lane[l]);
    return 0;
  }
  int inside2(uint32_t d, uint32_t nseq, bool do_sums, bool do_head) {
    launch_inside2(b, contra, d, gmax, nseq, block, do_sums, do_head, lane[kMain]);
    return 0;
  }
  int inside_zr2(uint32_t d, uint32_t nseq) {
    launch_inside_zr2(b, d, gmax, nseq, block, lane[kMain]);
    return 0;
  }
  int pair_tail(uint32_t d0, uint32_t nd, uint32_t nseq) {
    launch_pair_tail(b, contra, d0, nd, gmax, nseq, block, lane[kMain]);
    return 0;
  }
  int inside_lat(uint32_t d, uint32_t nseq, int form, bool do_combine, uint32_t pair_d) {
    launch_inside_lat(b, contra, d, gmax, nseq, form, do_combine, pair_d, lane[kMain]);
    return 0;
  }
  int pair_lat(Lane l, uint32_t d, uint32_t nseq) {
    launch_pair_lat(b, contra, false, d, gmax, nseq, lane[l]);
    return 0;
  }

  // the outside launches, timed as class cls (0 main, 1 tail, 2 / 3 small)
  int outside(uint8_t cls, Lane l, uint32_t d, uint32_t nseq, bool do_mb, bool do_tail, bool do_head, int roles) {
    timed(cls, lane[l], [&]() { launch_outside(b, contra, d, gmax, nseq, block, do_mb, do_tail, do_head, roles, lane[l]); });
    return 0;
  }
  int outside_lat(uint8_t cls, uint32_t d, uint32_t nseq, bool do_mb, bool do_tail, bool head) {
    timed(cls, lane[kMain], [&]() { launch_outside_lat(b, contra, d, gmax, nseq, do_mb, do_tail, head, lane[kMain]); });
    return 0;
  }
  int outside_pair_lat(uint8_t cls, Lane l, uint32_t d, uint32_t nseq) {
    timed(cls, lane[l], [&]() { launch_pair_lat(b, contra, true, d, gmax, nseq, lane[l]); });
    return 0;
  }

 private:
  template <class Launch>
  void timed(uint8_t cls, hipStream_t s, Launch&& launch) {
    if (!time_kernels) {
      launch();
      return;
    }
    const size_t x = kev_class.size();
    if (kev.grow(2 * (x + 1)) != hipSuccess) {  // out of events: stop timing, keep running
      launch();
      return;
    }
    (void)hipEventRecord(kev[2 * x], s);
    launch();
    (void)hipEventRecord(kev[2 * x + 1], s);
    kev_class.push_back(cls);
  }
};

// profiling: the milliseconds and counts of the timed outside kernels, by class
void classify_outside_kernels(rnamc_ctx* c) {
  for (size_t x = 0; x < c->kev_class.size(); x++) {
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->kev[2 * x], c->kev[2 * x + 1]) != hipSuccess) continue;
    if (c->kev_class[x] == 0) {
      c->stats.ms_outside_main += ms;
      c->stats.launches_outside_main++;
    } else if (c->kev_class[x] == 1) {
      c->stats.ms_outside_tail += ms;
      c->stats.launches_outside_tail++;
    } else {
      c->stats.ms_outside_small += ms;
      c->stats.launches_outside_small++;
    }
  }
}

SweepKnobs sweep_knobs(const rnamc_ctx* c) {
  SweepKnobs k{};
  k.latency_mode = c->latency_mode;
  k.lat_max_cells = c->lat_max_cells;
  k.lat_inside = c->lat_inside;
  k.lat_pairs = c->lat_pairs;
  k.lat_merge = c->lat_merge;
  k.lat_split = c->lat_split;
  k.lat_zr_ahead = c->lat_zr_ahead;
  k.lat_e_waves = c->lat_e_waves;
  k.fuse_inside = c->fuse_inside;
  k.dual_outside = c->dual_outside;
  k.dual_min_cells = c->dual_min_cells;
  k.dual_max_diag = c->dual_max_diag;
  k.debug_roles = c->debug_roles;
  k.block_threads = c->block_threads;
  k.ring = static_cast<uint32_t>(c->ev_a.size());
  k.profile = c->profile;
  return k;
}

// act[d], d = 0 .. gmax: the group's sequences with n > d (its descriptors are sorted longest first)
void fill_active(const SeqDesc* seqs, uint32_t nseq, std::vector<uint32_t>& act) {
  act.assign(static_cast<size_t>(seqs[0].n) + 1, 0u);
  for (uint32_t i = 0; i < nseq; i++)
    for (uint32_t d = (i + 1 < nseq) ? seqs[i + 1].n : 0u; d < seqs[i].n; d++) act[d] = i + 1;
}

}  // namespace

// Core: everything device-resident, work enqueued on `st` (and, where the schedule says so, on the
// context's second stream between two points of `st`).
int run_batch(rnamc_ctx* c, uint32_t n_seqs, const uint8_t* d_bases, const uint64_t* offsets, bool contra,
              bool allows_short, float* d_out, const uint64_t* out_offsets, float* d_logz, hipStream_t st,
              const SweepOpts& opts, const GroupHooks* hooks) {
  BatchPlan plan;
  int rc = plan.begin(c, n_seqs, offsets);
  if (rc || n_seqs == 0) return rc;
  const uint64_t ws_cap_floats = static_cast<uint64_t>(std::max<int64_t>(c->group_ws_bytes, 1)) / 4;
  // a sequence's ten triangles, then its packed copy and the lists of its canonical cells
  struct Extra {
    uint64_t pk_words, cidx_words, ccnt_words, c64_words;
    explicit Extra(uint32_t n)
        : pk_words(((static_cast<uint64_t>(n) + 160) / 16 + 4 + 63) & ~63ull),
          cidx_words((tri_pad_of(n) + 1) / 2),  // u16 per cell, in 4-byte units
          ccnt_words((static_cast<uint64_t>(n) + 63) & ~63ull),
          c64_words(((static_cast<uint64_t>(n) + 63) / 64 * (static_cast<uint64_t>(n) + 64) + 63) & ~63ull) {}
  };
  plan.cut(
      offsets, hooks ? nullptr : out_offsets, ws_cap_floats,
      [](uint32_t n) {
        const Extra x(n);
        return tri_pad_of(n) * M_COUNT + x.pk_words + x.cidx_words + x.ccnt_words + x.c64_words;
      },
      [](SeqDesc& sd) {
        const Extra x(sd.n);
        sd.tri_pad = static_cast<uint32_t>(tri_pad_of(sd.n));
        sd.pk_words = static_cast<uint32_t>(x.pk_words);
        sd.pk_off = sd.ws_off + tri_pad_of(sd.n) * M_COUNT;
        sd.cidx_off = sd.pk_off + x.pk_words;
        sd.ccnt_off = sd.cidx_off + x.cidx_words;
        sd.c64_off = sd.ccnt_off + x.ccnt_words;
      });
  rc = ensure_ws(c, plan.max_group_floats);
  if (rc) return rc;
  rc = upload_descs(c->d_seqs, c->descs, st);
  if (rc) return rc;
  const size_t n_groups = plan.n_groups();
  const bool prof = c->profile != 0;
  rc = plan.create_events();
  if (rc) return rc;
  const hipEvent_t* const gev = c->events.data();
  const SweepKnobs knobs = sweep_knobs(c);
  std::vector<uint32_t> act;

  for (size_t g = 0; g < n_groups; g++) {
    const uint32_t gb = c->group_begin[g], ge = c->group_begin[g + 1];
    const uint32_t nseq = ge - gb;
    const uint32_t gmax = c->descs[gb].n;
    DeviceBatch b{};
    b.seqs = c->d_seqs + gb;
    b.bases = d_bases;
    b.workspace = c->d_ws;
    b.out = d_out;
    if (hooks) {
      rc = hooks->before(g, &b.out);
      if (rc) return rc;
    }
    b.log_partition = d_logz;
    b.params = c->d_params;
    b.hp_init = c->d_hp_init;
    b.allows_short_hairpins = allows_short ? 1 : 0;
    b.cons = opts.cons;
    b.max_span = opts.max_span;
    b.order_inside = static_cast<int>(c->order_inside);
    b.order_outside = static_cast<int>(c->order_outside);
    fill_active(&c->descs[gb], nseq, act);
    const GroupShape shape{gmax, nseq, contra, contra ? 0u : (RNAMC_MIN_SPAN_HAIRPIN_CLOSE - 1),
                           (contra && allows_short) ? 1u : (RNAMC_MIN_SPAN_HAIRPIN_CLOSE - 1), act.data()};
    c->last_dmin_out = shape.dmin_out;  // (rnamc_debug_fetch)
    HipSink sink{b,        {st, c->aux_stream}, {c->ev_a.data(), c->ev_b.data()},
                 contra,   static_cast<uint32_t>(knobs.block_threads), gmax,
                 c->stats, knobs.profile >= 2,  c->kev,
                 c->kev_class};
    if (prof) HIPCHK(hipEventRecord(gev[4 * g + 0], st));
    launch_init(b, nseq, gmax, st);
    c->stats.launches_other++;
    if (opts.maxplus) {
      // max-plus sweep (rnamc_mfe_batch): no outside sweep, no finalize
      rc = schedule_maxplus(shape, sink);
      if (rc) return rc;
      if (prof)
        for (int e = 1; e <= 3; e++) HIPCHK(hipEventRecord(gev[4 * g + e], st));
    } else {
      rc = schedule_inside(knobs, shape, sink);
      if (rc) return rc;
      // (the inside schedule ends on `st` alone; the outside schedule orders the second stream
      // behind an event recorded on `st` after this point)
      if (hooks && hooks->mid && !opts.inside_only) {
        rc = hooks->mid(g, gb, nseq);
        if (rc) return rc;
      }
      if (prof) HIPCHK(hipEventRecord(gev[4 * g + 1], st));
      // (rnamc_fold_scores needs the sums_close key set only: no outside sweep; the output
      // triangle then holds -1 / expf of stale log-probabilities and is not looked at)
      if (!opts.inside_only) {
        rc = schedule_outside(knobs, shape, sink);
        if (rc) return rc;
      }
      if (prof) HIPCHK(hipEventRecord(gev[4 * g + 2], st));
      launch_finalize(b, nseq, gmax, shape.dmin_out, st);
      c->stats.launches_other++;
      if (prof) HIPCHK(hipEventRecord(gev[4 * g + 3], st));
    }
    HIPCHK(hipGetLastError());
    if (hooks) {
      rc = hooks->after(g, gb, nseq);
      if (rc) return rc;
    }
  }
  rc = plan.finish(st);
  if (rc) return rc;
  if (prof) classify_outside_kernels(c);
  return RNAMC_OK;
}

int run_batch_mode(rnamc_ctx* c, uint32_t n_seqs, const uint8_t* d_bases, const uint64_t* offsets, bool contra,
                   bool allows_short, float* d_out, const uint64_t* out_offsets, float* d_logz, hipStream_t st,
                   const SweepOpts& opts, const GroupHooks* hooks) {
  if (c->summation_mode == 1 && !opts.inside_only)
    return run_batch_tree(c, n_seqs, d_bases, offsets, contra, allows_short, d_out, out_offsets, d_logz, st,
                          opts, hooks);
  return run_batch(c, n_seqs, d_bases, offsets, contra, allows_short, d_out, out_offsets, d_logz, st, opts, hooks);
}

}  // namespace rnamc
