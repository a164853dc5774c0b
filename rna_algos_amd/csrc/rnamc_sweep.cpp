// rnamc_sweep.cpp — batch orchestration behind the C ABI: the batch plan and the reference-order sweep.
//
// A batch of independent sequences (the reference runs one thread-pool task per
// record: src/bin/mccaskill_algo.rs:64-93) is sorted by length and cut into
// lock-step groups; each group sweeps the anti-diagonals of all its sequences
// together, one kernel launch per diagonal and pass, on one HIP stream.  The DP
// state of a whole group lives in HBM (ten packed triangles per sequence); the
// 288 GB of an MI355X hold thousands of sequences at once.
#include "rnamc_ctx.h"

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

// Core: everything device-resident, work enqueued on `st`.
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
  // the launch loops below read the context's events and second stream as plain handles
  const hipEvent_t* const gev = c->events.data();
  const hipEvent_t* const ev_a = c->ev_a.data();
  const hipEvent_t* const ev_b = c->ev_b.data();
  hipStream_t const aux = c->aux_stream;
  const uint32_t block = static_cast<uint32_t>(c->block_threads);
  const uint32_t dmin_in = contra ? 0u : (RNAMC_MIN_SPAN_HAIRPIN_CLOSE - 1);
  const uint32_t dmin_out = (contra && allows_short) ? 1u : (RNAMC_MIN_SPAN_HAIRPIN_CLOSE - 1);

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
    auto active = [&](uint32_t d) { return plan.active(g, d); };
    if (prof) HIPCHK(hipEventRecord(gev[4 * g + 0], st));
    launch_init(b, nseq, gmax, st);
    c->stats.launches_other++;
    if (opts.maxplus) {
      // max-plus sweep (rnamc_mfe_batch): the closing-pair cells of diagonal dmin_in, then per
      // diagonal d its sums beside the closing-pair cells of d+1; no outside sweep, no finalize
      launch_mfe_inside(b, contra, gmax, dmin_in, gmax, nseq, st);
      for (uint32_t d = dmin_in; d < gmax; d++) launch_mfe_inside(b, contra, d, d + 1, gmax, active(d), st);
      c->stats.launches_inside += gmax - dmin_in + 1;
      if (prof)
        for (int e = 1; e <= 3; e++) HIPCHK(hipEventRecord(gev[4 * g + e], st));
      HIPCHK(hipGetLastError());
      if (hooks) {
        rc = hooks->after(g, gb, nseq);
        if (rc) return rc;
      }
      continue;
    }
    // Inside sweep.  Dependencies: the closing-pair block of diagonal D is a left fold whose
    // early part (hairpin, 2-loops) needs sums_close of diagonals <= D-2 and whose last term
    // needs the folds of diagonal D-2; the folds of diagonal D need the pair blocks of
    // diagonals <= D (<= D+1 for the second cell of a two-diagonal launch).
    //   one-diagonal launch d : folds(d) beside the whole pair block of d+1
    //   two-diagonal launch d : folds(d, d+1) beside the early part of pair blocks d+2, d+3;
    //                           their last term follows in a small launch of its own
    // `pairs_done`: pair blocks complete up to here; `heads_done`: early part parked.
    const bool do_sums = (c->debug_roles & 1) != 0, do_pair = (c->debug_roles & 2) != 0;
    int64_t pairs_done = static_cast<int64_t>(dmin_in) - 1;  // nothing pairs below dmin_in
    int64_t heads_done = pairs_done;
    const uint32_t ring = static_cast<uint32_t>(c->ev_a.size());
    auto need_pairs = [&](int64_t upto) {  // complete the pair blocks of diagonals <= upto
      upto = std::min<int64_t>(upto, static_cast<int64_t>(gmax) - 1);
      while (pairs_done < upto) {
        const uint32_t D = static_cast<uint32_t>(pairs_done + 1);
        if (static_cast<int64_t>(D) <= heads_done) {
          const uint32_t nd = static_cast<uint32_t>(std::min<int64_t>(heads_done, upto)) - D + 1;
          if (do_pair) {
            launch_pair_tail(b, contra, D, nd, gmax, active(D), block, st);
            c->stats.launches_inside++;
          }
          pairs_done = D + nd - 1;
        } else {
          if (D >= 1 && do_pair) {
            launch_inside(b, contra, D - 1, gmax, active(D), block, false, true, st);
            c->stats.launches_inside++;
          }
          pairs_done = D;
          heads_done = std::max(heads_done, pairs_done);
        }
      }
    };
    // Latency-form group: folds(d) on `st` (k_inside_lat) beside the pair block of d+1 on
    // aux_stream; folds(d) need the pair block of d (aux, step before), the pair block of
    // d+1 needs the folds of d-1 (st, step before).
    // (CONTRAfold's chains hold more general steps: its crossover against the batch forms lies
    // at half the cells, profiles/r02_latency_forms.txt)
    const bool lat = c->latency_mode == 2 ||
                     (c->latency_mode == 1 &&
                      static_cast<uint64_t>(nseq) * gmax <=
                          static_cast<uint64_t>(contra ? c->lat_max_cells / 2 : c->lat_max_cells));
    const bool lat_in = lat && (c->lat_inside != 0 || c->lat_pairs != 0);
    if (lat_in) {
      bool have_a = false, have_b = false, combine_due = false, zr_parked = false;
      for (uint32_t d = dmin_in; d < gmax; d++) {
        need_pairs(d);  // (only the first diagonal finds work here)
        const bool pair_next = heads_done < static_cast<int64_t>(d) + 1 && d + 1 < gmax;
        const uint32_t pv = (d + ring - 1) % ring, cu = d % ring;
        // The eight-chains form completes sums_1ormore_basepairs of diagonal d-1 in the launch
        // of diagonal d (sequences that end at d-1 included).
        const uint64_t chains = 3ull * (gmax - d) * active(d);
        // (CONTRAfold, eight-chains form: two more chain kinds per cell, see lat_zr_ahead)
        const uint64_t kinds_e = (contra && c->lat_zr_ahead != 0) ? 5 : 3;
        // (CONTRAfold: three times the waves — its three-lanes form folds two chains per cell
        // one after the other, measured crossover in profiles/r02_latency_forms.txt)
        const uint64_t e_waves = static_cast<uint64_t>(c->lat_e_waves) * (contra ? 3 : 1);
        // eight chains per wave on the diagonals with few enough waves
        const int form = (do_sums && c->lat_inside != 0 && (chains / 3 * kinds_e + 7) / 8 <= e_waves) ? 2 : 0;
        const bool wave_form = form != 0;
        // CONTRAfold: a cell's sums_rightmost_basepairs folds (d steps) precede its other
        // folds (d steps more); all but their last step needs nothing of diagonal d, so the
        // eight-chains launch of diagonal d-1 runs them ahead (flag 4: do so for d+1, flag 8:
        // this diagonal's were parked)
        const bool zr_ahead = form == 2 && kinds_e == 5;
        const int form_arg = form | (zr_ahead ? 4 : 0) | (form == 2 && zr_parked ? 8 : 0);
        // the closing-pair blocks of diagonal d+1 ride in the same launch as the wave-form
        // chains of diagonal d (one launch per diagonal, no cross-stream events: ~12 us per
        // diagonal less than the two-stream schedule, profiles/r02_latency_forms.txt)
        const bool merged = wave_form && c->lat_pairs != 0 && c->lat_merge != 0;
        if (pair_next && do_pair && !merged) {
          if (!have_a) {  // everything so far is on `st`
            HIPCHK(hipEventRecord(ev_a[pv], st));
            have_a = true;
          }
          HIPCHK(hipStreamWaitEvent(aux, ev_a[pv], 0));
          if (c->lat_pairs != 0) {
            launch_pair_lat(b, contra, false, d + 1, gmax, active(d + 1), aux);
          } else {
            launch_inside(b, contra, d, gmax, active(d + 1), block, false, true, aux);
          }
          c->stats.launches_inside++;
        }
        if (have_b) HIPCHK(hipStreamWaitEvent(st, ev_b[pv], 0));
        if (do_sums) {
          const uint32_t pair_d = (merged && pair_next && do_pair) ? d + 1 : 0;
          if (wave_form || combine_due) {
            launch_inside_lat(b, contra, d, gmax, active(d >= 1 ? d - 1 : 0), form_arg, combine_due, pair_d, st);
            c->stats.launches_inside++;
          }
          if (!wave_form) {
            launch_inside(b, contra, d, gmax, active(d), block, true, false, st);
            c->stats.launches_inside++;
          }
          combine_due = wave_form;
        }
        zr_parked = zr_ahead;
        if (merged) {
          have_a = false;  // (recorded when a later diagonal needs it)
        } else {
          HIPCHK(hipEventRecord(ev_a[cu], st));
          have_a = true;
        }
        if (pair_next) {
          if (!merged) HIPCHK(hipEventRecord(ev_b[cu], aux));
          have_b = !merged;
          pairs_done = heads_done = d + 1;
        } else {
          have_b = false;
        }
      }
      if (have_b) HIPCHK(hipStreamWaitEvent(st, ev_b[(gmax - 1) % ring], 0));
      if (combine_due)  // combine of the last diagonal
        launch_inside_lat(b, contra, gmax, gmax, active(gmax - 1), 0, true, 0, st);
    }
    for (uint32_t d = dmin_in; d < gmax && !lat_in;) {
      const bool fuse = c->fuse_inside != 0 && d >= 2 && d + 1 < gmax &&
                        !inside_is_split(d, gmax, active(d));
      if (fuse) {
        need_pairs(static_cast<int64_t>(d) + 1);
        const bool head = heads_done < static_cast<int64_t>(d) + 2 && d + 2 < gmax;
        if (contra && do_sums) {
          launch_inside_zr2(b, d, gmax, active(d), block, st);
          c->stats.launches_inside++;
        }
        launch_inside2(b, contra, d, gmax, active(d), block, do_sums, head && do_pair, st);
        c->stats.launches_inside++;
        if (head) heads_done = std::min<int64_t>(static_cast<int64_t>(d) + 3, gmax - 1);
        d += 2;
      } else {
        need_pairs(d);
        // the whole pair block of d+1 rides along unless its early part is parked already
        const bool pair_next = heads_done < static_cast<int64_t>(d) + 1 && d + 1 < gmax;
        launch_inside(b, contra, d, gmax, active(d), block, do_sums, pair_next && do_pair, st);
        c->stats.launches_inside++;
        if (pair_next) pairs_done = heads_done = d + 1;
        d += 1;
      }
    }
    // (both inside schedules end on `st` alone; the outside schedules order their second stream
    // behind an event recorded on `st` after this point)
    if (hooks && hooks->mid && !opts.inside_only) {
      rc = hooks->mid(g, gb, nseq);
      if (rc) return rc;
    }
    if (prof) HIPCHK(hipEventRecord(gev[4 * g + 1], st));
    // (rnamc_fold_scores needs the sums_close key set only: no outside sweep; the output
    // triangle then holds -1 / expf of stale log-probabilities and is not looked at)
    if (!opts.inside_only)
    // Outside sweep.  Launch d carries probs_multibranch and the pair tail of diagonal d and
    // the 2-loop half (pair head) of diagonal d-1: start one diagonal early.  Large launches
    // run the pair tail as its own kernel on a second stream beside the other two roles
    // (its register footprint would otherwise set their occupancy); both kernels of
    // diagonal d need both kernels of diagonal d+1.
    {
      const bool r_mb = (c->debug_roles & 4) != 0, r_pp = (c->debug_roles & 8) != 0;
      // (debug builds: bit 4 drops the 2-loop half, bit 5 the multibranch half)
      const bool r_head = r_pp && (c->debug_roles & 16) == 0, r_tail = r_pp && (c->debug_roles & 32) == 0;
      bool dual = false;  // the previous diagonal ran as two kernels
      // profiling: a pair of events around every kernel, on the stream it is launched on
      auto timed = [&](uint8_t cls, hipStream_t s, auto&& launch) {
        if (c->profile < 2) {
          launch();
          return;
        }
        const size_t x = c->kev_class.size();
        if (c->kev.grow(2 * (x + 1)) != hipSuccess) {  // out of events: stop timing, keep running
          launch();
          return;
        }
        (void)hipEventRecord(c->kev[2 * x], s);
        launch();
        (void)hipEventRecord(c->kev[2 * x + 1], s);
        c->kev_class.push_back(cls);
      };
      if (lat) {
        // latency-form group: {probs_multibranch, multibranch half of the pair probabilities}
        // of diagonal d on `st` (k_outside_lat) beside the 2-loop half of diagonal d-1 on
        // aux_stream; both need both of diagonal d+1
        // (lat_merge: both in ONE launch on `st`, no events)
        const bool merged = c->lat_pairs != 0 && c->lat_merge != 0 && c->lat_split == 0;
        bool first = true;
        for (uint32_t d = gmax + 1; d-- > dmin_out && merged;) {
          const bool head = d >= 1 && d - 1 >= dmin_out && r_head;
          if (d < gmax || head) {
            timed(0, st, [&]() {
              launch_outside_lat(b, contra, d, gmax, active(d >= 1 ? d - 1 : 0), r_mb, r_tail, head, st);
            });
            c->stats.launches_outside++;
          }
        }
        for (uint32_t d = gmax + 1; d-- > dmin_out && !merged;) {
          const bool head = d >= 1 && d - 1 >= dmin_out;
          const uint32_t na = active(d >= 1 ? d - 1 : 0);
          const uint32_t pv = (d + 1) % ring, cu = d % ring;
          if (first) {
            HIPCHK(hipEventRecord(ev_a[pv], st));
          } else {
            HIPCHK(hipStreamWaitEvent(st, ev_b[pv], 0));
          }
          HIPCHK(hipStreamWaitEvent(aux, ev_a[pv], 0));
          if (d < gmax) {
            if (c->lat_split != 0) {
              timed(1, st, [&]() { launch_outside_lat(b, contra, d, gmax, active(d), r_mb, false, false, st); });
              timed(0, st, [&]() { launch_outside_lat(b, contra, d, gmax, active(d), false, r_tail, false, st); });
            } else {
              timed(0, st, [&]() { launch_outside_lat(b, contra, d, gmax, active(d), r_mb, r_tail, false, st); });
            }
            c->stats.launches_outside++;
          }
          HIPCHK(hipEventRecord(ev_a[cu], st));
          if (head && r_head) {
            timed(3, aux, [&]() {
              if (c->lat_pairs != 0) {
                launch_pair_lat(b, contra, true, d - 1, gmax, na, aux);
              } else {
                launch_outside(b, contra, d, gmax, na, block, false, false, true, 4, aux);
              }
            });
            c->stats.launches_outside++;
          }
          HIPCHK(hipEventRecord(ev_b[cu], aux));
          first = false;
        }
        if (!first) HIPCHK(hipStreamWaitEvent(st, ev_b[dmin_out % ring], 0));
      }
      for (uint32_t d = gmax + 1; d-- > dmin_out && !lat;) {
        const bool head = d >= 1 && d - 1 >= dmin_out;
        const uint32_t na = active(d >= 1 ? d - 1 : 0);
        // worth it where the 2-loop blocks dominate a launch: the folds of a cell grow with
        // the length of the diagonal, its 496 probes do not
        const bool want_dual = c->dual_outside != 0 && d < gmax &&
                               gmax - d <= static_cast<uint64_t>(c->dual_max_diag) &&
                               static_cast<uint64_t>(gmax - d) * na >= c->dual_min_cells;
        if (!want_dual) {
          if (dual) {  // back to one stream: wait for the other kernel of d+1
            HIPCHK(hipStreamWaitEvent(st, ev_b[(d + 1) % ring], 0));
            dual = false;
          }
          timed(2, st, [&]() {
            launch_outside(b, contra, d, gmax, na, block, r_mb, r_tail, head && r_head, 7, st);
          });
          c->stats.launches_outside++;
        } else {
          // both kernels of diagonal d need both kernels of diagonal d+1
          hipEvent_t ea = ev_a[d % ring], eb = ev_b[d % ring];
          const uint32_t pv = (d + 1) % ring;
          if (!dual) {
            // first two-kernel diagonal: everything so far is on `st`
            HIPCHK(hipEventRecord(ev_a[pv], st));
          } else {
            HIPCHK(hipStreamWaitEvent(st, ev_b[pv], 0));
          }
          HIPCHK(hipStreamWaitEvent(aux, ev_a[pv], 0));
          timed(0, st, [&]() {
            launch_outside(b, contra, d, gmax, na, block, r_mb, false, head && r_head, 5, st);
          });
          HIPCHK(hipEventRecord(ea, st));
          timed(1, aux, [&]() {
            launch_outside(b, contra, d, gmax, na, block, false, r_tail, false, 2, aux);
          });
          HIPCHK(hipEventRecord(eb, aux));
          c->stats.launches_outside += 2;
          dual = true;
        }
      }
      if (dual) HIPCHK(hipStreamWaitEvent(st, ev_b[dmin_out % ring], 0));
    }
    if (prof) HIPCHK(hipEventRecord(gev[4 * g + 2], st));
    launch_finalize(b, nseq, gmax, dmin_out, st);
    c->stats.launches_other++;
    if (prof) HIPCHK(hipEventRecord(gev[4 * g + 3], st));
    HIPCHK(hipGetLastError());
    if (hooks) {
      rc = hooks->after(g, gb, nseq);
      if (rc) return rc;
    }
  }
  rc = plan.finish(st);
  if (rc) return rc;
  if (prof) {
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
