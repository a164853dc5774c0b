// rnamc_sweep_tree.cpp — the tree-order summation mode's sweep (rnamc_tree.hip) over a batch plan,
// and the 2-loop tables it reads.
#include "rnamc_ctx.h"

using namespace rnamc;

namespace {

// Length-dependent part of the generic 2-loop scores of the tree-order mode (TreeTabs), from
// the parameter block.  Turner: bulge_scores_init[len] | interior_scores_init[len] +
// max(ninio_coeff * |a-b|, ninio_max) (src/utils.rs:234-321); CONTRAfold: the cumulative
// bulge / interior length, symmetric / asymmetric and explicit terms (456-520).
void build_tree_tabs(const rnamc_params& P, TreeTabs& T) {
  std::memset(&T, 0, sizeof(T));
  const rnamc_turner_scores& t = P.turner;
  const rnamc_fold_score_sets& f = P.contra;
  for (uint32_t p = 0; p < 512; p++) {
    const uint32_t r = p >> 5, c = p & 31u;
    const bool first = c < 31u - r;
    const uint32_t a = first ? r : 30u - r, b = first ? c : c - (31u - r);
    if (!(r < 15u || c < 16u)) continue;  // not a probe slot
    const uint32_t len = a + b, diff = a > b ? a - b : b - a;
    const bool bulge = (a == 0u) != (b == 0u);
    if (len < 2u) continue;  // stack / 0x1: scored by the flat scorers
    if (bulge) {
      T.len[0][p] = t.bulge_scores_init[len];
      T.len[1][p] = f.bulge_scores_len_cumulative[len - 1u];
    } else if (a >= 1u && b >= 1u) {
      const float nin = t.ninio_coeff * static_cast<float>(diff);
      T.len[0][p] = t.interior_scores_init[len] + (nin > t.ninio_max ? nin : t.ninio_max);
      const float s0 = (a == b) ? f.interior_scores_symmetric_cumulative[a - 1u]
                                : f.interior_scores_asymmetric_cumulative[diff - 1u];
      const float se = (a <= RNAMC_MAX_INTERIOR_EXPLICIT && b <= RNAMC_MAX_INTERIOR_EXPLICIT)
                           ? f.interior_scores_explicit[a - 1u][b - 1u]
                           : 0.f;
      T.len[1][p] = (s0 + se) + f.interior_scores_len_cumulative[len - 2u];
    }
  }
  // the generic slots by class, then a + b (lane-per-cell sweeps); classes as slot_class of rnamc_tree.hip
  for (int m = 0; m < 2; m++) {
    uint32_t cnt = 0;
    for (uint32_t c = 0; c < 4u; c++) {
      T.gstart[m][c] = cnt;
      uint32_t in_class = 0;
      for (uint32_t s = 0; s <= 31u; s++) {
        for (uint32_t a = 0; a <= s && s <= 30u; a++) {
          const uint32_t b = s - a;
          const bool special = m == 0 ? ((a + b <= 1u) || (a >= 1u && a <= 2u && b >= 1u && b <= 2u)) : (a <= 1u && b <= 1u);
          if (special) continue;
          const uint32_t cls = ((a == 0u) != (b == 0u)) ? 0u
                               : (a == 1u || b == 1u) ? 1u
                               : ((a == 2u && b == 3u) || (a == 3u && b == 2u)) ? 2u : 3u;
          if (cls != c) continue;
          const uint32_t p = a <= 15u ? a * 32u + b : (30u - a) * 32u + b + a + 1u;  // (probe_slot's inverse)
          T.gslot[m][cnt] = a | (s << 8);
          T.glen[m][cnt] = T.len[m][p];
          cnt++;
          in_class++;
        }
        T.gcount[m][c][s] = in_class;
      }
      while (cnt % 8u != 0u) {  // (never counted: keeps an eight-wide read inside the list)
        T.gslot[m][cnt] = in_class ? T.gslot[m][cnt - 1] : 0u;
        T.glen[m][cnt] = 0.f;
        cnt++;
      }
    }
    // class 3 in runs of four consecutive a per level
    uint32_t ng = 0;
    for (uint32_t s = 0; s <= 31u; s++) {
      if (s <= 30u) {
        uint32_t amin = ~0u, amax = 0u;
        for (uint32_t a = 0; a <= s; a++) {
          const uint32_t b = s - a;
          const bool special = m == 0 ? ((a + b <= 1u) || (a >= 1u && a <= 2u && b >= 1u && b <= 2u)) : (a <= 1u && b <= 1u);
          const bool c3 = !special && a >= 2u && b >= 2u && !((a == 2u && b == 3u) || (a == 3u && b == 2u));
          if (!c3) continue;
          amin = std::min(amin, a);
          amax = std::max(amax, a);
        }
        for (uint32_t a0 = amin; amin != ~0u && a0 <= amax; a0 += 4u) {
          T.g4slot[m][ng] = a0 | (s << 8);
          for (uint32_t u = 0; u < 4u; u++) {
            const uint32_t a = a0 + u, b = s - a;  // (a <= amax <= s - 2: b >= 2)
            const uint32_t p = a <= 15u ? a * 32u + b : (30u - a) * 32u + b + a + 1u;
            T.g4len[m][ng][u] = a <= amax ? T.len[m][p] : -INFINITY;
          }
          ng++;
        }
      }
      T.g4count[m][s] = ng;
    }
    // classes 0 and 1 by level: (0, s), (s, 0), (1, s - 1), (s - 1, 1)
    for (uint32_t s = 0; s < 32u; s++)
      for (uint32_t u = 0; u < 4u; u++) {
        T.elen[m][s][u] = -INFINITY;
        if (s < 2u || s > 30u) continue;
        const uint32_t a = u == 0u ? 0u : (u == 1u ? s : (u == 2u ? 1u : s - 1u)), b = s - a;
        const bool special = m == 0 ? ((a + b <= 1u) || (a >= 1u && a <= 2u && b >= 1u && b <= 2u)) : (a <= 1u && b <= 1u);
        const uint32_t cls = ((a == 0u) != (b == 0u)) ? 0u : (a == 1u || b == 1u) ? 1u : 3u;
        if (special || cls != (u < 2u ? 0u : 1u)) continue;
        if (u == 3u && s - 1u == 1u) continue;  // ((1, 1) once)
        const uint32_t p = a <= 15u ? a * 32u + b : (30u - a) * 32u + b + a + 1u;
        T.elen[m][s][u] = T.len[m][p];
      }
    for (uint32_t x = 0; x < 8u && ng < 128u; x++, ng++) {  // (never counted: a step's reads stay inside the list)
      T.g4slot[m][ng] = T.g4slot[m][ng - 1];
      for (uint32_t u = 0; u < 4u; u++) T.g4len[m][ng][u] = -INFINITY;
    }
  }
}

int ensure_tree_tabs(rnamc_ctx* c, hipStream_t st) {
  if (c->tree_tabs_valid && c->d_tree_tabs) return RNAMC_OK;
  if (!c->d_tree_tabs) HIPCHK(c->d_tree_tabs.replace_exact(1));
  static thread_local TreeTabs tabs;  // (16 KB: not on the stack; the copy below is synchronous)
  build_tree_tabs(c->host_params, tabs);
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(hipMemcpy(c->d_tree_tabs, &tabs, sizeof(TreeTabs), hipMemcpyHostToDevice));
  c->tree_tabs_valid = true;
  return RNAMC_OK;
}

}  // namespace

namespace rnamc {

// Tree-order summation mode (rnamc_tree.hip): same grouping and per-diagonal sweep, dense
// n x n matrices, one workgroup per cell.  Fills c->descs / group_* like run_batch so that the
// host-buffer entry's drain thread works unchanged.
int run_batch_tree(rnamc_ctx* c, uint32_t n_seqs, const uint8_t* d_bases, const uint64_t* offsets, bool contra,
                   bool allows_short, float* d_out, const uint64_t* out_offsets, float* d_logz, hipStream_t st,
                   const SweepOpts& opts, const GroupHooks* hooks) {
  BatchPlan plan;
  int rc = plan.begin(c, n_seqs, offsets);
  if (rc || n_seqs == 0) return rc;
  const uint32_t max_n = plan.max_n;
  rc = ensure_tree_tabs(c, st);
  if (rc) return rc;
  uint64_t ws_cap_floats = static_cast<uint64_t>(std::max<int64_t>(c->group_ws_bytes, 1)) / 4;
  // banding needs two diagonals per launch aligned to even diagonals, 32-bit float offsets INSIDE
  // one matrix (true for every n <= RNAMC_MAX_SEQ_LEN: ld * n < 2^32), and sequences long enough
  // to have a banded diagonal at all
  uint32_t band = (c->tree_two != 0 && c->tree_band >= 32) ? static_cast<uint32_t>(c->tree_band) & ~31u : 0u;
  if (band > 128u) band = 128u;
  {
    const uint64_t ld = ((static_cast<uint64_t>(max_n) + 31u) & ~31ull) + 32u;
    if (ld * max_n + 128ull >= (1ull << 32) || max_n < 3u * band + 2u) band = 0u;
  }
  if (band && !c->bulk_stream) {
    int lo = 0, hi = 0;
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    HIPCHK(hipStreamCreateWithPriority(c->bulk_stream.put(), hipStreamNonBlocking, lo));
  }
  if (band) {
    // The banded sweep lives on the mid-field kernels running BESIDE it.  Whether the side stream
    // owns a hardware queue depends on what else the process created (round 3: created late it
    // shared the sweep's queue, 157 ms instead of 49.5): detected, not assumed — once per caller
    // stream; a serialised side stream means the unbanded sweep (slower, never wrong).
    if (c->tree_side_force == 1 || c->tree_side_force == 2) {  // (knob "tree_side_stream": the verdict is given)
      c->side_verdict = static_cast<int>(c->tree_side_force);
      c->side_probed = true;
      c->side_probed_for = nullptr;
    } else if (!c->side_probed || c->side_probed_for != st) {
      c->side_verdict = tree_side_stream_probe(st, c->bulk_stream);
      c->side_probed = true;
      c->side_probed_for = st;
    }
  }
  // lane-per-cell sweeps: what a batch's fat launches want (a lone sequence keeps the wave-per-cell chain)
  uint32_t lane_mode = 0u;
  {
    const int64_t mode = c->tree_lane & 3;
    // (a plane of the sweep is one raw buffer there: msz * 4 bytes in a 32-bit record count)
    const uint64_t ld_max = ((static_cast<uint64_t>(max_n) + 31u) & ~31ull) + 32u;
    if (band && ld_max * max_n * 4ull + 1024ull < (1ull << 31) && (mode == 2 || (mode == 1 && offsets[n_seqs] - offsets[0] >= static_cast<uint64_t>(c->tree_lane_min_nt) && n_seqs > 1)))
      lane_mode = 3u;
  }
  // (a serialised side stream: the unbanded sweep — unless the mid-field kernels run in front of their
  // band on the sweep's own stream anyway; sums_external's walks then simply queue behind)
  if (band && c->side_verdict == 2 && !(lane_mode && c->tree_mid_sync != 0)) {
    band = 0u;
    lane_mode = 0u;
  }
  if (lane_mode && c->tree_mid_sync != 0 && static_cast<uint32_t>(c->tree_lane_band) < band)
    band = static_cast<uint32_t>(c->tree_lane_band);
  if (lane_mode && !c->group_ws_user) {
    // The batch form's launches cost ~8 us each whatever they hold, and a group's 36 n^2 floats per
    // sequence are what limits its size: twice the default workspace where the device has the room
    // (measured on a 1 000-sequence slice of the bench batch: 16 / 32 / 64 / 128 GB -> 1167 / 909 / 787 /
    // 753 ms per pass).
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) {
      const uint64_t have = static_cast<uint64_t>(free_b) + c->ws_floats * 4ull;
      const uint64_t margin = 24ull << 30;
      if (have > (128ull << 30) + margin) ws_cap_floats = (128ull << 30) / 4;
    } else {
      (void)hipGetLastError();
    }
  }
  // two groups side by side (see tree_dual): each gets half of the cap
  bool dual = lane_mode != 0u && c->tree_mid_sync != 0 && c->tree_dual != 0 && hooks == nullptr &&
              st != c->aux_stream && st != c->own_stream;
  if (dual) ws_cap_floats /= 2;
  std::vector<TreeSeq>& tseqs = c->h_tseqs;
  tseqs.clear();
  tseqs.reserve(n_seqs);
  // a sequence's T_COUNT matrices and two vectors, then its packed copy and the rings
  auto layout = [](uint32_t n) {
    TreeSeq ts{};
    ts.n = n;
    ts.ld = ((n + 31u) & ~31u) + 32u;
    ts.msz = ((static_cast<uint64_t>(ts.ld) * n + 63ull) & ~63ull) + 64ull;
    const uint64_t vec = (static_cast<uint64_t>(n) + 64ull + 63ull) & ~63ull;
    ts.pk_words = static_cast<uint32_t>(((static_cast<uint64_t>(n) + 160) / 16 + 4 + 63) & ~63ull);
    ts.pk_off = ts.msz * T_COUNT + 2ull * vec;  // (relative to ws_off here)
    ts.mid_off = ts.pk_off + ts.pk_words;
    return ts;
  };
  plan.cut(
      offsets, hooks ? nullptr : out_offsets, ws_cap_floats,
      [&](uint32_t n) {
        // (mid-field ring: three products x 2 bands of diagonals x vec cells x {max, sum})
        // + the far ring (four diagonals x vec cells x {max, sum})
        const uint64_t vec = (static_cast<uint64_t>(n) + 64ull + 63ull) & ~63ull;
        return layout(n).mid_off + (band ? (3ull * (2ull * band) + 4ull) * vec * 2ull : 0ull);
      },
      [&](SeqDesc& sd) {  // (descs: host bookkeeping shared with the reference-order path)
        TreeSeq ts = layout(sd.n);
        ts.seq_off = sd.seq_off;
        ts.ws_off = sd.ws_off;
        ts.pk_off += sd.ws_off;
        ts.mid_off += sd.ws_off;
        ts.out_off = sd.out_off;
        ts.batch_idx = sd.batch_idx;
        tseqs.push_back(ts);
      });
  const uint64_t max_group_floats = plan.max_group_floats;
  if (c->group_begin.size() < 3) dual = false;  // (a single group)
  rc = ensure_ws(c, dual ? 2 * max_group_floats : max_group_floats);
  if (rc) return rc;
  if (dual && !c->ev_dual) {
    // (no new streams: a process's fifth and later streams share hardware queues on this runtime — the second
    // group's sweep would sit in the first one's queue, measured: 698 instead of 556 ms — so the second group
    // takes the two streams the context created first for the reference-order path, idle in this mode)
    c->dual_stream = c->aux_stream;
    c->bulk_stream2 = c->own_stream;
    HIPCHK(hipEventCreateWithFlags(c->ev_dual.put(), hipEventDisableTiming));
    HIPCHK(c->ev_a2.grow(c->ev_a.size()));
    HIPCHK(c->ev_b2.grow(c->ev_a.size()));
  }
  rc = upload_descs(c->d_tseqs, tseqs, st);
  if (rc) return rc;
  const size_t n_groups = plan.n_groups();
  const bool prof = c->profile != 0;
  rc = plan.create_events();
  if (rc) return rc;
  const hipEvent_t* const gev = c->events.data();  // (the launch loops below read plain handles)
  hipStream_t const bulk = c->bulk_stream;
  const uint32_t dmin_in = contra ? 0u : (RNAMC_MIN_SPAN_HAIRPIN_CLOSE - 1);
  const uint32_t dmin_out = (contra && allows_short) ? 1u : (RNAMC_MIN_SPAN_HAIRPIN_CLOSE - 1);
  if (dual) {  // (the second stream starts behind whatever the caller's stream holds: the descriptors' copy)
    HIPCHK(hipEventRecord(c->ev_dual, st));
    HIPCHK(hipStreamWaitEvent(c->dual_stream, c->ev_dual, 0));
  }
  for (size_t g = 0; g < n_groups; g++) {
    const bool odd = dual && (g & 1u) != 0u;
    hipStream_t gst = odd ? c->dual_stream : st;
    hipStream_t gbulk = odd ? c->bulk_stream2 : bulk;
    const hipEvent_t* const gev_a = (odd ? c->ev_a2 : c->ev_a).data();
    const hipEvent_t* const gev_b = (odd ? c->ev_b2 : c->ev_b).data();
    const uint32_t gb = c->group_begin[g], ge = c->group_begin[g + 1];
    const uint32_t nseq = ge - gb;
    const uint32_t gmax = c->descs[gb].n;
    TreeBatch b{};
    b.seqs = c->d_tseqs + gb;
    b.one = tseqs[gb];
    b.use_one = nseq == 1 ? 1u : 0u;
    b.bases = d_bases;
    b.workspace = c->d_ws + (odd ? max_group_floats : 0);
    b.out = d_out;
    if (hooks) {
      rc = hooks->before(g, &b.out);
      if (rc) return rc;
    }
    b.log_partition = d_logz;
    b.params = c->d_params;
    b.tabs = c->d_tree_tabs;
    b.hp_init = c->d_hp_init;
    b.allows_short_hairpins = allows_short ? 1 : 0;
#ifdef RNAMC_DEBUG_KNOBS
    b.debug = static_cast<int>(c->tree_debug);
#endif
    b.ring = 2u * band;
    b.lane = lane_mode;
    b.cons = opts.cons;
    b.max_span = opts.max_span;
    auto active = [&](uint32_t d) { return plan.active(g, d); };
    if (prof) HIPCHK(hipEventRecord(gev[4 * g + 0], gst));
    launch_tree_init(b, nseq, gmax, contra, 0, gst);
    launch_tree_static(b, contra, nseq, gmax, gst);
    c->stats.launches_other += 2;
    if (lane_mode) {
      launch_tlane_list(b, gmax, nseq, gst);
      c->stats.launches_other++;
    }
    const bool two = c->tree_two != 0;
    const uint32_t ering = static_cast<uint32_t>(c->ev_a.size());
    if (band) {
      // Banded sweep: launches are pairs (2m, 2m+1) (a lone first / last diagonal where the
      // range starts odd / ends even), so no launch straddles a band [x*band, (x+1)*band).
      // Inside: band x >= 3 takes the terms with both operand spans below thr = (x-1)*band from
      // k_tree_mid, which needs the diagonals below thr: enqueued on bulk_stream when band
      // x-1 starts, awaited when band x starts.  Rings: ev_a "the sweep reached a band boundary",
      // ev_b "mid-field of the band written".
      const uint32_t nb = (gmax + band - 1) / band;  // bands 0 .. nb-1
      // sums_external's first row and last column (k_tree_ext) trail the sweep by one band on
      // bulk_stream as well (the outside sweep is their only reader).
      auto boundary = [&](uint32_t x) -> int {  // "the sweep reached band x": bulk_stream may pass
        HIPCHK(hipEventRecord(gev_a[x % ering], gst));
        HIPCHK(hipStreamWaitEvent(gbulk, gev_a[x % ering], 0));
        return RNAMC_OK;
      };
      auto enqueue_mid = [&](bool outside, uint32_t x, uint32_t thr) -> int {
        const uint32_t dlo = x * band, dhi = std::min(gmax - 1, dlo + band - 1);
#ifdef RNAMC_DEBUG_KNOBS
        if (!(c->tree_debug & 32))  // (timing: the sweep without its mid-field kernels; results wrong)
#endif
        launch_tree_mid(b, outside, dlo, dhi, thr, gmax, active(dlo), c->tree_pol, gbulk);
        HIPCHK(hipEventRecord(gev_b[x % ering], gbulk));
        c->stats.launches_other++;
        return RNAMC_OK;
      };
      auto enqueue_ext = [&](uint32_t x) {  // band x of the inside sweep is enqueued whole
        const uint32_t dlo = std::max(dmin_in, x * band), dhi = std::min(gmax - 1, x * band + band - 1);
        if (dlo > dhi) return;
#ifdef RNAMC_DEBUG_KNOBS
        if (!(c->tree_debug & 64))
#endif
        launch_tree_ext(b, contra, dlo, dhi, gmax, active(dlo), gbulk);
        c->stats.launches_other++;
      };
      const bool sync_in = (lane_mode & 1u) != 0u && c->tree_mid_sync != 0;
      const bool sync_out = (lane_mode & 2u) != 0u && c->tree_mid_sync != 0;
      const bool ahead = c->tree_ahead != 0 && (c->tree_tpc == 0 || c->tree_tpc == 64);
      bool use_far = false;  // (the first launch of a sweep forms its blocks whole)
      uint32_t g_next = std::max(5u, dmin_in);  // lane-per-cell sweeps: the next diagonal without its generic 2-loop sums
      uint32_t d = dmin_in;
      uint32_t cur_band = ~0u;
      while (d < gmax) {
        const uint32_t x = d / band;
        if (x != cur_band) {
          // band x starts: everything below x*band is enqueued; sums_external of band x-1 and
          // the mid-field of band x+1 can go
          if (lane_mode && cur_band != ~0u) {  // (their readers want the band row- / column-major)
            launch_tlane_spread(b, false, cur_band * band, std::min(gmax - 1, cur_band * band + band - 1), gmax,
                                active(cur_band * band), gst);
            c->stats.launches_other++;
          }
          rc = boundary(x);
          if (rc) return rc;
          if (cur_band != ~0u) enqueue_ext(cur_band);
          cur_band = x;
          if (sync_in) {
            // (a batch: the band's mid-field in front of the band, on the sweep's own stream — every
            // diagonal below x * band is final, so the launches keep the terms of the band alone)
            if (x >= 1) {
              launch_tree_mid(b, false, x * band, std::min(gmax - 1, x * band + band - 1), x * band, gmax,
                              active(x * band), c->tree_pol, gst);
              c->stats.launches_other++;
            }
          } else {
            if (x + 1 >= 3 && x + 1 < nb) {
              rc = enqueue_mid(false, x + 1, x * band);
              if (rc) return rc;
            }
            if (x >= 3) HIPCHK(hipStreamWaitEvent(gst, gev_b[x % ering], 0));
          }
        }
        const uint32_t thr = sync_in ? x * band : (x >= 3 ? (x - 1) * band : 0u);
        if (lane_mode & 1u) {
          if (d == dmin_in) {  // (the first diagonal's closing-pair blocks: in FRONT of the generic sums below —
            // a batch of four enqueued ahead of it read X4 of this diagonal before it was written, which is
            // what made four diagonals a launch differ under Turner tables, whose first diagonal is 4)
            launch_tlane_inside(b, contra, ~0u, d, gmax, active(d), 0u, gst);
            c->stats.launches_inside++;
          }
          // (the generic 2-loop sums of diagonal d + 1, wanted by this launch's second role: up to three
          // diagonals at once — their slots read X4 up to their own diagonal minus four, i.e. up to d - 1;
          // X4 is complete up to d)
          while (g_next <= d + 1 && g_next < gmax) {
            const uint32_t gc = std::min<uint32_t>(static_cast<uint32_t>(c->tree_gen_batch), gmax - g_next);
            launch_tlane_gen(b, contra, false, g_next, gc, gmax, active(g_next), gst);
            c->stats.launches_inside++;
            g_next += gc;
          }
          launch_tlane_inside(b, contra, d, d + 1 < gmax ? d + 1 : ~0u, gmax, active(d), thr, gst);
          c->stats.launches_inside++;
          d++;
          continue;
        }
        const bool pair = (d % 2u == 0u) && d + 1 < gmax;
        // the next launch's diagonals: their 2-loop blocks' far parts ride in this launch
        const uint32_t nd0 = d + (pair ? 2u : 1u);
        const uint32_t ndc = (!ahead || nd0 >= gmax) ? 0u : ((nd0 % 2u == 0u && nd0 + 1 < gmax) ? 2u : 1u);
        launch_tree_inside(b, contra, d, gmax, active(d), c->tree_tpc, pair, thr, use_far, nd0, ndc, c->tree_pol, gst);
        use_far = ndc != 0u;
        c->stats.launches_inside++;
        d += pair ? 2 : 1;
      }
      if (cur_band != ~0u) {  // the last band's sums_external; the outside sweep reads them
        if (lane_mode) {
          launch_tlane_spread(b, false, cur_band * band, std::min(gmax - 1, cur_band * band + band - 1), gmax,
                              active(cur_band * band), gst);
          c->stats.launches_other++;
        }
        rc = boundary(cur_band + 1);
        if (rc) return rc;
        enqueue_ext(cur_band);
        HIPCHK(hipEventRecord(gev_b[(cur_band + 1) % ering], gbulk));
        HIPCHK(hipStreamWaitEvent(gst, gev_b[(cur_band + 1) % ering], 0));
      }
      if (prof) HIPCHK(hipEventRecord(gev[4 * g + 1], gst));
#ifdef RNAMC_DEBUG_KNOBS
      if (const char* dump = getenv("RNAMC_DUMP_MID")) {  // "<first slot>,<slots>,<path>": after the inside sweep
        int s0 = 0, ns = 1;
        char path[512] = {0};
        if (sscanf(dump, "%d,%d,%500s", &s0, &ns, path) == 3) {
          HIPCHK(hipDeviceSynchronize());
          const TreeSeq& t0 = tseqs[gb];
          std::vector<float> hbuf(static_cast<size_t>(ns) * t0.msz);
          HIPCHK(hipMemcpy(hbuf.data(), b.workspace + t0.ws_off + static_cast<uint64_t>(s0) * t0.msz,
                           hbuf.size() * sizeof(float), hipMemcpyDeviceToHost));
          if (FILE* fh = fopen(path, "wb")) {
            const uint64_t hdr[3] = {t0.n, t0.ld, t0.msz};
            fwrite(hdr, sizeof(hdr), 1, fh);
            fwrite(hbuf.data(), sizeof(float), hbuf.size(), fh);
            fclose(fh);
          }
        }
      }
#endif
      launch_tree_init(b, nseq, gmax, contra, 1, gst);
      c->stats.launches_other++;
      // Outside, from the top: band x takes the terms whose outside operand spans at least
      // thr = (x+2)*band (final once band x+2 is through) from k_tree_mid, enqueued when band x+1
      // starts.  (The first enqueue also orders bulk_stream after the inside sweep's last reads of
      // the ring and after launch_tree_init.)
      int64_t dd = static_cast<int64_t>(gmax) - 1;
      int64_t go_next = static_cast<int64_t>(gmax) - 5;  // (a generic enclosing 2-loop needs n >= d + 5)
      cur_band = ~0u;
      use_far = false;
      while (dd >= static_cast<int64_t>(dmin_out)) {
        const uint32_t du = static_cast<uint32_t>(dd);
        const uint32_t x = du / band;
        if (x != cur_band) {
          if (lane_mode && cur_band != ~0u) {  // (the band above is through: W and R for the mid-field kernels)
            launch_tlane_spread(b, true, cur_band * band, std::min(gmax - 1, cur_band * band + band - 1), gmax,
                                active(cur_band * band), gst);
            c->stats.launches_other++;
          }
          cur_band = x;
          if (sync_out) {
            if ((x + 1) * band < gmax) {  // (operands of span >= (x+1)*band: everything above this band)
              launch_tree_mid(b, true, x * band, std::min(gmax - 1, x * band + band - 1), (x + 1) * band, gmax,
                              active(x * band), c->tree_pol, gst);
              c->stats.launches_other++;
            }
          } else {
            if (x >= 1 && (x + 1) * band < gmax) {  // band x-1 has a mid-field: thr = (x+1)*band <= gmax-1
              rc = boundary(x);
              if (rc) return rc;
              rc = enqueue_mid(true, x - 1, (x + 1) * band);
              if (rc) return rc;
            }
            if ((x + 2) * band < gmax) HIPCHK(hipStreamWaitEvent(gst, gev_b[x % ering], 0));
          }
        }
        const uint32_t thr = sync_out ? ((x + 1) * band < gmax ? (x + 1) * band : 0u)
                                      : ((x + 2) * band < gmax ? (x + 2) * band : 0u);
        if (lane_mode & 2u) {
          // (the generic enclosing 2-loops of diagonal du, wanted by this launch: three diagonals downwards at
          // once — their slots read PX4 from their own diagonal plus four on, i.e. from du + 2)
          while (go_next >= static_cast<int64_t>(du) && go_next >= static_cast<int64_t>(dmin_out)) {
            const uint32_t gc = static_cast<uint32_t>(std::min<int64_t>(c->tree_gen_batch, go_next - static_cast<int64_t>(dmin_out) + 1));
            launch_tlane_gen(b, contra, true, static_cast<uint32_t>(go_next), gc, gmax,
                             active(static_cast<uint32_t>(go_next) - (gc - 1u)), gst);
            c->stats.launches_outside++;
            go_next -= gc;
          }
          if (du == gmax - 1) {  // (the top diagonal's enclosing 2-loops: none exist, the slots are written)
            launch_tlane_outside(b, contra, ~0u, du, gmax, active(du), 0u, gst);
            c->stats.launches_outside++;
          }
          // (sequences that enter the sweep with the next launch need their 2-loop sums too)
          const uint32_t dn = du > dmin_out ? du - 1 : ~0u;
          launch_tlane_outside(b, contra, du, dn, gmax, active(dn != ~0u ? dn : du), thr, gst);
          c->stats.launches_outside++;
          dd--;
          continue;
        }
        const bool pair = du % 2u == 1u && du - 1 >= dmin_out;
        const uint32_t lower = pair ? du - 1 : du;
        // the next launch (below): a pair when its top is odd and both diagonals are swept
        uint32_t nd0 = 0, ndc = 0;
        if (ahead && lower >= dmin_out + 1) {
          const uint32_t top = lower - 1;
          const bool npair = top % 2u == 1u && top - 1 >= dmin_out;
          nd0 = npair ? top - 1 : top;
          ndc = npair ? 2u : 1u;
        }
        // (sequences that enter the sweep with the next launch need their far parts too)
        launch_tree_outside(b, contra, lower, gmax, active(ndc ? nd0 : lower), c->tree_tpc, pair, thr, use_far,
                            nd0, ndc, c->tree_pol, gst);
        use_far = ndc != 0u;
        dd -= pair ? 2 : 1;
        c->stats.launches_outside++;
      }
    } else {
    for (uint32_t d = dmin_in; d < gmax; d += two ? 2 : 1) {
      launch_tree_inside(b, contra, d, gmax, active(d), c->tree_tpc, two, 0u, false, 0u, 0u, c->tree_pol, gst);
      c->stats.launches_inside++;
    }
    if (prof) HIPCHK(hipEventRecord(gev[4 * g + 1], gst));
    launch_tree_init(b, nseq, gmax, contra, 1, gst);
    c->stats.launches_other++;
    if (two) {
      // pairs (d+1, d) from the top; the lowest diagonal alone when their number is odd
      int64_t d = static_cast<int64_t>(gmax) - 1;
      for (; d - 1 >= static_cast<int64_t>(dmin_out); d -= 2) {
        launch_tree_outside(b, contra, static_cast<uint32_t>(d - 1), gmax, active(static_cast<uint32_t>(d - 1)),
                            c->tree_tpc, true, 0u, false, 0u, 0u, c->tree_pol, gst);
        c->stats.launches_outside++;
      }
      if (d >= static_cast<int64_t>(dmin_out)) {
        launch_tree_outside(b, contra, static_cast<uint32_t>(d), gmax, active(static_cast<uint32_t>(d)),
                            c->tree_tpc, false, 0u, false, 0u, 0u, c->tree_pol, gst);
        c->stats.launches_outside++;
      }
    } else
    for (uint32_t d = gmax; d-- > dmin_out;) {
      launch_tree_outside(b, contra, d, gmax, active(d), c->tree_tpc, false, 0u, false, 0u, 0u, c->tree_pol, gst);
      c->stats.launches_outside++;
    }
    }
    if (prof) HIPCHK(hipEventRecord(gev[4 * g + 2], gst));
    launch_tree_finalize(b, nseq, gmax, gst);
    c->stats.launches_other++;
    if (prof) HIPCHK(hipEventRecord(gev[4 * g + 3], gst));
    HIPCHK(hipGetLastError());
    if (hooks) {
      rc = hooks->after(g, gb, nseq);
      if (rc) return rc;
    }
  }
  if (dual) {  // (the caller's stream ends behind the second one)
    HIPCHK(hipEventRecord(c->ev_dual, c->dual_stream));
    HIPCHK(hipStreamWaitEvent(st, c->ev_dual, 0));
  }
#ifdef RNAMC_DEBUG_KNOBS
  if (const char* dump = getenv("RNAMC_DUMP_SLOT")) {  // "<first slot>,<slots>,<path>": the first sequence's matrices, raw
    int s0 = 0, ns = 1;
    char path[512] = {0};
    if (sscanf(dump, "%d,%d,%500s", &s0, &ns, path) == 3 && !tseqs.empty()) {
      HIPCHK(hipDeviceSynchronize());
      const TreeSeq& t0 = tseqs[0];
      std::vector<float> hbuf(static_cast<size_t>(ns) * t0.msz);
      HIPCHK(hipMemcpy(hbuf.data(), c->d_ws + t0.ws_off + static_cast<uint64_t>(s0) * t0.msz, hbuf.size() * sizeof(float),
                       hipMemcpyDeviceToHost));
      if (FILE* fh = fopen(path, "wb")) {
        const uint64_t hdr[3] = {t0.n, t0.ld, t0.msz};
        fwrite(hdr, sizeof(hdr), 1, fh);
        fwrite(hbuf.data(), sizeof(float), hbuf.size(), fh);
        fclose(fh);
      }
    }
  }
#endif
  c->stats.tree_side_stream = static_cast<uint64_t>(c->side_probed ? c->side_verdict : 0);
  return plan.finish(st);
}

}  // namespace rnamc
