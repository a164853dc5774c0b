// rnamc_schedule.h — the launch schedule of the reference-order sweep, free of HIP and of rnamc_ctx.
//
// For one lock-step group the functions below decide which kernel form every diagonal takes, on
// which of two lanes (kMain: the sweep's stream, kAux: the context's second stream) it runs and
// which slot of the two event rings orders it against its neighbours.  They do nothing themselves:
// every decision is a call on a Sink, which may
//   - launch one of the forms of rnamc_device.h (named like its launch_* function, with the
//     arguments that vary; an outside launch also says in which class it is timed: 0 main, 1 tail,
//     2 / 3 small),
//   - record(ring, slot, lane) / wait(lane, ring, slot),
//   - count_inside(n) / count_outside(n): the statistics are stated here, not inferred from the
//     launches (a launch that finds no blocks is counted; see the two exceptions below).
// A sink call returns a status; a schedule returns the first nonzero one.  rnamc_sweep.cpp holds the
// sink that enqueues (HipSink), tests/schedule_host_check.cpp one that records and one that checks
// the rules below on a CPU.
//
// What the kernels need of each other — the rules a schedule has to keep:
//   Inside sweep.  The closing-pair block of diagonal D is a left fold: its early part (hairpin,
//   2-loops) needs the complete pair blocks of diagonals <= D-2, its last (multibranch) term the
//   folds of diagonal D-2.  The folds of diagonal D need the complete pair blocks of diagonals <= D
//   (<= D+1 for the second cell of a two-diagonal launch).  Parts that ride in one launch owe each
//   other nothing.
//     one-diagonal launch d : folds(d) beside the whole pair block of d+1
//     two-diagonal launch d : folds(d, d+1) beside the early part of pair blocks d+2, d+3; their
//                             last term follows in a small launch of its own (pair_tail)
//     latency forms         : folds(d) on kMain beside the pair block of d+1 on kAux — folds(d) need
//                             the pair block of d (kAux, a step before), the pair block of d+1 the
//                             folds of d-1 (kMain, a step before); or both in one launch on kMain.
//                             The eight-chains form completes sums_1ormore_basepairs of diagonal
//                             d-1 in the launch of d (sequences that end at d-1 included); the
//                             combine of the last diagonal follows everything and is not counted.
//                             CONTRAfold: the launch of d-1 may run the sums_rightmost_basepairs
//                             folds of d ahead (flag 4), which the launch of d then consumes (flag 8).
//   Outside sweep, from the top.  Launch d carries probs_multibranch and the pair tail (multibranch
//   half of the pair probabilities) of diagonal d and the pair head (2-loop half) of diagonal d-1:
//   it starts one diagonal early.  Every kernel of launch d needs every kernel of launch d+1,
//   whatever lanes they ran on.
//   Lanes.  A schedule starts and ends on kMain alone: what it put on kAux is ordered behind an
//   event recorded on kMain inside the schedule and before the schedule's last point on kMain (the
//   caller's hooks and launch_finalize run on kMain only).  A wait sees the latest record of its slot:
//   a ring slot is waited for before the ring comes round to it again.
#ifndef RNAMC_SCHEDULE_H
#define RNAMC_SCHEDULE_H

#include <algorithm>
#include <cstdint>

namespace rnamc {

// A copy of every knob the schedule reads (rnamc_ctx.h says what they mean), taken once per call.
struct SweepKnobs {
  int64_t latency_mode, lat_max_cells, lat_inside, lat_pairs, lat_merge, lat_split, lat_zr_ahead, lat_e_waves;
  int64_t fuse_inside, dual_outside;
  uint64_t dual_min_cells;
  int64_t dual_max_diag;
  int64_t debug_roles;    // bit 0 folds, 1 pair blocks, 2 probs_multibranch, 3 pair probabilities
                          // (debug builds: bit 4 drops their 2-loop half, bit 5 the multibranch half)
  int64_t block_threads;  // (for the sink)
  uint32_t ring;          // slots of either event ring
  int64_t profile;        // (for the sink: 2 times every outside kernel)
};

// A lock-step group as the schedule sees it.
struct GroupShape {
  uint32_t gmax, nseq;  // longest sequence, number of sequences
  bool contra;
  uint32_t dmin_in, dmin_out;  // first diagonal of the inside sweep, last of the outside sweep
  const uint32_t* act;         // [0 .. gmax]: sequences with n > d
  uint32_t active(uint32_t d) const { return d <= gmax ? act[d] : 0u; }
};

enum Lane : int { kMain = 0, kAux = 1 };
enum Ring : int { kRingA = 0, kRingB = 1 };

#define RNAMC_SCHED(call)             \
  do {                                \
    if (int rc_ = (call)) return rc_; \
  } while (0)

// true when the folds of diagonal d run in the split form (launch too small to fill the chip)
inline bool inside_is_split(uint32_t d, uint32_t max_n, uint32_t nseq) {
  const uint32_t cells_s = d < max_n ? max_n - d : 0;
  return static_cast<uint64_t>(cells_s) * nseq < 64ull * 1024ull;
}

// A group that cannot fill the chip takes the latency forms (rnamc_latency.h) on every diagonal.
// (CONTRAfold's chains hold more general steps: its crossover against the batch forms lies at half
// the cells, profiles/r02_latency_forms.txt)
inline bool is_latency_group(const SweepKnobs& k, const GroupShape& g) {
  if (k.latency_mode != 1) return k.latency_mode == 2;
  return static_cast<uint64_t>(g.nseq) * g.gmax <=
         static_cast<uint64_t>(g.contra ? k.lat_max_cells / 2 : k.lat_max_cells);
}

// Max-plus sweep (rnamc_mfe_batch): the closing-pair cells of diagonal dmin_in, then per diagonal
// d its sums beside the closing-pair cells of d+1, all on kMain.
template <class Sink>
int schedule_maxplus(const GroupShape& g, Sink& s) {
  RNAMC_SCHED(s.mfe_inside(g.gmax, g.dmin_in, g.nseq));
  for (uint32_t d = g.dmin_in; d < g.gmax; d++) RNAMC_SCHED(s.mfe_inside(d, d + 1, g.active(d)));
  return s.count_inside(g.gmax - g.dmin_in + 1);
}

// The form of the latency-form folds of diagonal d: 2 = eight chains per wave, on the diagonals
// with few enough waves; 0 = three lanes per cell (k_inside's split form).
struct LatForm {
  int form;
  bool zr_ahead;  // CONTRAfold: this launch also runs the sums_rightmost_basepairs folds of d+1
};
inline LatForm lat_inside_form(const SweepKnobs& k, const GroupShape& g, uint32_t d) {
  const uint64_t cells = static_cast<uint64_t>(g.gmax - d) * g.active(d);
  // (CONTRAfold, eight-chains form: two more chain kinds per cell, see lat_zr_ahead)
  const uint64_t kinds = (g.contra && k.lat_zr_ahead != 0) ? 5 : 3;
  // (CONTRAfold: three times the waves — its three-lanes form folds two chains per cell one after
  // the other, measured crossover in profiles/r02_latency_forms.txt)
  const uint64_t e_waves = static_cast<uint64_t>(k.lat_e_waves) * (g.contra ? 3 : 1);
  const bool eight = (k.debug_roles & 1) != 0 && k.lat_inside != 0 && (cells * kinds + 7) / 8 <= e_waves;
  // CONTRAfold: a cell's sums_rightmost_basepairs folds (d steps) precede its other folds (d steps
  // more); all but their last step needs nothing of diagonal d, so the launch of d-1 runs them ahead
  return LatForm{eight ? 2 : 0, eight && kinds == 5};
}

// Latency-form inside sweep.  Un-merged, a step is: pair block of d+1 on kAux behind ring A (the
// folds of d-1), folds of d on kMain behind ring B (the pair block of d).  Merged (eight-chains
// form with lat_pairs and lat_merge), the pair block of d+1 rides in the launch of the folds of d:
// one launch per diagonal, no events (~12 us per diagonal less, profiles/r02_latency_forms.txt).
template <class Sink>
int schedule_inside_lat(const SweepKnobs& k, const GroupShape& g, Sink& s) {
  const bool do_sums = (k.debug_roles & 1) != 0, do_pair = (k.debug_roles & 2) != 0;
  const uint32_t gmax = g.gmax, ring = k.ring;
  if (g.dmin_in >= gmax) return 0;
  if (g.dmin_in >= 1 && do_pair) {  // the pair block of the first diagonal (diagonal 0 has none)
    RNAMC_SCHED(s.inside(kMain, g.dmin_in - 1, g.active(g.dmin_in), false, true));
    RNAMC_SCHED(s.count_inside(1));
  }
  bool have_a = false;  // ring A holds everything enqueued on kMain so far (slot pv)
  bool have_b = false;  // the pair block of d is on kAux (ring B, slot pv)
  bool combine_due = false, zr_parked = false;
  for (uint32_t d = g.dmin_in; d < gmax; d++) {
    const bool pair_next = d + 1 < gmax;
    const uint32_t pv = (d + ring - 1) % ring, cu = d % ring;
    const LatForm f = lat_inside_form(k, g, d);
    const bool wave_form = f.form != 0;
    const int form_arg = f.form | (f.zr_ahead ? 4 : 0) | (wave_form && zr_parked ? 8 : 0);
    const bool merged = wave_form && k.lat_pairs != 0 && k.lat_merge != 0;
    if (pair_next && do_pair && !merged) {
      if (!have_a) {  // everything so far is on kMain
        RNAMC_SCHED(s.record(kRingA, pv, kMain));
        have_a = true;
      }
      RNAMC_SCHED(s.wait(kAux, kRingA, pv));
      if (k.lat_pairs != 0) {
        RNAMC_SCHED(s.pair_lat(kAux, d + 1, g.active(d + 1)));
      } else {
        RNAMC_SCHED(s.inside(kAux, d, g.active(d + 1), false, true));
      }
      RNAMC_SCHED(s.count_inside(1));
    }
    if (have_b) RNAMC_SCHED(s.wait(kMain, kRingB, pv));
    if (do_sums) {
      const uint32_t pair_d = (merged && pair_next && do_pair) ? d + 1 : 0;
      if (wave_form || combine_due) {
        RNAMC_SCHED(s.inside_lat(d, g.active(d >= 1 ? d - 1 : 0), form_arg, combine_due, pair_d));
        RNAMC_SCHED(s.count_inside(1));
      }
      if (!wave_form) {
        RNAMC_SCHED(s.inside(kMain, d, g.active(d), true, false));
        RNAMC_SCHED(s.count_inside(1));
      }
      combine_due = wave_form;
    }
    zr_parked = f.zr_ahead;
    have_a = !merged;  // (merged: recorded when a later diagonal needs it)
    if (!merged) RNAMC_SCHED(s.record(kRingA, cu, kMain));
    have_b = pair_next && !merged;
    if (have_b) RNAMC_SCHED(s.record(kRingB, cu, kAux));
  }
  if (have_b) RNAMC_SCHED(s.wait(kMain, kRingB, (gmax - 1) % ring));
  if (combine_due) RNAMC_SCHED(s.inside_lat(gmax, g.active(gmax - 1), 0, true, 0));  // of the last diagonal
  return 0;
}

// Batch inside sweep: how far the closing-pair blocks have come.  `done`: complete up to this
// diagonal; `heads`: early part parked up to this one (by two-diagonal launches).
template <class Sink>
struct PairBlocks {
  const GroupShape& g;
  Sink& s;
  bool do_pair;
  int64_t done, heads;
  PairBlocks(const GroupShape& shape, Sink& sink, bool pair)
      : g(shape), s(sink), do_pair(pair), done(static_cast<int64_t>(shape.dmin_in) - 1), heads(done) {}
  // nothing pairs below dmin_in

  // does the early part of the pair block of diagonal d still have to run?
  bool unparked(uint32_t d) const { return heads < static_cast<int64_t>(d) && d < g.gmax; }
  // complete the pair blocks of diagonals <= upto: the last term of the parked ones in one launch,
  // the others whole, one launch each
  int complete(int64_t upto) {
    upto = std::min<int64_t>(upto, static_cast<int64_t>(g.gmax) - 1);
    while (done < upto) {
      const uint32_t D = static_cast<uint32_t>(done + 1);
      if (static_cast<int64_t>(D) <= heads) {
        const uint32_t nd = static_cast<uint32_t>(std::min<int64_t>(heads, upto)) - D + 1;
        if (do_pair) {
          RNAMC_SCHED(s.pair_tail(D, nd, g.active(D)));
          RNAMC_SCHED(s.count_inside(1));
        }
        done = D + nd - 1;
      } else {
        if (D >= 1 && do_pair) {
          RNAMC_SCHED(s.inside(kMain, D - 1, g.active(D), false, true));
          RNAMC_SCHED(s.count_inside(1));
        }
        done = heads = D;
      }
    }
    return 0;
  }
};

// Batch inside sweep, all on kMain: two diagonals per launch where the launches are large
// (fuse_inside), one elsewhere.
template <class Sink>
int schedule_inside_batch(const SweepKnobs& k, const GroupShape& g, Sink& s) {
  const bool do_sums = (k.debug_roles & 1) != 0, do_pair = (k.debug_roles & 2) != 0;
  const uint32_t gmax = g.gmax;
  PairBlocks<Sink> pairs(g, s, do_pair);
  for (uint32_t d = g.dmin_in; d < gmax;) {
    const bool fuse = k.fuse_inside != 0 && d >= 2 && d + 1 < gmax && !inside_is_split(d, gmax, g.active(d));
    if (fuse) {
      RNAMC_SCHED(pairs.complete(static_cast<int64_t>(d) + 1));
      const bool head = pairs.unparked(d + 2);
      if (g.contra && do_sums) {
        RNAMC_SCHED(s.inside_zr2(d, g.active(d)));
        RNAMC_SCHED(s.count_inside(1));
      }
      RNAMC_SCHED(s.inside2(d, g.active(d), do_sums, head && do_pair));
      RNAMC_SCHED(s.count_inside(1));
      if (head) pairs.heads = std::min<int64_t>(static_cast<int64_t>(d) + 3, gmax - 1);
      d += 2;
    } else {
      RNAMC_SCHED(pairs.complete(d));
      // the whole pair block of d+1 rides along unless its early part is parked already
      const bool pair_next = pairs.unparked(d + 1);
      RNAMC_SCHED(s.inside(kMain, d, g.active(d), do_sums, pair_next && do_pair));
      RNAMC_SCHED(s.count_inside(1));
      if (pair_next) pairs.done = pairs.heads = d + 1;
      d += 1;
    }
  }
  return 0;
}

template <class Sink>
int schedule_inside(const SweepKnobs& k, const GroupShape& g, Sink& s) {
  if (is_latency_group(k, g) && (k.lat_inside != 0 || k.lat_pairs != 0)) return schedule_inside_lat(k, g, s);
  return schedule_inside_batch(k, g, s);
}

// The role bits of the outside sweep.
struct OutsideRoles {
  bool mb, head, tail;
  explicit OutsideRoles(int64_t debug_roles)
      : mb((debug_roles & 4) != 0),
        head((debug_roles & 8) != 0 && (debug_roles & 16) == 0),
        tail((debug_roles & 8) != 0 && (debug_roles & 32) == 0) {}
};

// Latency-form outside sweep.  Merged (lat_pairs and lat_merge, not lat_split): one launch per
// diagonal on kMain, no events.  Otherwise probs_multibranch and the pair tail of diagonal d on
// kMain (k_outside_lat; lat_split: as two launches that count as one, timed as tail and main)
// beside the pair head of diagonal d-1 on kAux; ring A carries kMain's launch of d, ring B kAux's.
template <class Sink>
int schedule_outside_lat(const SweepKnobs& k, const GroupShape& g, Sink& s) {
  const OutsideRoles r(k.debug_roles);
  const uint32_t gmax = g.gmax, dmin_out = g.dmin_out, ring = k.ring;
  if (k.lat_pairs != 0 && k.lat_merge != 0 && k.lat_split == 0) {
    for (uint32_t d = gmax + 1; d-- > dmin_out;) {
      const bool head = d >= 1 && d - 1 >= dmin_out && r.head;
      if (d < gmax || head) {
        RNAMC_SCHED(s.outside_lat(0, d, g.active(d >= 1 ? d - 1 : 0), r.mb, r.tail, head));
        RNAMC_SCHED(s.count_outside(1));
      }
    }
    return 0;
  }
  if (gmax < dmin_out) return 0;
  for (uint32_t d = gmax + 1; d-- > dmin_out;) {
    const bool head = d >= 1 && d - 1 >= dmin_out;
    const uint32_t na = g.active(d >= 1 ? d - 1 : 0);
    const uint32_t pv = (d + 1) % ring, cu = d % ring;
    if (d == gmax) {  // the first step: everything so far is on kMain
      RNAMC_SCHED(s.record(kRingA, pv, kMain));
    } else {
      RNAMC_SCHED(s.wait(kMain, kRingB, pv));
    }
    RNAMC_SCHED(s.wait(kAux, kRingA, pv));
    if (d < gmax) {
      if (k.lat_split != 0) {
        RNAMC_SCHED(s.outside_lat(1, d, g.active(d), r.mb, false, false));
        RNAMC_SCHED(s.outside_lat(0, d, g.active(d), false, r.tail, false));
      } else {
        RNAMC_SCHED(s.outside_lat(0, d, g.active(d), r.mb, r.tail, false));
      }
      RNAMC_SCHED(s.count_outside(1));
    }
    RNAMC_SCHED(s.record(kRingA, cu, kMain));
    if (head && r.head) {
      if (k.lat_pairs != 0) {
        RNAMC_SCHED(s.outside_pair_lat(3, kAux, d - 1, na));
      } else {
        RNAMC_SCHED(s.outside(3, kAux, d, na, false, false, true, 4));
      }
      RNAMC_SCHED(s.count_outside(1));
    }
    RNAMC_SCHED(s.record(kRingB, cu, kAux));
  }
  return s.wait(kMain, kRingB, dmin_out % ring);
}

// Batch outside sweep.  Large launches run the pair tail as its own kernel on kAux beside the other
// two roles (its register footprint would otherwise set their occupancy): worth it where the
// 2-loop blocks dominate a launch — the folds of a cell grow with the length of the diagonal, its
// 496 probes do not.  Roles: 7 = all three in one kernel, 5 = probs_multibranch + pair head, 2 =
// pair tail.
template <class Sink>
int schedule_outside_batch(const SweepKnobs& k, const GroupShape& g, Sink& s) {
  const OutsideRoles r(k.debug_roles);
  const uint32_t gmax = g.gmax, dmin_out = g.dmin_out, ring = k.ring;
  bool dual = false;  // the previous diagonal ran as two kernels
  for (uint32_t d = gmax + 1; d-- > dmin_out;) {
    const bool head = d >= 1 && d - 1 >= dmin_out;
    const uint32_t na = g.active(d >= 1 ? d - 1 : 0);
    const uint32_t pv = (d + 1) % ring, cu = d % ring;
    const bool want_dual = k.dual_outside != 0 && d < gmax && gmax - d <= static_cast<uint64_t>(k.dual_max_diag) &&
                           static_cast<uint64_t>(gmax - d) * na >= k.dual_min_cells;
    if (!want_dual) {
      if (dual) RNAMC_SCHED(s.wait(kMain, kRingB, pv));  // back to one lane: the other kernel of d+1
      dual = false;
      RNAMC_SCHED(s.outside(2, kMain, d, na, r.mb, r.tail, head && r.head, 7));
      RNAMC_SCHED(s.count_outside(1));
    } else {
      if (!dual) {  // first two-kernel diagonal: everything so far is on kMain
        RNAMC_SCHED(s.record(kRingA, pv, kMain));
      } else {
        RNAMC_SCHED(s.wait(kMain, kRingB, pv));
      }
      RNAMC_SCHED(s.wait(kAux, kRingA, pv));
      RNAMC_SCHED(s.outside(0, kMain, d, na, r.mb, false, head && r.head, 5));
      RNAMC_SCHED(s.record(kRingA, cu, kMain));
      RNAMC_SCHED(s.outside(1, kAux, d, na, false, r.tail, false, 2));
      RNAMC_SCHED(s.record(kRingB, cu, kAux));
      RNAMC_SCHED(s.count_outside(2));
      dual = true;
    }
  }
  if (dual) RNAMC_SCHED(s.wait(kMain, kRingB, dmin_out % ring));
  return 0;
}

template <class Sink>
int schedule_outside(const SweepKnobs& k, const GroupShape& g, Sink& s) {
  return is_latency_group(k, g) ? schedule_outside_lat(k, g, s) : schedule_outside_batch(k, g, s);
}

#undef RNAMC_SCHED

}  // namespace rnamc

#endif
