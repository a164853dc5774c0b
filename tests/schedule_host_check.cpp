// schedule_host_check.cpp — the launch schedule of the reference-order sweep
// (rna_algos_amd/csrc/rnamc_schedule.h) driven without a device, by two sinks of its own.
//
//  * RecSink writes one text line per sink call.  For every case of the grid the program prints
//    the number of sink calls, the statistics, the timed outside launches per class and a digest
//    (FNV-1a, 64 bits) of the trace; tests/test_schedule_cpu.py holds the lines of the cases marked
//    for the fixture against tests/golden/sweep_schedule.txt.  `--dump <case>` prints a whole trace.
//  * CheckSink decides from the steps alone whether the schedule is safe: it keeps, per lane, how
//    far into either lane the lane's next step is ordered (program order, and record -> wait edges
//    where a wait binds to the LATEST record of its slot when it is enqueued, as HIP does), every
//    launch declares what it writes and reads in units of (role, diagonal), and every read must be
//    ordered after its producer.  The rules are the ones stated next to the schedule functions.
//
// Built with the address and undefined-behaviour sanitizers and run as a plain program.  A line
// starts with "G" where tests/test_gpu_schedule_counts.py runs the case on the card, "F" for the
// other fixture cases and "-" for the rest of the grid (checked, not recorded in the fixture).
#include <algorithm>
#include <cinttypes>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../rna_algos_amd/csrc/rnamc_schedule.h"

using namespace rnamc;

static int g_fails = 0;
static std::string g_case;  // the running case, for messages
#define CHECK(cond, ...)                                          \
  do {                                                            \
    if (!(cond)) {                                                \
      if (g_fails < 200) {                                        \
        std::printf("FAIL %s: %s: ", g_case.c_str(), #cond);      \
        std::printf(__VA_ARGS__);                                 \
        std::printf("\n");                                        \
      }                                                           \
      g_fails++;                                                  \
    }                                                             \
  } while (0)

// ---- the recording sink --------------------------------------------------------------------------

struct RecSink {
  bool keep = false;  // --dump: keep the lines
  std::vector<std::string> lines;
  uint64_t digest = 1469598103934665603ull, steps = 0;
  uint64_t launches_inside = 0, launches_outside = 0, cls[4] = {0, 0, 0, 0};

  int line(const char* fmt, ...) __attribute__((format(printf, 2, 3))) {
    char buf[160];
    va_list ap;
    va_start(ap, fmt);
    const int n = std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    for (int x = 0; x < n; x++) digest = (digest ^ static_cast<uint8_t>(buf[x])) * 1099511628211ull;
    digest = (digest ^ static_cast<uint8_t>('\n')) * 1099511628211ull;
    steps++;
    if (keep) lines.emplace_back(buf);
    return 0;
  }
  static char ring(Ring r) { return r == kRingA ? 'A' : 'B'; }

  int record(Ring r, uint32_t slot, Lane l) { return line("record %c%u lane=%d", ring(r), slot, l); }
  int wait(Lane l, Ring r, uint32_t slot) { return line("wait %c%u lane=%d", ring(r), slot, l); }
  int count_inside(uint32_t n) {
    launches_inside += n;
    return line("count inside %u", n);
  }
  int count_outside(uint32_t n) {
    launches_outside += n;
    return line("count outside %u", n);
  }
  int mfe_inside(uint32_t d_sums, uint32_t d_pair, uint32_t nseq) {
    return line("mfe_inside sums=%u pair=%u n=%u lane=0", d_sums, d_pair, nseq);
  }
  int inside(Lane l, uint32_t d, uint32_t nseq, bool do_sums, bool do_pair) {
    return line("inside d=%u n=%u sums=%d pair=%d lane=%d", d, nseq, do_sums, do_pair, l);
  }
  int inside2(uint32_t d, uint32_t nseq, bool do_sums, bool do_head) {
    return line("inside2 d=%u n=%u sums=%d head=%d lane=0", d, nseq, do_sums, do_head);
  }
  int inside_zr2(uint32_t d, uint32_t nseq) { return line("inside_zr2 d=%u n=%u lane=0", d, nseq); }
  int pair_tail(uint32_t d0, uint32_t nd, uint32_t nseq) {
    return line("pair_tail d=%u nd=%u n=%u lane=0", d0, nd, nseq);
  }
  int inside_lat(uint32_t d, uint32_t nseq, int form, bool do_combine, uint32_t pair_d) {
    return line("inside_lat d=%u n=%u form=%d combine=%d pair_d=%u lane=0", d, nseq, form, do_combine, pair_d);
  }
  int pair_lat(Lane l, uint32_t d, uint32_t nseq) { return line("pair_lat inside d=%u n=%u lane=%d", d, nseq, l); }
  int outside(uint8_t c, Lane l, uint32_t d, uint32_t nseq, bool do_mb, bool do_tail, bool do_head, int roles) {
    cls[c]++;
    return line("outside d=%u n=%u mb=%d tail=%d head=%d roles=%d lane=%d class=%u", d, nseq, do_mb, do_tail,
                do_head, roles, l, c);
  }
  int outside_lat(uint8_t c, uint32_t d, uint32_t nseq, bool do_mb, bool do_tail, bool head) {
    cls[c]++;
    return line("outside_lat d=%u n=%u mb=%d tail=%d head=%d lane=0 class=%u", d, nseq, do_mb, do_tail, head, c);
  }
  int outside_pair_lat(uint8_t c, Lane l, uint32_t d, uint32_t nseq) {
    cls[c]++;
    return line("pair_lat outside d=%u n=%u lane=%d class=%u", d, nseq, l, c);
  }
};

// ---- the checking sink ---------------------------------------------------------------------------

enum Role : int {
  R_FOLDS,       // the folds of a diagonal (inside)
  R_PAIR_EARLY,  // early part of its closing-pair block: hairpin, 2-loops
  R_PAIR_LAST,   // last (multibranch) term of its closing-pair block
  R_COMBINE,     // eight-chains form: sums_1ormore_basepairs of the diagonal completed
  R_ZR,          // CONTRAfold: sums_rightmost_basepairs of the diagonal, run ahead of its other folds
  R_MB,          // probs_multibranch (outside)
  R_TAIL,        // multibranch half of the pair probabilities
  R_HEAD,        // 2-loop half of the pair probabilities
  R_COUNT
};
static const char* const kRoleName[R_COUNT] = {"folds", "pair-early", "pair-last", "combine",
                                               "zr",    "mb",         "tail",      "head"};

struct CheckSink {
  struct Stamp {
    uint32_t seen[2];  // ordered after the first seen[l] steps of lane l
  };
  struct Producer {
    int lane = -1;
    uint32_t pos = 0;  // 1-based position in its lane
    uint32_t times = 0, reads = 0;
  };
  const GroupShape& g;
  uint32_t ring;
  uint32_t count[2] = {0, 0};  // steps enqueued per lane
  Stamp cur[2] = {{{0, 0}}, {{0, 0}}};
  std::vector<Stamp> slot[2];
  std::vector<bool> slot_set[2];
  std::vector<Producer> prod[R_COUNT];
  uint64_t launches_inside = 0, launches_outside = 0;  // what the schedule states
  uint64_t counted_inside = 0, counted_outside = 0;    // what the steps say (see the two exceptions)
  // the launch being declared
  Lane at = kMain;
  uint32_t main_floor = 0;  // an aux step must be ordered after this many steps of the main lane

  CheckSink(const GroupShape& shape, uint32_t ring_size) : g(shape), ring(ring_size) {
    for (int r = 0; r < 2; r++) {
      slot[r].assign(ring, Stamp{{0, 0}});
      slot_set[r].assign(ring, false);
    }
    for (auto& p : prod) p.assign(static_cast<size_t>(g.gmax) + 2, Producer{});
  }

  // ---- ordering
  void step(Lane l) {
    at = l;
    count[l]++;
    if (l == kAux)
      CHECK(cur[kAux].seen[kMain] >= main_floor, "aux step %u is not ordered after main step %u", count[l], main_floor);
  }
  void done(Lane l) { cur[l].seen[l] = count[l]; }
  int record(Ring r, uint32_t s, Lane l) {
    CHECK(s < ring, "slot %u", s);
    count[l]++;
    done(l);
    slot[r][s] = cur[l];
    slot_set[r][s] = true;
    return 0;
  }
  int wait(Lane l, Ring r, uint32_t s) {
    CHECK(s < ring, "slot %u", s);
    CHECK(slot_set[r][s], "lane %d waits for ring %d slot %u that nothing of this group recorded", l, r, s);
    count[l]++;
    done(l);
    for (int x = 0; x < 2; x++) cur[l].seen[x] = std::max(cur[l].seen[x], slot[r][s].seen[x]);
    return 0;
  }
  // a point of the main lane that stands for work of the caller's (the hooks, launch_finalize)
  void main_point() {
    count[kMain]++;
    done(kMain);
  }
  void aux_joined(const char* where) {
    CHECK(cur[kMain].seen[kAux] >= count[kAux], "%s: %u aux steps, the main lane is ordered after %u", where,
          count[kAux], cur[kMain].seen[kAux]);
  }

  // ---- what a launch writes and reads
  bool live(Role r, int64_t d) const {
    if (d < 0 || d >= static_cast<int64_t>(g.gmax)) return false;
    if (r >= R_MB) return d >= g.dmin_out;
    return d >= g.dmin_in;
  }
  void writes(Role r, int64_t d) {
    CHECK(live(r, d), "%s of diagonal %" PRId64 " is outside the sweep", kRoleName[r], d);
    if (!live(r, d)) return;
    Producer& p = prod[r][d];
    p.lane = at;
    p.pos = count[at];
    p.times++;
  }
  void reads(Role r, int64_t d) {
    if (!live(r, d)) return;  // k_init's values
    Producer& p = prod[r][d];
    p.reads++;
    CHECK(p.times > 0, "%s of diagonal %" PRId64 " read before anything wrote it", kRoleName[r], d);
    if (p.times == 0) return;
    const bool beside = p.lane == at && p.pos == count[at];
    CHECK(!beside, "%s of diagonal %" PRId64 " read by the launch that writes it", kRoleName[r], d);
    const bool ordered = p.lane == at ? p.pos < count[at] : p.pos <= cur[at].seen[p.lane];
    CHECK(ordered, "lane %d step %u reads %s of diagonal %" PRId64 " (lane %d step %u), ordered after %u", at,
          count[at], kRoleName[r], d, p.lane, p.pos, cur[at].seen[p.lane]);
  }
  void reads_pairs_upto(int64_t d) {  // the complete pair blocks of diagonals <= d
    for (int64_t x = std::max<int64_t>(g.dmin_in, 1); x <= d; x++) {
      reads(R_PAIR_EARLY, x);
      reads(R_PAIR_LAST, x);
    }
  }
  void folds(uint32_t d, uint32_t pairs_upto) {
    writes(R_FOLDS, d);
    reads_pairs_upto(pairs_upto);
  }
  void pair_early(uint32_t d) {
    writes(R_PAIR_EARLY, d);
    reads_pairs_upto(static_cast<int64_t>(d) - 2);
  }
  void pair_last(uint32_t d) {
    writes(R_PAIR_LAST, d);
    reads(R_FOLDS, static_cast<int64_t>(d) - 2);
  }

  int count_inside(uint32_t n) {
    launches_inside += n;
    return 0;
  }
  int count_outside(uint32_t n) {
    launches_outside += n;
    return 0;
  }

  int mfe_inside(uint32_t d_sums, uint32_t d_pair, uint32_t) {
    step(kMain);
    counted_inside++;
    if (d_pair < g.gmax) {
      writes(R_PAIR_EARLY, d_pair);  // (the max-plus sweep's pair cells start at dmin_in, diagonal 0 included)
      reads_pairs_upto(static_cast<int64_t>(d_pair) - 2);
      pair_last(d_pair);
    }
    if (d_sums < g.gmax) folds(d_sums, d_sums);
    done(kMain);
    return 0;
  }
  int inside(Lane l, uint32_t d, uint32_t, bool do_sums, bool do_pair) {
    step(l);
    counted_inside++;
    if (do_pair && d + 1 < g.gmax) {
      pair_early(d + 1);
      pair_last(d + 1);
    }
    if (do_sums && d < g.gmax) folds(d, d);
    done(l);
    return 0;
  }
  int inside2(uint32_t d, uint32_t, bool do_sums, bool do_head) {
    step(kMain);
    counted_inside++;
    CHECK(d + 1 < g.gmax, "two-diagonal launch at %u", d);
    if (do_head)
      for (uint32_t x = d + 2; x <= d + 3 && x < g.gmax; x++) pair_early(x);
    if (do_sums) {
      if (g.contra) {
        reads(R_ZR, d);
        reads(R_ZR, d + 1);
      }
      folds(d, d);
      folds(d + 1, d + 1);
    }
    done(kMain);
    return 0;
  }
  int inside_zr2(uint32_t d, uint32_t) {
    step(kMain);
    counted_inside++;
    CHECK(g.contra && d + 1 < g.gmax, "inside_zr2 at %u", d);
    writes(R_ZR, d);
    writes(R_ZR, d + 1);
    reads_pairs_upto(static_cast<int64_t>(d) + 1);
    done(kMain);
    return 0;
  }
  int pair_tail(uint32_t d0, uint32_t nd, uint32_t) {
    step(kMain);
    counted_inside++;
    for (uint32_t d = d0; d < d0 + nd && d < g.gmax; d++) {
      reads(R_PAIR_EARLY, d);
      pair_last(d);
    }
    done(kMain);
    return 0;
  }
  int inside_lat(uint32_t d, uint32_t, int form, bool do_combine, uint32_t pair_d) {
    step(kMain);
    if (d < g.gmax) counted_inside++;  // (the combine of the last diagonal is not counted)
    if (pair_d != 0 && pair_d < g.gmax) {
      pair_early(pair_d);
      pair_last(pair_d);
    }
    if (do_combine && d >= 1) {
      writes(R_COMBINE, d - 1);
      reads(R_FOLDS, d - 1);
    }
    if ((form & 3) && d < g.gmax) {
      if (form & 8) reads(R_ZR, d);
      folds(d, d);
      if ((form & 4) && d + 1 < g.gmax) {
        writes(R_ZR, d + 1);
        reads_pairs_upto(d);
      }
      eight_chains.push_back(d);
    } else {
      CHECK((form & 12) == 0, "flags %d without the eight-chains form", form);
    }
    if (d == g.gmax) aux_joined("combine of the last diagonal");
    done(kMain);
    return 0;
  }
  int pair_lat(Lane l, uint32_t d, uint32_t) {
    step(l);
    counted_inside++;
    pair_early(d);
    pair_last(d);
    done(l);
    return 0;
  }

  // outside: launch d carries probs_multibranch and the pair tail of diagonal d and the pair head of
  // diagonal d-1; every kernel of launch d needs every kernel of launch d+1
  void outside_roles(uint32_t d, bool mb, bool tail, bool head) {
    if (d < g.gmax) {
      if (mb) writes(R_MB, d);
      if (tail) writes(R_TAIL, d);
    }
    if (head) writes(R_HEAD, static_cast<int64_t>(d) - 1);
    reads(R_MB, static_cast<int64_t>(d) + 1);
    reads(R_TAIL, static_cast<int64_t>(d) + 1);
    reads(R_HEAD, d);  // (carried by launch d+1)
  }
  int outside(uint8_t c, Lane l, uint32_t d, uint32_t, bool do_mb, bool do_tail, bool do_head, int roles) {
    step(l);
    counted_outside++;
    CHECK(c == (roles == 7 ? 2 : roles == 5 ? 0 : roles == 2 ? 1 : 3), "class %u of roles %d", c, roles);
    CHECK(!(do_mb && !(roles & 1)) && !(do_tail && !(roles & 2)) && !(do_head && !(roles & 4)), "roles %d", roles);
    outside_roles(d, do_mb, do_tail, do_head);
    done(l);
    return 0;
  }
  int outside_lat(uint8_t c, uint32_t d, uint32_t, bool do_mb, bool do_tail, bool head) {
    step(kMain);
    if (c != 1) counted_outside++;  // (lat_split: the two launches of a diagonal count as one)
    outside_roles(d, do_mb, do_tail, head);
    done(kMain);
    return 0;
  }
  int outside_pair_lat(uint8_t, Lane l, uint32_t d, uint32_t) {
    step(l);
    counted_outside++;
    outside_roles(d + 1, false, false, true);
    done(l);
    return 0;
  }

  std::vector<uint32_t> eight_chains;  // diagonals whose folds ran in the eight-chains form

  // ---- after a schedule: every role once on every diagonal of its range, nothing below
  void covered(Role r, uint32_t lo, const char* what) {
    for (uint32_t d = 0; d < g.gmax; d++) {
      const uint32_t want = d >= lo ? 1u : 0u;
      CHECK(prod[r][d].times == want, "%s: %s of diagonal %u written %u times", what, kRoleName[r], d,
            prod[r][d].times);
    }
  }
  void end_inside(bool maxplus) {
    aux_joined("end of the inside schedule");
    covered(R_FOLDS, g.dmin_in, "inside");
    const uint32_t pair_lo = maxplus ? g.dmin_in : std::max(g.dmin_in, 1u);
    covered(R_PAIR_EARLY, pair_lo, "inside");
    covered(R_PAIR_LAST, pair_lo, "inside");
    std::vector<uint32_t> want(g.gmax + 1u, 0u);
    for (uint32_t d : eight_chains) want[d] = 1;
    for (uint32_t d = 0; d < g.gmax; d++) {
      CHECK(prod[R_COMBINE][d].times == want[d], "combine of diagonal %u: %u times", d, prod[R_COMBINE][d].times);
      // a parked diagonal is consumed by exactly its own launch
      CHECK(prod[R_ZR][d].times <= 1 && prod[R_ZR][d].reads == prod[R_ZR][d].times, "zr of diagonal %u: %u / %u",
            d, prod[R_ZR][d].times, prod[R_ZR][d].reads);
    }
    // the max-plus sweep states gmax - dmin_in + 1, in 32 bits, whatever it launched: the count of a
    // group with gmax < dmin_in (Turner, fewer than 4 bases) is not the single launch it made
    if (maxplus) CHECK(launches_inside == static_cast<uint32_t>(g.gmax - g.dmin_in + 1), "max-plus count");
    if (!maxplus || g.gmax >= g.dmin_in)
      CHECK(launches_inside == counted_inside, "launches_inside %" PRIu64 ", counted steps %" PRIu64, launches_inside,
            counted_inside);
  }
  void end_outside() {
    aux_joined("end of the outside schedule");
    covered(R_MB, g.dmin_out, "outside");
    covered(R_TAIL, g.dmin_out, "outside");
    covered(R_HEAD, g.dmin_out, "outside");
    CHECK(launches_outside == counted_outside, "launches_outside %" PRIu64 ", counted steps %" PRIu64,
          launches_outside, counted_outside);
  }
};

// ---- the grid ------------------------------------------------------------------------------------

struct Shape {
  std::string name;
  std::vector<uint32_t> lens;  // longest first
  std::vector<uint32_t> act;
  bool in_fixture;
};

static Shape make_shape(const std::string& name, std::vector<uint32_t> lens, bool in_fixture = false) {
  std::sort(lens.begin(), lens.end(), [](uint32_t a, uint32_t b) { return a > b; });
  Shape s{name, lens, {}, in_fixture};
  s.act.assign(lens[0] + 1u, 0u);
  for (uint32_t d = 0; d <= lens[0]; d++)
    for (uint32_t n : lens) s.act[d] += n > d ? 1u : 0u;
  return s;
}

static std::string lens_spec(const std::vector<uint32_t>& lens) {
  std::string out;
  for (size_t x = 0; x < lens.size();) {
    size_t y = x;
    while (y < lens.size() && lens[y] == lens[x]) y++;
    if (!out.empty()) out += ',';
    out += std::to_string(lens[x]);
    if (y - x > 1) out += "x" + std::to_string(y - x);
    x = y;
  }
  return out;
}

// the context's defaults (rnamc_ctx.h; the cases marked G hold them against the library itself)
static SweepKnobs default_knobs() {
  SweepKnobs k{};
  k.latency_mode = 1;
  k.lat_max_cells = 32768;
  k.lat_inside = 2;
  k.lat_pairs = 1;
  k.lat_merge = 1;
  k.lat_split = 0;
  k.lat_zr_ahead = 1;
  k.lat_e_waves = 2048;
  k.fuse_inside = 1;
  k.dual_outside = 1;
  k.dual_min_cells = 256 * 1024;
  k.dual_max_diag = 1 << 30;
  k.debug_roles = 15;
  k.block_threads = 256;
  k.ring = 16;
  k.profile = 2;
  return k;
}

typedef std::vector<std::pair<std::string, int64_t>> KnobSet;

static void apply(SweepKnobs& k, const KnobSet& set) {
  for (const auto& kv : set) {
    const std::string& n = kv.first;
    const int64_t v = kv.second;
    if (n == "latency_mode") k.latency_mode = v;
    else if (n == "lat_max_cells") k.lat_max_cells = v;
    else if (n == "lat_inside") k.lat_inside = v;
    else if (n == "lat_pairs") k.lat_pairs = v;
    else if (n == "lat_merge") k.lat_merge = v;
    else if (n == "lat_split") k.lat_split = v;
    else if (n == "lat_zr_ahead") k.lat_zr_ahead = v;
    else if (n == "lat_e_waves") k.lat_e_waves = v;
    else if (n == "fuse_inside") k.fuse_inside = v;
    else if (n == "dual_outside") k.dual_outside = v;
    else if (n == "dual_min_cells") k.dual_min_cells = static_cast<uint64_t>(v);
    else if (n == "dual_max_diag") k.dual_max_diag = v;
    else {
      std::printf("FAIL unknown knob %s\n", n.c_str());
      g_fails++;
    }
  }
}

static std::string knobs_name(const KnobSet& set) {
  if (set.empty()) return "-";
  std::string out;
  for (const auto& kv : set) out += (out.empty() ? "" : ",") + kv.first + "=" + std::to_string(kv.second);
  return out;
}

// every value the GPU suite sets (tests/knob_table.py), each against the defaults and under either
// forced form, and the knobs that interact as products
static std::vector<KnobSet> knob_sets(uint32_t nseq, uint32_t gmax) {
  const int64_t cells = static_cast<int64_t>(nseq) * gmax;
  std::vector<KnobSet> singles = {{}};
  auto vary = [&](const char* name, std::initializer_list<int64_t> values) {
    for (int64_t v : values) singles.push_back({{name, v}});
  };
  vary("lat_inside", {0});
  vary("lat_pairs", {0});
  vary("lat_merge", {0});
  vary("lat_split", {1});
  vary("lat_zr_ahead", {0});
  vary("lat_e_waves", {0, 64, 200});
  vary("fuse_inside", {0});
  vary("dual_outside", {0});
  vary("dual_min_cells", {0, 2000, 4096});
  vary("dual_max_diag", {37, 90});
  std::vector<KnobSet> out;
  for (int64_t mode : {1, 0, 2})
    for (const KnobSet& s : singles) {
      KnobSet set;
      if (mode != 1) set.push_back({"latency_mode", mode});
      set.insert(set.end(), s.begin(), s.end());
      out.push_back(set);
    }
  // the crossover of latency_mode 1 (halved under CONTRAfold), un-merged so that the forms differ
  for (int64_t v : {cells, cells - 1, 2 * cells, 2 * cells - 1, int64_t{750}}) {
    out.push_back({{"lat_max_cells", v}});
    out.push_back({{"lat_max_cells", v}, {"lat_merge", 0}});
  }
  for (int64_t pairs : {0, 1})
    for (int64_t merge : {0, 1})
      for (int64_t split : {0, 1})
        for (int64_t inside : {0, 2})
          out.push_back({{"latency_mode", 2}, {"lat_pairs", pairs}, {"lat_merge", merge}, {"lat_split", split},
                         {"lat_inside", inside}});
  for (int64_t waves : {0, 64, 200, 2048})
    for (int64_t inside : {0, 2})
      for (int64_t zr : {0, 1})
        out.push_back({{"latency_mode", 2}, {"lat_inside", inside}, {"lat_e_waves", waves}, {"lat_zr_ahead", zr},
                       {"lat_merge", 0}});
  for (int64_t min_cells : {0, 2000, 4096, 256 * 1024})
    for (int64_t max_diag : {37, 90, 1 << 30})
      out.push_back({{"latency_mode", 0}, {"dual_min_cells", min_cells}, {"dual_max_diag", max_diag}});
  return out;
}

struct Model {
  const char* name;
  bool contra, allows_short;
};
static const Model kModels[3] = {{"turner", false, false}, {"contra", true, false}, {"contra-short", true, true}};
static const char* const kOpts[3] = {"full", "inside_only", "maxplus"};
static const uint32_t kSpan = 5;  // RNAMC_MIN_SPAN_HAIRPIN_CLOSE (include/rnamc.h)
// the knob sets whose traces the fixture holds: either form forced, the two-lane latency schedules (a
// ring of 16 wraps on gmax 17 and 120), the eight-chains crossover, and the batch forms unfused, with
// two kernels on every outside diagonal and with a window of them
static const char* const kFixtureKnobs[] = {
    "latency_mode=0", "latency_mode=2", "latency_mode=2,lat_merge=0", "latency_mode=2,lat_split=1",
    "latency_mode=2,lat_pairs=0", "latency_mode=2,lat_e_waves=64", "latency_mode=0,fuse_inside=0",
    "latency_mode=0,dual_min_cells=0", "latency_mode=0,dual_min_cells=2000,dual_max_diag=37"};

template <class Sink>
static int drive(const SweepKnobs& k, const GroupShape& g, int opts, Sink& s, CheckSink* chk) {
  if (opts == 2) {
    if (int rc = schedule_maxplus(g, s)) return rc;
    if (chk) chk->end_inside(true);
    return 0;
  }
  if (int rc = schedule_inside(k, g, s)) return rc;
  if (chk) {
    chk->end_inside(false);
    chk->main_point();  // the `mid` hook
    chk->main_floor = chk->count[kMain];
  }
  if (opts == 0) {
    if (int rc = schedule_outside(k, g, s)) return rc;
    if (chk) chk->end_outside();
  }
  return 0;
}

int main(int argc, char** argv) {
  const char* dump = (argc == 3 && std::strcmp(argv[1], "--dump") == 0) ? argv[2] : nullptr;
  if (argc != 1 && !dump) {
    std::fprintf(stderr, "usage: %s [--dump <case>]\n", argv[0]);
    return 2;
  }
  std::vector<Shape> shapes;
  // gmax around RNAMC_MIN_SPAN_HAIRPIN_CLOSE (1 .. 7; 3: the max-plus count at gmax < dmin_in), around the ring of 16 (15 .. 18, 33), and 120
  const uint32_t ragged_pool[] = {1, 2, 5, 64, 65, 3, 4, 6, 7, 9, 12, 15, 16, 17, 18, 20, 25, 33, 33, 47, 90, 100, 119};
  for (uint32_t gmax : {1u, 2u, 3u, 4u, 5u, 6u, 7u, 15u, 16u, 17u, 18u, 33u, 120u}) {
    shapes.push_back(make_shape("equal" + std::to_string(gmax), std::vector<uint32_t>(6, gmax), gmax == 17));
    std::vector<uint32_t> lens = {gmax};
    for (uint32_t n : ragged_pool)
      if (n <= gmax) lens.push_back(n);
    shapes.push_back(make_shape("ragged" + std::to_string(gmax), lens, gmax == 120));
  }
  // cells * nseq >= 65 536 on the low diagonals: the fused and the unfused batch forms, k_inside2 heads
  shapes.push_back(make_shape("wide120", std::vector<uint32_t>(700, 120), true));
  // the 41 lengths of tests/test_gpu_knob_forms.py, ragged_lens()
  shapes.push_back(make_shape("ragged41", {330, 322, 322, 322, 308, 308, 305, 304, 298, 293, 292, 290, 285, 277,
                                           276, 270, 266, 265, 264, 264, 262, 258, 257, 256, 255, 221, 202, 192,
                                           186, 174, 129, 128, 112, 101, 94,  65,  64,  36,  5,   2,   1}));
  shapes.push_back(make_shape("equal120x3", std::vector<uint32_t>(3, 120)));
  shapes.push_back(make_shape("equal90x3", std::vector<uint32_t>(3, 90)));
  // the cases tests/test_gpu_schedule_counts.py runs on the card
  const std::vector<std::string> gpu_cases = {
      "equal120/turner/full/-",
      "equal120/turner/full/latency_mode=0",
      "equal120/turner/full/latency_mode=2,lat_merge=0",
      "equal120/turner/full/lat_split=1",
      "ragged41/turner/full/latency_mode=0,dual_min_cells=2000,dual_max_diag=90",
      "equal120x3/contra/full/-",
      "equal90x3/contra/full/-",
      "equal120/contra-short/full/-",
      "equal120/turner/maxplus/-",
  };
  std::vector<bool> gpu_found(gpu_cases.size(), false);

  uint64_t n_cases = 0;
  bool dumped = false;
  for (const Shape& sh : shapes)
    for (const Model& m : kModels)
      for (int opts = 0; opts < 3; opts++) {
        const uint32_t gmax = sh.lens[0], nseq = static_cast<uint32_t>(sh.lens.size());
        const GroupShape g{gmax, nseq, m.contra, m.contra ? 0u : kSpan - 1, (m.contra && m.allows_short) ? 1u : kSpan - 1,
                           sh.act.data()};
        std::vector<KnobSet> sets = knob_sets(nseq, gmax);
        if (opts == 2) sets.resize(1);  // the max-plus sweep reads no knob
        for (const KnobSet& set : sets) {
          SweepKnobs k = default_knobs();
          apply(k, set);
          g_case = sh.name + "/" + m.name + "/" + kOpts[opts] + "/" + knobs_name(set);
          if (dump && g_case != dump) continue;
          n_cases++;
          CheckSink chk(g, k.ring);
          CHECK(drive(k, g, opts, chk, &chk) == 0, "status");
          RecSink rec;
          rec.keep = dump && g_case == dump;
          CHECK(drive(k, g, opts, rec, nullptr) == 0, "status");
          CHECK(rec.launches_inside == chk.launches_inside && rec.launches_outside == chk.launches_outside, "counts");
          if (rec.keep) {
            for (const std::string& ln : rec.lines) std::printf("%s\n", ln.c_str());
            dumped = true;
          }
          // the fixture: three shapes under the default knobs and, for the full sweep, under kFixtureKnobs
          const std::string kn = knobs_name(set);
          const bool listed = std::find(std::begin(kFixtureKnobs), std::end(kFixtureKnobs), kn) != std::end(kFixtureKnobs);
          char mark = sh.in_fixture && (set.empty() || (opts == 0 && listed)) ? 'F' : '-';
          for (size_t x = 0; x < gpu_cases.size(); x++)
            if (gpu_cases[x] == g_case) {
              mark = 'G';
              gpu_found[x] = true;
            }
          if (!dump)
            std::printf("%c %s lens=%s steps=%" PRIu64 " inside=%" PRIu64 " outside=%" PRIu64
                        " other=%d main=%" PRIu64 " tail=%" PRIu64 " small=%" PRIu64 " digest=%016" PRIx64 "\n",
                        mark, g_case.c_str(), lens_spec(sh.lens).c_str(), rec.steps, rec.launches_inside,
                        rec.launches_outside, opts == 2 ? 1 : 2, rec.cls[0], rec.cls[1], rec.cls[2] + rec.cls[3],
                        rec.digest);
        }
      }
  g_case = "grid";
  if (dump) {
    if (!dumped) std::fprintf(stderr, "no such case: %s\n", dump);
    return dumped ? 0 : 2;
  }
  for (size_t x = 0; x < gpu_cases.size(); x++) CHECK(gpu_found[x], "%s is not in the grid", gpu_cases[x].c_str());
  std::printf("cases %" PRIu64 "\n", n_cases);
  std::printf(g_fails ? "FAILED %d\n" : "OK\n", g_fails);
  return g_fails ? 1 : 0;
}
