// rnamc_ctx.h — the device context behind the C ABI and what the host translation units that work
// on it share: rnamc_ctx.cpp (life cycle, knobs, statistics), rnamc_sweep.cpp (batch plan and the
// reference-order sweep), rnamc_sweep_tree.cpp (tree-order sweep), rnamc_entries.cpp (the entries).
#ifndef RNAMC_CTX_H
#define RNAMC_CTX_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <atomic>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include "rnamc_device.h"
#include "rnamc_scoring.h"

#define HIPCHK(expr)                                                                       \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess) {                                                                \
      rnamc::set_last_error(std::string(#expr) + ": " + hipGetErrorString(_e));                   \
      (void)hipGetLastError(); /* reported: a later call must not find it again */         \
      return (_e == hipErrorOutOfMemory) ? RNAMC_ERR_OOM : RNAMC_ERR_HIP;                  \
    }                                                                                      \
  } while (0)

// Options of one sweep; the defaults are the unconstrained full sweep.
struct SweepOpts {
  bool inside_only = false;  // no outside sweep (reference order whatever summation_mode says)
  bool maxplus = false;      // with inside_only: the max-plus sweep alone (rnamc_mfe_batch)
  const int32_t* cons = nullptr;  // staged constraint words (two per base, laid out like the bases)
  uint32_t max_span = 0xffffffffu;
};

struct rnamc_ctx {
  int device = 0;
  rnamc_params host_params;
  rnamc_params* d_params = nullptr;
  float* d_hp_init = nullptr;
  std::vector<float> h_hp_init;  // host copy, for rnamc_fold_scores
  uint32_t hp_init_len = 0;
  float* d_ws = nullptr;
  uint64_t ws_floats = 0;
  rnamc::SeqDesc* d_seqs = nullptr;
  uint64_t seqs_cap = 0;
  rnamc::TreeSeq* d_tseqs = nullptr;  // descriptors of the tree-order mode
  uint64_t tseqs_cap = 0;
  std::vector<rnamc::TreeSeq> h_tseqs;  // (host copy: source of an async upload, must outlive it)
  rnamc::TreeTabs* d_tree_tabs = nullptr;  // 2-loop tables of the tree-order mode (built from the params)
  bool tree_tabs_valid = false;
  // host-buffer entry: device staging of bases / result / log partition (grow-only)
  // The result is staged per lock-step GROUP in two alternating device buffers: group g's
  // D2H (copy stream, pinned bounce chunks, a host thread) runs while group g+1 sweeps.
  uint8_t* st_bases = nullptr;
  float* st_out[2] = {nullptr, nullptr};
  float* st_logz = nullptr;
  uint64_t st_bases_cap = 0, st_out_cap[2] = {0, 0}, st_logz_cap = 0;
  hipStream_t copy_stream = nullptr;
  float* pinned[2] = {nullptr, nullptr};  // bounce chunks (hipHostMalloc)
  hipEvent_t pinned_ev[2] = {nullptr, nullptr};
  hipEvent_t group_done[2] = {nullptr, nullptr};
  std::vector<uint64_t> group_out_floats;  // per group, when the output is staged group-local
  hipStream_t own_stream = nullptr;
  hipStream_t aux_stream = nullptr;           // pair tail of large outside launches
  std::vector<hipEvent_t> ev_a, ev_b;         // per-diagonal completion, ring of 16
  std::mutex mu;  // one call at a time; no entry re-enters it (StagedCall, rnamc_entries.cpp)
  // knobs
  // 0: every logsumexp fold in the reference's order (the parity gate); 1: order-free sums
  // (rnamc_tree.hip), not bit-comparable with the reference
  int64_t summation_mode = 0;
  int64_t tree_tpc = 0;  // tree mode: threads per cell (64 / 256 / 1024), 0 = by diagonal size
  int64_t tree_two = 1;  // tree mode: two diagonals per launch
  // tree mode: width of a band of diagonals whose products take their mid-field from k_tree_mid
  // (a multiple of 32, at most 128; 0: every launch walks its sums whole)
  int64_t tree_band = 64;
  // tree mode: lane-per-cell sweeps (rnamc_tree_lane.h) — 0 never, 1 for batches (a call of at least
  // tree_lane_min_nt nucleotides whose sweeps are banded), 2 always
  int64_t tree_lane = 1;
  int64_t tree_lane_min_nt = 65536;
  // lane-per-cell sweeps: a band's mid-field kernel runs in front of the band on the sweep's stream
  // (threshold = the band's first / last diagonal) instead of a band ahead beside it
  int64_t tree_mid_sync = 1;
  // lane-per-cell sweeps with the mid-field in front of its band: the band's width (the in-band terms are
  // the lanes' own loops: narrower bands, fewer of them; the matrix-core mid-field takes the rest)
  int64_t tree_lane_band = 32;
  // lane-per-cell sweeps: diagonals whose generic 2-loop sums share a launch (k_tlane_gen), 1 .. 3
  int64_t tree_gen_batch = 3;
  // tree mode, banded sweeps: the far part of a launch's 2-loop blocks is summed by extra
  // workgroups of the previous launch (rnamc_tree.hip, Ahead)
  int64_t tree_ahead = 1;
  rnamc::TreePolicy tree_pol;  // launch shapes of the tree-order sweep ("tree_waves", "tree_short", ...)
  hipStream_t bulk_stream = nullptr;  // k_tree_mid, beside the sweep (lowest priority)
  // tree mode, batch form: every other group of a call sweeps on a second stream with its own half of the
  // workspace, side stream and event rings — two groups side by side fill each other's launch gaps (the
  // per-diagonal launches cost ~8 us whatever they hold); "tree_dual" 0 switches it off
  int64_t tree_dual = 1;
  hipStream_t dual_stream = nullptr, bulk_stream2 = nullptr;
  std::vector<hipEvent_t> ev_a2, ev_b2;
  hipEvent_t ev_dual = nullptr;
  // does bulk_stream run beside the stream of the last banded call?  (probed once per stream:
  // tree_side_stream_probe; 0 unknown, 1 yes, 2 no -> unbanded sweeps on that stream)
  hipStream_t side_probed_for = nullptr;
  bool side_probed = false;
  int side_verdict = 0;
  int64_t tree_side_force = 0;  // knob "tree_side_stream": 0 probe, 1 take it as concurrent, 2 as serialised
  int64_t tree_debug = 0;  // (RNAMC_DEBUG_KNOBS builds: bit 0 no 2-loops, 1 no products, 2 empty kernels)
  int64_t group_max_seqs = 8192;
  int64_t group_max_nt = 2ll << 20;  // a group holds ~2M nucleotides (or 64 GB of DP state)
  int64_t group_ws_bytes = 64ll << 30;
  bool group_ws_user = false;  // the knob was set: the tree-order batch form takes it as given
  int64_t block_threads = 256;
  int64_t profile = 0;
  // dispatch order of the role blocks of a launch (measured: pair-probability chains first,
  // probs_multibranch last is 2.5 % faster than the reverse; the inside order does not matter)
  int64_t order_inside = 0, order_outside = 1;
  int64_t dual_outside = 1;   // large outside launches: pair tail as its own kernel/stream
  uint64_t dual_min_cells = 256 * 1024;
  int64_t dual_max_diag = 1 << 30;  // ... while the diagonal has at most this many cells
  int64_t fuse_inside = 1;  // Turner: fold two diagonals per launch where launches are large
  // latency forms (rnamc_latency.h) for groups that cannot fill the chip: 0 never, 1 when the
  // group's longest diagonal holds at most lat_max_cells cells over all its sequences (half of
  // that under CONTRAfold), 2 always
  int64_t latency_mode = 1;
  int64_t lat_max_cells = 32768;
  // inside folds of such a group: lat_inside != 0 takes the eight-chains-per-wave form (8-lane
  // speculative logsumexp) on the diagonals whose launches need at most lat_e_waves waves (beyond
  // ~2 waves per SIMD that form is issue-bound and loses: profiles/r02_latency_forms.txt), the
  // three-lanes-per-cell form elsewhere
  int64_t lat_inside = 2;
  int64_t lat_e_waves = 2048;
  // debug: probs_multibranch and the pair-probability chains as two launches (timing splits)
  int64_t lat_split = 0;
  // one launch per diagonal in a latency-form group (chains + 2-loop blocks), no second stream
  int64_t lat_merge = 1;
  // CONTRAfold, eight-chains form: the sums_rightmost_basepairs folds run one launch ahead
  int64_t lat_zr_ahead = 1;
  int64_t lat_pairs = 1;   // its 2-loop blocks run one wave per listed cell (both sweeps)
  // role mask of timing experiments (bit0 folds, 1 pair block, 2 mb, 3 pair probs); settable
  // only in builds with -DRNAMC_DEBUG_KNOBS (make DEBUG_KNOBS=1), constant 15 otherwise
  int64_t debug_roles = 15;
  // bookkeeping of the last call
  rnamc_batch_stats stats{};
  std::vector<rnamc::SeqDesc> descs;       // all groups, group-major
  std::vector<uint32_t> group_begin;  // prefix into descs
  std::vector<hipEvent_t> events;
  std::vector<hipEvent_t> kev;        // per-launch event pairs of the outside kernels (profiling)
  std::vector<uint8_t> kev_class;     // 0 main, 1 tail, 2 / 3 small; one per pair
  // rnamc_fold_scores: sums_close key set of the last sequence it swept, so that the usual
  // "count, allocate, fill" pair of calls runs the device sweep once
  std::vector<uint8_t> fs_bases;
  std::vector<float> fs_qb;
  int fs_contra = -1, fs_short = -1;
  // rnamc_sample_batch (grow-only): a group's rows and log-weights, the per-wave stacks of pending
  // cells, the per-descriptor row offsets
  uint8_t* sm_rows = nullptr;
  float* sm_w = nullptr;
  uint64_t* sm_stack = nullptr;
  uint64_t* sm_rowoff = nullptr;
  uint64_t sm_rows_cap = 0, sm_w_cap = 0, sm_stack_cap = 0, sm_rowoff_cap = 0;
  // rnamc_mfe_batch (grow-only, beside the sampler's buffers): a group's sweep values
  float* mf_dp = nullptr;
  uint64_t mf_dp_cap = 0;
  // hard constraints of the running call: the staged words (two per base, laid out like st_bases;
  // grow-only), handed to the sweep in its SweepOpts
  int32_t* st_cons = nullptr;
  uint64_t st_cons_cap = 0;
  // rnamc_centroid_fold_batch (grow-only, beside the sampler's rows and stacks): a chunk's item
  // descriptors, pair counts and accuracies.  centroid_chunk_bytes: the (max,+) matrices one chunk
  // of items may take; 0 = the workspace the context holds for the group
  rnamc::CentroidItem* cf_items = nullptr;
  uint32_t* cf_np = nullptr;
  float* cf_acc = nullptr;
  uint64_t cf_items_cap = 0, cf_np_cap = 0, cf_acc_cap = 0;
  int64_t centroid_chunk_bytes = 0;
  // rnamc_bpp_batch_sparse (grow-only): a group's record descriptors and totals, its staged lists
  // (i, j, p) and paired probabilities
  rnamc::SparseItem* sp_items = nullptr;
  uint32_t* sp_totals = nullptr;
  uint32_t* sp_i = nullptr;
  uint32_t* sp_j = nullptr;
  float* sp_p = nullptr;
  float* sp_paired = nullptr;
  uint64_t sp_items_cap = 0, sp_totals_cap = 0, sp_i_cap = 0, sp_j_cap = 0, sp_p_cap = 0, sp_paired_cap = 0;
  // rnamc_bpp_windowed (grow-only): a chunk's window descriptors, the call's integer accumulators
  // ([d * n + i]), its band ([i * band + d]) and paired probabilities.  window_chunk_nt: nucleotides
  // of windows that go through one staged call of the sweep (never less than one window)
  rnamc::WindowItem* wn_items = nullptr;
  int64_t* wn_sum = nullptr;
  uint32_t* wn_cnt = nullptr;
  float* wn_band = nullptr;
  float* wn_paired = nullptr;
  uint64_t wn_items_cap = 0, wn_sum_cap = 0, wn_cnt_cap = 0, wn_band_cap = 0, wn_paired_cap = 0;
  std::vector<hipEvent_t> wn_events;  // profiling: a pair around every run of window kernels
  int64_t window_chunk_nt = 64ll << 20;
  // rnamc_mutant_scan (grow-only): the wild type's triangle and paired probabilities, kept for the
  // whole call; a chunk's descriptors for the compare and the paired kernel; the call's accumulators
  // (one sum and one max key per mutant) and a chunk's paired probabilities ([record * n + x]).
  // mutant_chunk_nt: nucleotides of mutants that go through one staged call of the sweep (never
  // less than one mutant)
  float* mt_wt = nullptr;
  float* mt_wt_paired = nullptr;
  rnamc::MutantItem* mt_items = nullptr;
  rnamc::SparseItem* mt_pitems = nullptr;
  int64_t* mt_sum = nullptr;
  uint64_t* mt_key = nullptr;
  float* mt_paired = nullptr;
  uint64_t mt_wt_cap = 0, mt_wt_paired_cap = 0, mt_items_cap = 0, mt_pitems_cap = 0, mt_sum_cap = 0, mt_key_cap = 0,
           mt_paired_cap = 0;
  std::vector<hipEvent_t> mt_events;  // profiling: a pair around every run of mutant kernels
  int64_t mutant_chunk_nt = 64ll << 20;
};

namespace rnamc {

struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && hipSetDevice(dev) == hipSuccess) ok = true;
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
};

// Grow-only device buffer: `need` bytes at least (an eighth of headroom when it fits).
hipError_t grow_device(void** p, uint64_t* cap, uint64_t need);
int ensure_ws(rnamc_ctx* c, uint64_t floats);

// Per-group hooks of the host-buffer entry: where group g's result goes, and what happens
// once its work is enqueued.  With hooks the output offsets are group-local (packed in group
// order), without them the caller's out_offsets address one device buffer.
struct GroupHooks {
  std::function<int(size_t g, float** out_base)> before;
  std::function<int(size_t g, uint32_t first_desc, uint32_t n_desc)> after;
};

// The front the two sweeps share: a batch sorted longest-first and cut greedily into lock-step
// groups (c->descs, group_begin, group_out_floats).  What a sequence takes of the workspace and how
// it is laid out stays with the sweep.
struct BatchPlan {
  rnamc_ctx* c = nullptr;
  uint32_t max_n = 0;
  std::vector<uint32_t> order;  // longest first, ties in the caller's order
  uint64_t max_group_floats = 0;
  // resets the call's bookkeeping, validates the offsets, sizes hp_init, sorts (nothing of it for n_seqs == 0)
  int begin(rnamc_ctx* ctx, uint32_t n_seqs, const uint64_t* offsets);
  // need(n): workspace floats of a sequence; place(sd): the sweep's own layout of a descriptor whose
  // n, seq_off, ws_off, out_off (group-local without out_offsets) and batch_idx are set
  void cut(const uint64_t* offsets, const uint64_t* out_offsets, uint64_t ws_cap_floats,
           const std::function<uint64_t(uint32_t)>& need, const std::function<void(SeqDesc&)>& place);
  size_t n_groups() const { return c->group_begin.size() - 1; }
  uint32_t active(size_t g, uint32_t d) const;  // sequences of group g with n > d: a prefix of it
  int create_events();                          // profiling: four per group
  int finish(hipStream_t st);                   // n_groups, workspace_bytes; profiling: ms_inside / _outside / _other
};
// grow-only device copy of a call's descriptors (d_seqs / d_tseqs), uploaded on `st`
int upload_descs(void** d, uint64_t* cap, const void* h, uint64_t count, uint64_t elem_bytes, hipStream_t st);

int run_batch(rnamc_ctx* c, uint32_t n_seqs, const uint8_t* d_bases, const uint64_t* offsets, bool contra,
              bool allows_short, float* d_out, const uint64_t* out_offsets, float* d_logz, hipStream_t st,
              const SweepOpts& opts, const GroupHooks* hooks = nullptr);
int run_batch_tree(rnamc_ctx* c, uint32_t n_seqs, const uint8_t* d_bases, const uint64_t* offsets, bool contra,
                   bool allows_short, float* d_out, const uint64_t* out_offsets, float* d_logz, hipStream_t st,
                   const SweepOpts& opts, const GroupHooks* hooks = nullptr);
// the sweep of the context's summation mode (an inside-only sweep needs the reference-order
// workspace layout and always takes that path)
int run_batch_mode(rnamc_ctx* c, uint32_t n_seqs, const uint8_t* d_bases, const uint64_t* offsets, bool contra,
                   bool allows_short, float* d_out, const uint64_t* out_offsets, float* d_logz, hipStream_t st,
                   const SweepOpts& opts, const GroupHooks* hooks = nullptr);

}  // namespace rnamc

#endif
