// rnamc_ctx.h — the device context behind the C ABI and what the host translation units that work
// on it share: rnamc_ctx.cpp (life cycle, knobs, statistics), rnamc_sweep.cpp (batch plan and the
// reference-order sweep), rnamc_sweep_tree.cpp (tree-order sweep), rnamc_entries.cpp (the entries).
//
// Every device buffer, pinned chunk, event and stream of the context is a member of an owner type
// (DevBuf, PinnedBuf, Event, EventRing, Stream): non-copyable, released by its destructor, read at a
// call site as the plain pointer or handle.  An entry that needs device state adds one member to
// rnamc_ctx and nothing else; rnamc_ctx_destroy deletes the context and names no resource.
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

namespace rnamc {

// A device buffer and its capacity in bytes.
template <class T>
struct DevBuf {
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { (void)reset(); }
  operator T*() const { return p; }
  T* get() const { return p; }
  uint64_t bytes() const { return cap; }
  hipError_t reset() {  // free now
    const hipError_t e = p ? hipFree(p) : hipSuccess;
    p = nullptr;
    cap = 0;
    return e;
  }
  // free, then allocate exactly `count` elements (callers with sizing and sync rules of their own)
  hipError_t replace_exact(uint64_t count) {
    if (hipError_t e = reset()) return e;
    return alloc(count * sizeof(T));
  }
  // grow-only: `count` elements at least (an eighth of headroom when it fits)
  hipError_t grow(uint64_t count) {
    const uint64_t need = count * sizeof(T);
    if (p && cap >= need) return hipSuccess;
    (void)reset();
    if (alloc(std::max<uint64_t>(need + need / 8, 4096)) == hipSuccess) return hipSuccess;
    return alloc(std::max<uint64_t>(need, 1));  // the headroom is optional
  }
  // grow, then copy `count` elements of host memory behind the work of `st`
  hipError_t upload(const T* h, uint64_t count, hipStream_t st) {
    if (hipError_t e = grow(count)) return e;
    return hipMemcpyAsync(p, h, count * sizeof(T), hipMemcpyHostToDevice, st);
  }

 private:
  hipError_t alloc(uint64_t n_bytes) {
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&p), n_bytes);
    if (e == hipSuccess) cap = n_bytes;
    return e;
  }
  T* p = nullptr;
  uint64_t cap = 0;
};

// A pinned host chunk (hipHostMalloc), allocated once.
struct PinnedBuf {
  PinnedBuf() = default;
  PinnedBuf(const PinnedBuf&) = delete;
  PinnedBuf& operator=(const PinnedBuf&) = delete;
  ~PinnedBuf() {
    if (p) (void)hipHostFree(p);
  }
  operator float*() const { return p; }
  hipError_t alloc(uint64_t floats) {
    return hipHostMalloc(reinterpret_cast<void**>(&p), floats * sizeof(float), hipHostMallocDefault);
  }

 private:
  float* p = nullptr;
};

// One event or stream.  The owner creates nothing by itself: whoever needs the handle creates it
// into put(), when and how it wants it (the order in which a process creates its streams matters:
// rnamc_ctx_create).
template <class H, hipError_t (*Destroy)(H)>
struct Handle {
  Handle() = default;
  Handle(const Handle&) = delete;
  Handle& operator=(const Handle&) = delete;
  ~Handle() {
    if (h) (void)Destroy(h);
  }
  operator H() const { return h; }
  H* put() { return &h; }

 private:
  H h = nullptr;
};
using Event = Handle<hipEvent_t, hipEventDestroy>;
using Stream = Handle<hipStream_t, hipStreamDestroy>;

// A grow-only ring of events of one kind (timed unless the flags say hipEventDisableTiming).  A
// launch loop reads it through data(): plain handles.
struct EventRing {
  explicit EventRing(unsigned event_flags = hipEventDefault) : flags(event_flags) {}
  EventRing(const EventRing&) = delete;
  EventRing& operator=(const EventRing&) = delete;
  ~EventRing() {
    for (hipEvent_t e : ev) (void)hipEventDestroy(e);
  }
  size_t size() const { return ev.size(); }
  const hipEvent_t* data() const { return ev.data(); }
  hipEvent_t operator[](size_t x) const { return ev[x]; }
  hipError_t grow(size_t count) {
    while (ev.size() < count) {
      hipEvent_t e = nullptr;
      if (hipError_t err = hipEventCreateWithFlags(&e, flags)) return err;
      ev.push_back(e);
    }
    return hipSuccess;
  }
  // profiling: pair p = events 2p, 2p + 1 around an entry's own kernels; the milliseconds of the
  // first `pairs` pairs added to *ms once their stream is drained
  hipError_t pairs(size_t pairs) { return grow(2 * pairs); }
  hipError_t pairs_ms(size_t pairs, double* ms) const {
    for (size_t p = 0; p < pairs; p++) {
      float t = 0.f;
      if (hipError_t err = hipEventElapsedTime(&t, ev[2 * p], ev[2 * p + 1])) return err;
      *ms += t;
    }
    return hipSuccess;
  }

 private:
  std::vector<hipEvent_t> ev;
  unsigned flags;
};

}  // namespace rnamc

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
  rnamc::DevBuf<rnamc_params> d_params;
  rnamc::DevBuf<float> d_hp_init;
  std::vector<float> h_hp_init;  // host copy, for rnamc_fold_scores
  uint32_t hp_init_len = 0;
  rnamc::DevBuf<float> d_ws;  // the workspace (ensure_ws)
  uint64_t ws_floats = 0;
  rnamc::DevBuf<rnamc::SeqDesc> d_seqs;
  rnamc::DevBuf<rnamc::TreeSeq> d_tseqs;  // descriptors of the tree-order mode
  std::vector<rnamc::TreeSeq> h_tseqs;  // (host copy: source of an async upload, must outlive it)
  rnamc::DevBuf<rnamc::TreeTabs> d_tree_tabs;  // 2-loop tables of the tree-order mode (built from the params)
  bool tree_tabs_valid = false;
  // host-buffer entry: device staging of bases / result / log partition (grow-only)
  // The result is staged per lock-step GROUP in two alternating device buffers: group g's
  // D2H (copy stream, pinned bounce chunks, a host thread) runs while group g+1 sweeps.
  rnamc::DevBuf<uint8_t> st_bases;
  rnamc::DevBuf<float> st_out[2];
  rnamc::DevBuf<float> st_logz;
  rnamc::Stream copy_stream;     // (created by the first rnamc_bpp_batch, not with the context)
  rnamc::PinnedBuf pinned[2];    // bounce chunks
  rnamc::Event pinned_ev[2];
  rnamc::Event group_done[2];
  std::vector<uint64_t> group_out_floats;  // per group, when the output is staged group-local
  rnamc::Stream own_stream;
  rnamc::Stream aux_stream;  // pair tail of large outside launches
  rnamc::EventRing ev_a{hipEventDisableTiming}, ev_b{hipEventDisableTiming};  // per-diagonal completion, ring of 16
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
  rnamc::Stream bulk_stream;  // k_tree_mid, beside the sweep (lowest priority)
  // tree mode, batch form: every other group of a call sweeps on a second stream with its own half of the
  // workspace, side stream and event rings — two groups side by side fill each other's launch gaps (the
  // per-diagonal launches cost ~8 us whatever they hold); "tree_dual" 0 switches it off
  int64_t tree_dual = 1;
  hipStream_t dual_stream = nullptr, bulk_stream2 = nullptr;  // (not owned: aux_stream and own_stream)
  rnamc::EventRing ev_a2{hipEventDisableTiming}, ev_b2{hipEventDisableTiming};
  rnamc::Event ev_dual;
  // does bulk_stream run beside the stream of the last banded call?  (probed once per stream:
  // tree_side_stream_probe; 0 unknown, 1 yes, 2 no -> unbanded sweeps on that stream)
  hipStream_t side_probed_for = nullptr;  // (not owned: the caller's stream)
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
  uint32_t last_dmin_out = 0;         // lowest diagonal the outside sweep of the last reference-order call wrote
  rnamc::EventRing events;            // profiling: four per group
  rnamc::EventRing kev;               // per-launch event pairs of the outside kernels (profiling)
  std::vector<uint8_t> kev_class;     // 0 main, 1 tail, 2 / 3 small; one per pair
  // rnamc_fold_scores: sums_close key set of the last sequence it swept, so that the usual
  // "count, allocate, fill" pair of calls runs the device sweep once
  std::vector<uint8_t> fs_bases;
  std::vector<float> fs_qb;
  int fs_contra = -1, fs_short = -1;
  // rnamc_sample_batch (grow-only): a group's rows and log-weights, the per-wave stacks of pending
  // cells, the per-descriptor row offsets
  rnamc::DevBuf<uint8_t> sm_rows;
  rnamc::DevBuf<float> sm_w;
  rnamc::DevBuf<uint64_t> sm_stack;
  rnamc::DevBuf<uint64_t> sm_rowoff;
  // rnamc_mfe_batch (grow-only, beside the sampler's buffers): a group's sweep values
  rnamc::DevBuf<float> mf_dp;
  // hard constraints of the running call: the staged words (two per base, laid out like st_bases;
  // grow-only), handed to the sweep in its SweepOpts
  rnamc::DevBuf<int32_t> st_cons;
  // rnamc_centroid_fold_batch (grow-only, beside the sampler's rows and stacks): a chunk's item
  // descriptors, pair counts and accuracies.  centroid_chunk_bytes: the (max,+) matrices one chunk
  // of items may take; 0 = the workspace the context holds for the group
  rnamc::DevBuf<rnamc::CentroidItem> cf_items;
  rnamc::DevBuf<uint32_t> cf_np;
  rnamc::DevBuf<float> cf_acc;
  int64_t centroid_chunk_bytes = 0;
  // rnamc_bpp_batch_sparse (grow-only): a group's record descriptors and totals, its staged lists
  // (i, j, p) and paired probabilities
  rnamc::DevBuf<rnamc::SparseItem> sp_items;
  rnamc::DevBuf<uint32_t> sp_totals, sp_i, sp_j;
  rnamc::DevBuf<float> sp_p, sp_paired;
  // rnamc_bpp_windowed (grow-only): a chunk's window descriptors, the call's integer accumulators
  // ([d * n + i]), its band ([i * band + d]) and paired probabilities.  window_chunk_nt: nucleotides
  // of windows that go through one staged call of the sweep (never less than one window)
  rnamc::DevBuf<rnamc::WindowItem> wn_items;
  rnamc::DevBuf<int64_t> wn_sum;
  rnamc::DevBuf<uint32_t> wn_cnt;
  rnamc::DevBuf<float> wn_band, wn_paired;
  rnamc::EventRing wn_events;  // profiling: a pair around every run of window kernels
  int64_t window_chunk_nt = 64ll << 20;
  // rnamc_bpp_alignment (grow-only): the call's row descriptors and column maps, its integer
  // accumulators and the averaged triangle (packed diagonal-major over the columns: 16 bytes per
  // column-pair cell in all), and the column profile
  rnamc::DevBuf<rnamc::AlignItem> al_items;
  rnamc::DevBuf<uint32_t> al_maps;
  rnamc::DevBuf<int64_t> al_sum;
  rnamc::DevBuf<uint32_t> al_cnt;
  rnamc::DevBuf<float> al_out, al_paired;
  // rnamc_mutant_scan (grow-only): the wild type's triangle and paired probabilities, kept for the
  // whole call; a chunk's descriptors for the compare and the paired kernel; the call's accumulators
  // (one sum and one max key per mutant) and a chunk's paired probabilities ([record * n + x]).
  // mutant_chunk_nt: nucleotides of mutants that go through one staged call of the sweep (never
  // less than one mutant)
  rnamc::DevBuf<float> mt_wt, mt_wt_paired;
  rnamc::DevBuf<rnamc::MutantItem> mt_items;
  rnamc::DevBuf<rnamc::SparseItem> mt_pitems;
  rnamc::DevBuf<int64_t> mt_sum;
  rnamc::DevBuf<uint64_t> mt_key;
  rnamc::DevBuf<float> mt_paired;
  rnamc::EventRing mt_events;  // profiling: a pair around every run of mutant kernels
  int64_t mutant_chunk_nt = 64ll << 20;
  // rnamc_context_profile_batch (grow-only): a group's record descriptors, its copies of
  // sums_multibranch (taken between the two sweeps), its integer accumulators and staged profiles
  rnamc::DevBuf<rnamc::ContextItem> cx_items;
  rnamc::DevBuf<float> cx_qm, cx_out;
  rnamc::DevBuf<unsigned long long> cx_acc;
  rnamc::EventRing cx_events;  // profiling: a pair around every group's context kernels
  uint64_t cx_launches = 0;    // rnamc_context_profile_stats: of the last call (BatchPlan::begin resets them)
  double cx_ms = 0.0;
  // rnamc_duplex_batch (grow-only): a chunk's pair descriptors and per-pair results, its staged
  // probabilities (match, then bound) and structure bytes
  rnamc::DevBuf<rnamc::DuplexPair> dx_pairs;
  rnamc::DevBuf<rnamc::DuplexRes> dx_res;
  rnamc::DevBuf<float> dx_out;
  rnamc::DevBuf<uint8_t> dx_structs;
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

int ensure_ws(rnamc_ctx* c, uint64_t floats);

// Per-group hooks of the host-buffer entry: where group g's result goes, and what happens
// once its work is enqueued.  With hooks the output offsets are group-local (packed in group
// order), without them the caller's out_offsets address one device buffer.
struct GroupHooks {
  std::function<int(size_t g, float** out_base)> before;
  std::function<int(size_t g, uint32_t first_desc, uint32_t n_desc)> after;
  // optional (reference-order sweep with an outside sweep only): between group g's inside and
  // outside sweeps, everything of the inside sweep enqueued on the sweep's stream and nothing of the
  // outside sweep on any -- what it enqueues there precedes the first outside launch on either stream
  std::function<int(size_t g, uint32_t first_desc, uint32_t n_desc)> mid;
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
  int create_events();                          // profiling: four per group (c->events)
  int finish(hipStream_t st);                   // n_groups, workspace_bytes; profiling: ms_inside / _outside / _other
};
// grow-only device copy of a call's descriptors (d_seqs / d_tseqs), uploaded on `st`: 1 024 at least, no
// headroom; earlier calls may still read the old copy
template <class T>
int upload_descs(DevBuf<T>& d, const std::vector<T>& h, hipStream_t st) {
  if (d.bytes() < h.size() * sizeof(T)) {
    if (d) HIPCHK(hipDeviceSynchronize());
    HIPCHK(d.replace_exact(std::max<uint64_t>(h.size(), 1024)));
  }
  HIPCHK(hipMemcpyAsync(d, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, st));
  return RNAMC_OK;
}

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
