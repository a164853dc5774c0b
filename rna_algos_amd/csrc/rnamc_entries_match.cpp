// rnamc_entries_match.cpp — pairwise alignment off match-probability matrices that stay on the
// device (rnamc_match.hip): rnamc_match_align_mats over the caller's dense
// matrices, rnamc_durbin_align_batch behind the pair-HMM kernels of rnamc_durbin_batch.  Both cut
// their matrices into chunks and hand every chunk to one stage: thresholded lists (count, scan,
// fill), per-base marginals, and the gamma-centroid alignment of every (matrix, gamma).
#include "rnamc_entries.h"

using namespace rnamc;

namespace {

// what both entries take after their inputs
struct MatchArgs {
  float min_prob;
  const float* gammas;
  uint32_t ng;
  uint32_t* match_i;
  uint32_t* match_j;
  float* match_prob;
  uint64_t cap;
  uint64_t* list_start;
  uint64_t* list_count;
  uint64_t* list_total;
  int32_t* mate;
  const uint64_t* mate_offsets;
  uint32_t* n_matched;
  float* accuracy;
  float* matched;
  const uint64_t* matched_offsets;

  bool aligns() const { return ng != 0 && (mate || n_matched || accuracy); }
};

// argument checks of both entries: nothing of the context is read before they pass
int match_check(const char* who, const MatchArgs& a, uint32_t n_items) {
  if (!a.list_total) return RNAMC_ERR_INVALID_ARG;
  if (!std::isfinite(a.min_prob) || a.min_prob < 0.f) {
    set_last_error(std::string(who) + ": min_prob must be finite and >= 0");
    return RNAMC_ERR_INVALID_ARG;
  }
  const int given = (a.match_i != nullptr) + (a.match_j != nullptr) + (a.match_prob != nullptr);
  if (given != 0 && given != 3) {
    set_last_error(std::string(who) + ": match_i, match_j and match_prob go together");
    return RNAMC_ERR_INVALID_ARG;
  }
  if (given == 3 && n_items && (!a.list_start || !a.list_count)) return RNAMC_ERR_INVALID_ARG;
  if (a.ng > 64u || (a.ng && !a.gammas)) {
    set_last_error(std::string(who) + ": at most 64 gammas");
    return RNAMC_ERR_INVALID_ARG;
  }
  for (uint32_t g = 0; g < a.ng; g++)
    if (!std::isfinite(a.gammas[g])) {
      set_last_error(std::string(who) + ": gammas must be finite");
      return RNAMC_ERR_INVALID_ARG;
    }
  if (n_items && ((a.mate && !a.mate_offsets) || (a.matched && !a.matched_offsets))) return RNAMC_ERR_INVALID_ARG;
  return RNAMC_OK;
}

// The stage over one chunk of device-resident matrices after another.  add() plans a matrix of the
// running chunk (its part of the workspace, of the staged mates and marginals), run() launches the
// chunk on the context's stream, drains it and writes the caller's arrays for items
// first .. first + count - 1.  The device and host scratch lives in the stage and only grows.
struct MatchStage {
  rnamc_ctx* c;
  const char* who;
  MatchArgs a;
  hipStream_t st;
  uint64_t cursor = 0;  // listed cells of the chunks so far: where the next chunk's lists go

  std::vector<MatchMat> items;
  uint64_t ws = 0, n_mate = 0, n_marg = 0;
  uint32_t max_blocks = 0, max_side = 0;

  MatchStage(rnamc_ctx* ctx, const char* entry, const MatchArgs& args)
      : c(ctx), who(entry), a(args), st(ctx->own_stream), drain{ctx->own_stream} {}

  // floats of workspace a matrix takes: block counts, spilled diagonals, direction bytes
  static uint64_t ws_floats(uint32_t n1, uint32_t n2, uint32_t ng_aligned) {
    const uint64_t blocks = (static_cast<uint64_t>(n1) * n2 + 255u) / 256u;
    const uint64_t w = n1 - 1u;
    const uint64_t spill = w > kMatchDiagLds ? 3u * w * ng_aligned : 0u;
    return blocks + spill + (match_dir_bytes(n1, n2) * ng_aligned + 3u) / 4u;
  }
  uint32_t ng_aligned() const { return a.aligns() ? a.ng : 0u; }

  int begin() {
    HIPCHK(hipEventCreateWithFlags(counted.put(), hipEventDisableTiming));
    if (a.aligns()) HIPCHK(d_gammas.upload(a.gammas, a.ng, st));
    return RNAMC_OK;
  }

  void clear() {
    items.clear();
    ws = n_mate = n_marg = 0;
    max_blocks = max_side = 0;
  }

  void add(uint32_t n1, uint32_t n2, uint64_t p_off) {
    const uint32_t ng = ng_aligned();
    MatchMat mt{};
    mt.p_off = p_off;
    mt.n1 = n1;
    mt.n2 = n2;
    mt.n_blocks = static_cast<uint32_t>((static_cast<uint64_t>(n1) * n2 + 255u) / 256u);
    mt.blk_off = ws;
    mt.spill_off = ws + mt.n_blocks;
    const uint64_t w = n1 - 1u;
    mt.dir_off = (mt.spill_off + (w > kMatchDiagLds ? 3u * w * ng : 0u)) * sizeof(float);
    mt.mate_off = n_mate;
    mt.marg_off = n_marg;
    items.push_back(mt);
    ws += ws_floats(n1, n2, ng);
    n_mate += static_cast<uint64_t>(ng) * n1;
    n_marg += static_cast<uint64_t>(n1) + n2;
    max_blocks = std::max(max_blocks, mt.n_blocks);
    max_side = std::max(max_side, n1 + n2);
  }

  // the chunk's workspace is c->d_ws (ensure_ws(ws) passed); everything that wrote d_probs and
  // everything that used the workspace before is enqueued on `st`
  int run(const float* d_probs, uint32_t first) {
    const uint32_t count = static_cast<uint32_t>(items.size());
    const uint32_t ng = ng_aligned();
    try {  // nothing may throw across the C boundary
      h_totals.resize(count);
      if (a.matched) h_marg.resize(n_marg);
      if (ng) {
        h_mate.resize(n_mate);
        h_nm.resize(static_cast<size_t>(count) * ng);
        h_acc.resize(static_cast<size_t>(count) * ng);
      }
    } catch (const std::exception&) {
      set_last_error(std::string(who) + ": no host memory for a chunk");
      return RNAMC_ERR_OOM;
    }
    uint32_t* d_blocks = reinterpret_cast<uint32_t*>(c->d_ws.get());
    HIPCHK(d_mats.upload(items.data(), count, st));
    HIPCHK(d_totals.grow(count));
    launch_match_count(d_mats, count, max_blocks, d_probs, d_blocks, a.min_prob, st);
    launch_match_scan(d_mats, count, d_blocks, d_totals, st);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_totals.data(), d_totals, count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(counted, st));
    // the marginals and the alignments run while the host places the lists
    if (a.matched) {
      HIPCHK(d_marg.grow(n_marg));
      launch_match_marginals(d_mats, count, max_side, d_probs, d_marg, st);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(h_marg.data(), d_marg, n_marg * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    if (ng) {
      HIPCHK(d_mate.grow(n_mate));
      HIPCHK(d_nm.grow(static_cast<uint64_t>(count) * ng));
      HIPCHK(d_acc.grow(static_cast<uint64_t>(count) * ng));
      launch_match_align(d_mats, count, d_probs, d_gammas, ng, c->d_ws, d_mate, d_nm, d_acc, st);
      HIPCHK(hipGetLastError());
      if (a.mate) HIPCHK(hipMemcpyAsync(h_mate.data(), d_mate, n_mate * sizeof(int32_t), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(h_nm.data(), d_nm, h_nm.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(h_acc.data(), d_acc, h_acc.size() * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipEventSynchronize(counted));
    uint64_t total = 0;
    for (uint32_t x = 0; x < count; x++) {
      items[x].out_off = total;
      total += h_totals[x];
    }
    const uint64_t start = cursor;
    cursor += total;
    // a chunk that does not fit (or a counting call) is counted only; the entry compares the total
    // with the capacity when all chunks are through
    const bool fill = a.match_i != nullptr && start + total <= a.cap;
    for (uint32_t x = 0; x < count; x++) {
      if (a.list_count) a.list_count[first + x] = h_totals[x];
      if (fill) a.list_start[first + x] = start + items[x].out_off;
    }
    if (fill && total) {
      HIPCHK(d_i.grow(total));
      HIPCHK(d_j.grow(total));
      HIPCHK(d_p.grow(total));
      // (behind the kernels above in stream order: they read the items as they were)
      HIPCHK(hipMemcpyAsync(d_mats, items.data(), count * sizeof(MatchMat), hipMemcpyHostToDevice, st));
      launch_match_list(d_mats, count, max_blocks, d_probs, d_blocks, a.min_prob, d_i, d_j, d_p, st);
      HIPCHK(hipGetLastError());
      // the chunk's lists are contiguous in the caller's arrays: one copy per array
      HIPCHK(hipMemcpyAsync(a.match_i + start, d_i, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(a.match_j + start, d_j, total * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      HIPCHK(hipMemcpyAsync(a.match_prob + start, d_p, total * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    // (the next chunk reuses the workspace and the matrices: everything above is done first)
    HIPCHK(hipStreamSynchronize(st));
    for (uint32_t x = 0; x < count; x++) {
      const MatchMat& mt = items[x];
      const uint64_t p = first + x;
      if (a.matched)
        std::memcpy(a.matched + a.matched_offsets[p], h_marg.data() + mt.marg_off,
                    (static_cast<size_t>(mt.n1) + mt.n2) * sizeof(float));
      if (!ng) continue;
      if (a.mate)
        std::memcpy(a.mate + a.mate_offsets[p], h_mate.data() + mt.mate_off,
                    static_cast<size_t>(ng) * mt.n1 * sizeof(int32_t));
      for (uint32_t g = 0; g < ng; g++) {
        if (a.n_matched) a.n_matched[p * ng + g] = h_nm[static_cast<size_t>(x) * ng + g];
        if (a.accuracy) a.accuracy[p * ng + g] = h_acc[static_cast<size_t>(x) * ng + g];
      }
    }
    return RNAMC_OK;
  }

  // the end both entries share: the total, and the status of a call whose arrays were too small
  int finish() {
    *a.list_total = cursor;
    if (a.match_i && cursor > a.cap) {
      set_last_error(std::string(who) + ": " + std::to_string(cursor) + " listed cells, capacity " +
                     std::to_string(a.cap));
      return RNAMC_ERR_INVALID_ARG;
    }
    return RNAMC_OK;
  }

 private:
  DevBuf<MatchMat> d_mats;
  DevBuf<float> d_gammas, d_p, d_acc, d_marg;
  DevBuf<uint32_t> d_totals, d_i, d_j, d_nm;
  DevBuf<int32_t> d_mate;
  Event counted;  // the chunk's totals are on the host
  std::vector<uint32_t> h_totals, h_nm;
  std::vector<float> h_marg, h_acc;
  std::vector<int32_t> h_mate;
  // declared after the buffers, so run before they are released: whatever still uses them is done
  struct Drain {
    hipStream_t st;
    ~Drain() { (void)hipStreamSynchronize(st); }
  } drain;
};

uint64_t ws_cap_floats(const rnamc_ctx* c) {
  return static_cast<uint64_t>(std::max<int64_t>(c->group_ws_bytes, 1)) / sizeof(float);
}

}  // namespace

extern "C" {

int rnamc_match_align_mats(rnamc_ctx* c, uint32_t n_mats, const uint32_t* n1, const uint32_t* n2,
                           const float* probs, const uint64_t* prob_offsets, float min_prob, const float* gammas,
                           uint32_t n_gammas, uint32_t* match_i, uint32_t* match_j, float* match_prob,
                           uint64_t cap, uint64_t* list_start, uint64_t* list_count, uint64_t* list_total,
                           int* mate, const uint64_t* mate_offsets, uint32_t* n_matched, float* expect_accuracy,
                           float* matched, const uint64_t* matched_offsets) {
  static const char* who = "rnamc_match_align_mats";
  if (!c || (n_mats && (!n1 || !n2 || !probs || !prob_offsets))) return RNAMC_ERR_INVALID_ARG;
  const MatchArgs args{min_prob,   gammas,     n_gammas, match_i,      match_j,   match_prob,      cap,    list_start,
                       list_count, list_total, mate,     mate_offsets, n_matched, expect_accuracy, matched,
                       matched_offsets};
  if (int rc = match_check(who, args, n_mats)) return rc;
  for (uint32_t m = 0; m < n_mats; m++) {
    // (a ProbMat has its two border rows and columns)
    if (n1[m] < 2u || n2[m] < 2u) return RNAMC_ERR_EMPTY_SEQ;
    if (n1[m] > RNAMC_MAX_SEQ_LEN + 2ull || n2[m] > RNAMC_MAX_SEQ_LEN + 2ull) return RNAMC_ERR_SEQ_TOO_LONG;
  }
  *list_total = 0;
  if (n_mats == 0) return RNAMC_OK;
  std::lock_guard<std::mutex> lock(c->mu);
  DeviceGuard guard(c->device);
  if (!guard.ok) return RNAMC_ERR_NO_DEVICE;
  DevBuf<float> d_probs;
  MatchStage stage(c, who, args);  // (declared after d_probs: drained before it is released)
  if (int rc = stage.begin()) return rc;
  // matrices in chunks that fit the workspace budget together with what the stage makes of them
  const uint64_t ws_cap = ws_cap_floats(c);
  std::vector<float> h_probs;
  for (uint32_t m0 = 0; m0 < n_mats;) {
    stage.clear();
    uint64_t cells_sum = 0;
    uint32_t m = m0;
    for (; m < n_mats; m++) {
      const uint64_t cells = static_cast<uint64_t>(n1[m]) * n2[m];
      const uint64_t need = MatchStage::ws_floats(n1[m], n2[m], stage.ng_aligned());
      if (m > m0 && (cells_sum + cells + stage.ws + need > ws_cap || m - m0 >= 65535u)) break;
      stage.add(n1[m], n2[m], cells_sum);
      cells_sum += cells;
    }
    try {
      h_probs.resize(cells_sum);
    } catch (...) {
      return RNAMC_ERR_OOM;
    }
    for (uint32_t x = m0; x < m; x++)
      std::memcpy(h_probs.data() + stage.items[x - m0].p_off, probs + prob_offsets[x],
                  static_cast<uint64_t>(n1[x]) * n2[x] * sizeof(float));
    if (int rc = ensure_ws(c, stage.ws)) return rc;
    // (the chunk before is drained: nothing uses the buffer)
    HIPCHK(d_probs.grow(cells_sum));
    HIPCHK(hipMemcpyAsync(d_probs, h_probs.data(), cells_sum * sizeof(float), hipMemcpyHostToDevice, stage.st));
    if (int rc = stage.run(d_probs, m0)) return rc;
    m0 = m;
  }
  return stage.finish();
}

int rnamc_durbin_align_batch(rnamc_ctx* c, const rnamc_align_scores* scores, uint32_t n_seqs, const uint8_t* bases,
                             const uint64_t* offsets, uint32_t n_pairs, const uint32_t* pair_a,
                             const uint32_t* pair_b, float min_prob, const float* gammas, uint32_t n_gammas,
                             uint32_t* match_i, uint32_t* match_j, float* match_prob, uint64_t cap,
                             uint64_t* list_start, uint64_t* list_count, uint64_t* list_total, int* mate,
                             const uint64_t* mate_offsets, uint32_t* n_matched, float* expect_accuracy,
                             float* matched, const uint64_t* matched_offsets, float* match_probs,
                             const uint64_t* out_offsets) {
  static const char* who = "rnamc_durbin_align_batch";
  if (!c || !scores || !offsets || (n_seqs && !bases) || (n_pairs && (!pair_a || !pair_b)) ||
      (match_probs != nullptr) != (out_offsets != nullptr))
    return RNAMC_ERR_INVALID_ARG;
  const MatchArgs args{min_prob,   gammas,     n_gammas, match_i,      match_j,   match_prob,      cap,    list_start,
                       list_count, list_total, mate,     mate_offsets, n_matched, expect_accuracy, matched,
                       matched_offsets};
  if (int rc = match_check(who, args, n_pairs)) return rc;
  // real bases inside, anything (PSEUDO_BASE) at the two ends, which are never scored
  if (int rc = check_records(n_seqs, bases, offsets, 1)) return rc;
  for (uint32_t p = 0; p < n_pairs; p++)
    if (pair_a[p] >= n_seqs || pair_b[p] >= n_seqs) return RNAMC_ERR_INVALID_ARG;
  *list_total = 0;
  if (n_pairs == 0) return RNAMC_OK;
  std::lock_guard<std::mutex> lock(c->mu);
  DeviceGuard guard(c->device);
  if (!guard.ok) return RNAMC_ERR_NO_DEVICE;
  hipStream_t st = c->own_stream;
  const uint64_t base_lo = offsets[0], base_hi = offsets[n_seqs];
  DevBuf<uint8_t> d_bases;
  DevBuf<DurbinPair> d_pairs;
  DevBuf<float> d_out;
  MatchStage stage(c, who, args);  // (declared after the buffers: drained before they are released)
  if (int rc = stage.begin()) return rc;
  HIPCHK(d_bases.grow(std::max<uint64_t>(base_hi - base_lo, 1)));
  HIPCHK(hipMemcpyAsync(d_bases, bases + base_lo, base_hi - base_lo, hipMemcpyHostToDevice, st));
  // pairs in chunks whose six matrices per pair, and then what the stage makes of the pair's
  // ProbMat in their place, fit the workspace budget
  const uint64_t ws_cap = ws_cap_floats(c);
  std::vector<DurbinPair> chunk;
  std::vector<float> h_out;
  for (uint32_t p0 = 0; p0 < n_pairs;) {
    chunk.clear();
    stage.clear();
    uint64_t ws = 0, out = 0;
    uint32_t max_cells = 0, p = p0;
    for (; p < n_pairs; p++) {
      DurbinPair dp{};
      dp.n1 = static_cast<uint32_t>(offsets[pair_a[p] + 1] - offsets[pair_a[p]]);
      dp.n2 = static_cast<uint32_t>(offsets[pair_b[p] + 1] - offsets[pair_b[p]]);
      const uint64_t cells = static_cast<uint64_t>(dp.n1) * dp.n2;
      const uint64_t need = MatchStage::ws_floats(dp.n1, dp.n2, stage.ng_aligned());
      // (k_durbin_probs and the stage index pairs through blockIdx.y: at most 65535 per launch)
      if (!chunk.empty() && (ws + 6 * cells > ws_cap || stage.ws + need > ws_cap || chunk.size() >= 65535u)) break;
      dp.a_off = offsets[pair_a[p]] - base_lo;
      dp.b_off = offsets[pair_b[p]] - base_lo;
      dp.ws_off = ws;
      dp.out_off = out;
      chunk.push_back(dp);
      stage.add(dp.n1, dp.n2, out);
      ws += 6 * cells;
      out += cells;
      max_cells = static_cast<uint32_t>(std::min<uint64_t>(std::max<uint64_t>(max_cells, cells), 0xFFFFFFFFull));
    }
    // the pair-HMM's matrices are dead when the stage starts: it runs in their place
    if (int rc = ensure_ws(c, std::max(ws, stage.ws))) return rc;
    // (the chunk before is drained: nothing uses its buffers)
    HIPCHK(d_pairs.upload(chunk.data(), chunk.size(), st));
    HIPCHK(d_out.grow(out));
    launch_durbin(d_pairs, static_cast<uint32_t>(chunk.size()), max_cells, d_bases, c->d_ws, d_out, *scores, st);
    HIPCHK(hipGetLastError());
    if (match_probs) {
      // one D2H per chunk, scattered on the host (as rnamc_durbin_batch does)
      try {
        h_out.resize(out);
      } catch (...) {
        return RNAMC_ERR_OOM;
      }
      HIPCHK(hipMemcpyAsync(h_out.data(), d_out, out * sizeof(float), hipMemcpyDeviceToHost, st));
    }
    if (int rc = stage.run(d_out, p0)) return rc;
    if (match_probs)
      for (size_t x = 0; x < chunk.size(); x++)
        std::memcpy(match_probs + out_offsets[p0 + x], h_out.data() + chunk[x].out_off,
                    static_cast<uint64_t>(chunk[x].n1) * chunk[x].n2 * sizeof(float));
    p0 = p;
  }
  return stage.finish();
}

}  // extern "C"
