// rnamc_entries.cpp — the entries of the C ABI that run a sweep: argument and record checks, staging
// of the caller's host buffers, and what each entry does with a group once its sweep is enqueued.
#include "rnamc_entries.h"

using namespace rnamc;

namespace {

// FoldScores of one sequence on the host, given the sums_close key set (packed
// diagonal-major, finite = key present).  Work is split by closing diagonal.
template <class Model>
void fold_scores_host(const Model& M, bool contra, bool allows_short, const uint8_t* s, uint32_t n,
                      const float* qb, float* hp, float* mb, float* ac, rnamc_twoloop_score* tl,
                      const std::vector<uint64_t>* tl_begin, std::vector<uint64_t>* tl_count) {
  const float nan = std::numeric_limits<float>::quiet_NaN();
  const float ninf = -std::numeric_limits<float>::infinity();
  auto tri = [n](uint32_t i, uint32_t j) {
    const uint64_t d = j - i;
    return d * n - d * (d - 1ull) / 2ull + i;
  };
  const unsigned hw = std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  std::vector<std::thread> pool;
  std::atomic<uint32_t> next{0};
  auto work = [&]() {
    for (;;) {
      const uint32_t d = next.fetch_add(1);
      if (d >= n) return;
      uint64_t cnt = 0;
      uint64_t w = tl_begin ? (*tl_begin)[d] : 0;
      for (uint32_t i = 0; i + d < n; i++) {
        const uint32_t j = i + d;
        const uint64_t x = tri(i, j);
        const bool act = canonical(s[i], s[j]) &&
                         ((contra && allows_short) || d + 1 >= RNAMC_MIN_SPAN_HAIRPIN_CLOSE);
        if (!tl_begin) {
          if (hp) hp[x] = (act && (!contra || d - 1 <= RNAMC_MAX_LOOP_LEN)) ? M.hairpin(s, n, i, j) : nan;
          const bool member = act && qb[x] > ninf;
          if (mb) mb[x] = member ? M.mbclose(s, n, i, j) : nan;
          if (ac) ac[x] = member ? M.accessible(s, n, i, j) : nan;
        }
        if (!act || d < 3) continue;
        // k in i+1 .. j-2, a = k-i-1 <= 30; l from j-1 down to k+1, a + b <= 30
        for (uint32_t k = i + 1; k + 1 < j && k - i - 1 <= RNAMC_MAX_2LOOP_LEN; k++) {
          for (uint32_t l = j - 1; l > k && (j - l - 1) + (k - i - 1) <= RNAMC_MAX_2LOOP_LEN; l--) {
            if (!(qb[tri(k, l)] > ninf)) continue;
            if (tl_begin) tl[w++] = rnamc_twoloop_score{i, j, k, l, M.twoloop(s, i, j, k, l)};
            cnt++;
          }
        }
      }
      if (tl_count) (*tl_count)[d] = cnt;
    }
  };
  for (unsigned t = 1; t < hw; t++) pool.emplace_back(work);
  work();
  for (auto& t : pool) t.join();
}

// What rnamc_sample_batch and rnamc_mfe_batch do with a group once its inside sweep is enqueued: the
// walk kernel (n_samples walks per sequence) on the same stream before the next group reuses the
// workspace, then its rows, a value per walk and (MFE) a sweep value per sequence copied out and
// scattered to the caller's arrays by batch index.
struct WalkStage {
  rnamc_ctx* c;
  const char* who;
  void (*launch)(const SampleBatch&, bool contra, uint32_t n_waves, hipStream_t);
  bool contra;
  uint32_t n_seqs, n_samples;
  uint64_t seed;
  const uint64_t* offsets;
  uint8_t* structs;
  float* values;     // per walk, may be null
  bool with_dp;      // MFE: the sweep values beside the tracebacks' (mf_dp)
  float* dp_scores;  // per sequence, may be null
  int cus = 0;
  std::vector<uint64_t> rowoff;
  std::vector<uint8_t> h_rows;
  std::vector<float> h_w, h_dp;

  int init() {
    try {  // nothing may throw across the C boundary
      rowoff.resize(n_seqs);
    } catch (const std::exception&) {
      set_last_error(std::string(who) + ": no host memory");
      return RNAMC_ERR_OOM;
    }
    HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    return RNAMC_OK;
  }

  // before the first group (every group's descriptors exist): the buffers sized for the largest group
  int size_buffers() {
    uint64_t rows_max = 0, w_max = 0, seq_max = 0, stack_max = 0;
    for (size_t h = 0; h + 1 < c->group_begin.size(); h++) {
      const uint32_t gb = c->group_begin[h], ge = c->group_begin[h + 1];
      uint64_t r = 0;
      for (uint32_t x = gb; x < ge; x++) {
        rowoff[x] = r;
        r += static_cast<uint64_t>(c->descs[x].n) * n_samples;
      }
      const uint64_t items = static_cast<uint64_t>(ge - gb) * n_samples;
      const uint32_t gmax = c->descs[gb].n;
      rows_max = std::max(rows_max, r);
      w_max = std::max(w_max, items);
      seq_max = std::max<uint64_t>(seq_max, ge - gb);
      stack_max = std::max<uint64_t>(stack_max, static_cast<uint64_t>(waves_of(cus, items, gmax)) * (gmax + 1ull));
    }
    try {
      h_rows.resize(rows_max);
      h_w.resize(w_max);
      if (with_dp) h_dp.resize(seq_max);
    } catch (const std::exception&) {
      set_last_error(std::string(who) + ": no host memory for a group's rows");
      return RNAMC_ERR_OOM;
    }
    HIPCHK(c->sm_rows.grow(rows_max));
    HIPCHK(c->sm_w.grow(w_max));
    if (with_dp) HIPCHK(c->mf_dp.grow(seq_max));
    HIPCHK(c->sm_stack.grow(stack_max));
    HIPCHK(c->sm_rowoff.upload(rowoff.data(), n_seqs, c->own_stream));
    return RNAMC_OK;
  }

  int run(uint32_t first, uint32_t count) {
    SampleBatch a{};
    a.seqs = c->d_seqs + first;
    a.bases = c->st_bases;
    a.workspace = c->d_ws;
    a.params = c->d_params;
    a.hp_init = c->d_hp_init;
    a.row_off = c->sm_rowoff + first;
    a.rows = c->sm_rows;
    a.log_weights = c->sm_w;
    if (with_dp) a.dp_scores = c->mf_dp;
    a.stack = c->sm_stack;
    a.stack_cap = c->descs[first].n + 1u;
    a.nseq = count;
    a.n_samples = n_samples;
    a.seed = seed;
    const uint64_t items = static_cast<uint64_t>(count) * n_samples;
    launch(a, contra, waves_of(cus, items, c->descs[first].n), c->own_stream);
    c->stats.launches_other++;
    HIPCHK(hipGetLastError());
    const uint64_t rows = rowoff[first + count - 1] +
                          static_cast<uint64_t>(c->descs[first + count - 1].n) * n_samples;
    HIPCHK(hipMemcpyAsync(h_rows.data(), c->sm_rows, rows, hipMemcpyDeviceToHost, c->own_stream));
    HIPCHK(hipMemcpyAsync(h_w.data(), c->sm_w, items * sizeof(float), hipMemcpyDeviceToHost,
                          c->own_stream));
    if (with_dp)
      HIPCHK(hipMemcpyAsync(h_dp.data(), c->mf_dp, count * sizeof(float), hipMemcpyDeviceToHost,
                            c->own_stream));
    HIPCHK(hipStreamSynchronize(c->own_stream));
    for (uint32_t x = first; x < first + count; x++) {
      const SeqDesc& sd = c->descs[x];
      const uint64_t s = sd.batch_idx;
      std::memcpy(structs + n_samples * (offsets[s] - offsets[0]), h_rows.data() + rowoff[x],
                  static_cast<size_t>(sd.n) * n_samples);
      if (values)
        std::memcpy(values + s * n_samples, h_w.data() + static_cast<uint64_t>(x - first) * n_samples,
                    n_samples * sizeof(float));
      if (dp_scores) dp_scores[s] = h_dp[x - first];
    }
    return RNAMC_OK;
  }
};

// rnamc_bpp_batch_constrained once its arguments passed (`locked`: the caller holds c->mu).
// inside_only: the reference-order inside sweep alone, its sums left in the workspace for
// rnamc_fold_scores / rnamc_fold_sums (the triangles that reach `bpp` are then not looked at).
int bpp_host(rnamc_ctx* c, bool locked, uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
             const ConsCall& cons, bool inside_only, bool contra, bool allows_short, float* bpp,
             const uint64_t* out_offsets, float* log_partition) {
  StagedCall sc(c, locked);
  if (int rc = sc.stage(c, "rnamc_bpp_batch", n_seqs, bases, offsets, cons)) return rc;
  sc.opts.inside_only = inside_only;
  // The result is never staged whole: group g's triangles sit in st_out[g & 1] while a host
  // thread drains them (copy stream -> pinned bounce chunks -> the caller's buffers) and
  // group g+1 sweeps into the other buffer.
  constexpr uint64_t kChunkFloats = 16ull << 20;  // 64 MB bounce chunks
  if (!c->copy_stream) HIPCHK(hipStreamCreateWithFlags(c->copy_stream.put(), hipStreamNonBlocking));
  for (int k = 0; k < 2; k++) {
    if (!c->pinned[k]) HIPCHK(c->pinned[k].alloc(kChunkFloats));
    if (!c->pinned_ev[k]) HIPCHK(hipEventCreateWithFlags(c->pinned_ev[k].put(), hipEventDisableTiming));
    if (!c->group_done[k]) HIPCHK(hipEventCreateWithFlags(c->group_done[k].put(), hipEventDisableTiming));
  }

  // drain thread: one job per group, in order
  struct Job {
    size_t g;
    uint32_t first, count;
  };
  std::mutex mu;
  std::condition_variable cv;
  std::vector<Job> jobs;
  size_t jobs_taken = 0, drained = 0;  // groups handed over / fully copied out
  bool stop = false;
  int drain_err = RNAMC_OK;
  std::string drain_msg;
  const int device = c->device;
  auto drain = [&]() {
    (void)hipSetDevice(device);
    for (;;) {
      Job job;
      {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return stop || jobs_taken < jobs.size(); });
        if (jobs_taken >= jobs.size()) return;  // stop and nothing left
        job = jobs[jobs_taken++];
      }
      const int k = static_cast<int>(job.g & 1);
      hipError_t e = hipEventSynchronize(c->group_done[k]);
      const uint64_t total = c->group_out_floats[job.g];
      const float* src = c->st_out[k];
      const uint64_t nchunks = (total + kChunkFloats - 1) / kChunkFloats;
      auto issue = [&](uint64_t ch) {
        const uint64_t lo = ch * kChunkFloats, len = std::min(kChunkFloats, total - lo);
        hipError_t e2 = hipMemcpyAsync(c->pinned[ch & 1], src + lo, len * sizeof(float),
                                       hipMemcpyDeviceToHost, c->copy_stream);
        if (e2 == hipSuccess) e2 = hipEventRecord(c->pinned_ev[ch & 1], c->copy_stream);
        return e2;
      };
      uint32_t cur = job.first;  // descriptor whose triangle holds the next float to place
      if (e == hipSuccess && nchunks) e = issue(0);
      for (uint64_t ch = 0; ch < nchunks && e == hipSuccess; ch++) {
        if (ch + 1 < nchunks) e = issue(ch + 1);
        if (e == hipSuccess) e = hipEventSynchronize(c->pinned_ev[ch & 1]);
        if (e != hipSuccess) break;
        // scatter [lo, hi) of the group's staging buffer to the caller's triangles
        const uint64_t lo = ch * kChunkFloats, hi = std::min(total, lo + kChunkFloats);
        uint64_t pos = lo;
        while (pos < hi) {
          const SeqDesc& sd = c->descs[cur];
          const uint64_t s_lo = sd.out_off, s_hi = sd.out_off + rnamc_bpp_len(sd.n);
          if (pos >= s_hi) {
            cur++;
            continue;
          }
          const uint64_t upto = std::min(hi, s_hi);
          std::memcpy(bpp + out_offsets[sd.batch_idx] + (pos - s_lo), c->pinned[ch & 1] + (pos - lo),
                      (upto - pos) * sizeof(float));
          pos = upto;
        }
      }
      {
        std::lock_guard<std::mutex> lk(mu);
        if (e != hipSuccess && drain_err == RNAMC_OK) {
          drain_err = RNAMC_ERR_HIP;
          drain_msg = std::string("result drain: ") + hipGetErrorString(e);
        }
        drained++;
      }
      cv.notify_all();
    }
  };
  std::thread drainer;
  try {
    drainer = std::thread(drain);
  } catch (...) {  // no thread: nothing has been enqueued yet
    set_last_error("rnamc_bpp_batch: could not start the result-drain thread");
    return RNAMC_ERR_OOM;
  }
  GroupHooks hooks;
  hooks.before = [&](size_t g, float** out_base) -> int {
    const int k = static_cast<int>(g & 1);
    {
      // buffer k was last used by group g-2: wait until it is copied out
      std::unique_lock<std::mutex> lk(mu);
      cv.wait(lk, [&] { return g < 2 || drained + 2 > g; });
      if (drain_err) return drain_err;
    }
    // nothing on the device still writes to or reads from this buffer, but a free synchronises the
    // device: rare (buffers only grow)
    const hipError_t e = c->st_out[k].grow(std::max<uint64_t>(c->group_out_floats[g], 1));
    if (e != hipSuccess) {
      set_last_error(std::string("result staging buffer: ") + hipGetErrorString(e));
      return e == hipErrorOutOfMemory ? RNAMC_ERR_OOM : RNAMC_ERR_HIP;
    }
    *out_base = c->st_out[k];
    return RNAMC_OK;
  };
  hooks.after = [&](size_t g, uint32_t first, uint32_t count) -> int {
    HIPCHK(hipEventRecord(c->group_done[g & 1], c->own_stream));
    {
      std::lock_guard<std::mutex> lk(mu);
      jobs.push_back(Job{g, first, count});
    }
    cv.notify_all();
    return RNAMC_OK;
  };
  int rc = run_batch_mode(c, n_seqs, c->st_bases, sc.doff.data(), contra, allows_short, nullptr, out_offsets,
                          c->st_logz, c->own_stream, sc.opts, &hooks);
  {
    std::lock_guard<std::mutex> lk(mu);
    stop = true;
  }
  cv.notify_all();
  drainer.join();
  if (rc == RNAMC_OK && drain_err) {
    set_last_error(drain_msg);
    rc = drain_err;
  }
  rc = sc.finish(c, rc, n_seqs, log_partition);
  if (rc) return rc;
  for (int k = 0; k < 2; k++)  // (two group buffers stay for the next call unless huge)
    if (c->st_out[k].bytes() > (24ull << 30)) (void)c->st_out[k].reset();
  return RNAMC_OK;
}

}  // namespace

extern "C" {

int rnamc_bpp_batch_device(rnamc_ctx* c, uint32_t n_seqs, const uint8_t* d_bases,
                           const uint64_t* offsets, int uses_contra_model,
                           int allows_short_hairpins, float* d_bpp, const uint64_t* out_offsets,
                           float* d_log_partition, void* hip_stream) {
  if (!c || !offsets || !out_offsets || (n_seqs && (!d_bases || !d_bpp)))
    return RNAMC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(c->mu);
  DeviceGuard guard(c->device);
  if (!guard.ok) return RNAMC_ERR_NO_DEVICE;
  return run_batch_mode(c, n_seqs, d_bases, offsets, uses_contra_model != 0,
                        allows_short_hairpins != 0, d_bpp, out_offsets, d_log_partition,
                        static_cast<hipStream_t>(hip_stream), SweepOpts{});
}

int rnamc_bpp_batch(rnamc_ctx* c, uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
                    int uses_contra_model, int allows_short_hairpins, float* bpp,
                    const uint64_t* out_offsets, float* log_partition) {
  return rnamc_bpp_batch_constrained(c, n_seqs, bases, offsets, nullptr, 0, uses_contra_model,
                                     allows_short_hairpins, bpp, out_offsets, log_partition);
}

int rnamc_bpp_batch_constrained(rnamc_ctx* c, uint32_t n_seqs, const uint8_t* bases,
                                const uint64_t* offsets, const char* constraints, uint32_t max_bp_span,
                                int uses_contra_model, int allows_short_hairpins, float* bpp,
                                const uint64_t* out_offsets, float* log_partition) {
  if (!c || !offsets || !out_offsets || (n_seqs && (!bases || !bpp))) return RNAMC_ERR_INVALID_ARG;
  if (n_seqs == 0) return RNAMC_OK;
  if (int rc = check_records(n_seqs, bases, offsets)) return rc;
  ConsCall cons;
  if (int rc = cons.prepare(n_seqs, offsets, constraints, max_bp_span)) return rc;
  return bpp_host(c, false, n_seqs, bases, offsets, cons, false, uses_contra_model != 0,
                  allows_short_hairpins != 0, bpp, out_offsets, log_partition);
}

int rnamc_fold_scores(rnamc_ctx* c, const uint8_t* bases, uint32_t n, int uses_contra_model,
                      int allows_short_hairpins, float* hairpin_scores,
                      float* multibranch_close_scores, float* accessible_scores,
                      rnamc_twoloop_score* twoloop_scores, uint64_t twoloop_cap,
                      uint64_t* twoloop_count) {
  if (!c || !bases) return RNAMC_ERR_INVALID_ARG;
  if (n == 0) return RNAMC_ERR_EMPTY_SEQ;
  std::lock_guard<std::mutex> lock(c->mu);
  const uint64_t tri_len = rnamc_bpp_len(n);
  const bool contra = uses_contra_model != 0, shorthp = allows_short_hairpins != 0;
  const bool cached = c->fs_contra == (contra ? 1 : 0) && c->fs_short == (shorthp ? 1 : 0) &&
                      c->fs_bases.size() == n && std::memcmp(c->fs_bases.data(), bases, n) == 0 &&
                      c->fs_qb.size() == tri_len;
  if (!cached) {
    // the device sweep of this one sequence leaves sums_close in the workspace
    const uint64_t offsets[2] = {0, n}, out_offsets[2] = {0, 0};
    c->fs_contra = c->fs_short = -1;
    c->fs_qb.assign(tri_len, 0.f);
    if (int rc = check_records(1, bases, offsets)) return rc;
    DeviceGuard guard(c->device);
    if (!guard.ok) return RNAMC_ERR_NO_DEVICE;
    if (int rc = bpp_host(c, true, 1, bases, offsets, ConsCall{}, true, contra, shorthp, c->fs_qb.data(),
                          out_offsets, nullptr))
      return rc;
    const SeqDesc& sd = c->descs.back();
    // sums_close, packed diagonal-major like the result
    HIPCHK(hipMemcpy(c->fs_qb.data(),
                     c->d_ws + sd.ws_off + static_cast<uint64_t>(M_QB) * sd.tri_pad,
                     tri_len * sizeof(float), hipMemcpyDeviceToHost));
    c->fs_bases.assign(bases, bases + n);
    c->fs_contra = contra ? 1 : 0;
    c->fs_short = shorthp ? 1 : 0;
  }
  const std::vector<float>& qb = c->fs_qb;
  std::vector<uint64_t> count(n, 0), begin(n + 1, 0);
  const Turner MT{c->host_params.turner, c->h_hp_init.data()};
  const Contra MC{c->host_params.contra};
  auto pass = [&](rnamc_twoloop_score* tl, const std::vector<uint64_t>* b, std::vector<uint64_t>* k) {
    if (contra)
      fold_scores_host(MC, true, shorthp, bases, n, qb.data(), hairpin_scores,
                       multibranch_close_scores, accessible_scores, tl, b, k);
    else
      fold_scores_host(MT, false, shorthp, bases, n, qb.data(), hairpin_scores,
                       multibranch_close_scores, accessible_scores, tl, b, k);
  };
  pass(nullptr, nullptr, &count);
  for (uint32_t d = 0; d < n; d++) begin[d + 1] = begin[d] + count[d];
  if (twoloop_count) *twoloop_count = begin[n];
  if (twoloop_scores) {
    if (twoloop_cap < begin[n]) {
      set_last_error("rnamc_fold_scores: twoloop_cap is smaller than the entry count");
      return RNAMC_ERR_INVALID_ARG;
    }
    pass(twoloop_scores, &begin, nullptr);
  }
  return RNAMC_OK;
}

int rnamc_fold_sums(rnamc_ctx* c, const uint8_t* bases, uint32_t n, int uses_contra_model,
                    int allows_short_hairpins, float* sums_external,
                    float* sums_rightmost_basepairs_external,
                    float* sums_rightmost_basepairs_multibranch, float* sums_close,
                    float* sums_accessible, float* sums_multibranch,
                    float* sums_1ormore_basepairs) {
  if (!c || !bases) return RNAMC_ERR_INVALID_ARG;
  if (n == 0) return RNAMC_ERR_EMPTY_SEQ;
  if (n > RNAMC_MAX_SEQ_LEN) return RNAMC_ERR_SEQ_TOO_LONG;  // (before anything is sized by n)
  std::lock_guard<std::mutex> lock(c->mu);
  const uint64_t tri_len = rnamc_bpp_len(n);
  // the inside sweep alone (reference order whatever the context's mode is), results left in
  // the workspace; the fold-scores cache of the context is for another sequence afterwards
  const uint64_t offsets[2] = {0, n}, out_offsets[2] = {0, 0};
  c->fs_contra = c->fs_short = -1;
  std::vector<float> packed;
  try {  // nothing may throw across the C boundary
    packed.resize(tri_len);
  } catch (const std::exception&) {
    rnamc::set_last_error("rnamc_fold_sums: no host memory for a packed triangle");
    return RNAMC_ERR_OOM;
  }
  if (int rc = check_records(1, bases, offsets)) return rc;
  DeviceGuard guard(c->device);
  if (!guard.ok) return RNAMC_ERR_NO_DEVICE;
  if (int rc = bpp_host(c, true, 1, bases, offsets, ConsCall{}, true, uses_contra_model != 0,
                        allows_short_hairpins != 0, packed.data(), out_offsets, nullptr))
    return rc;
  const SeqDesc& sd = c->descs.back();
  const float ninf = -std::numeric_limits<float>::infinity();
  struct Want {
    float* out;
    int slot;       // workspace slot, or -1: the reference never writes this member in this model
    float initial;  // the reference's initial value (FoldSums::new, 213-226)
  };
  const Want wants[7] = {
      {sums_external, M_Z, 0.f},
      {sums_rightmost_basepairs_external, M_ZRE, ninf},
      {sums_rightmost_basepairs_multibranch, uses_contra_model ? M_ZRM : -1, ninf},
      {sums_close, M_QB, ninf},
      {sums_accessible, M_QA, ninf},
      {sums_multibranch, M_QM, ninf},
      {sums_1ormore_basepairs, M_Q1D, ninf},
  };
  for (const Want& w : wants) {
    if (!w.out) continue;
    for (uint64_t x = 0; x < static_cast<uint64_t>(n) * n; x++) w.out[x] = w.initial;
    if (w.slot < 0) continue;
    HIPCHK(hipMemcpy(packed.data(), c->d_ws + sd.ws_off + static_cast<uint64_t>(w.slot) * sd.tri_pad,
                     tri_len * sizeof(float), hipMemcpyDeviceToHost));
    uint64_t x = 0;  // diagonal-major: cell (i, i+d) at d*n - d(d-1)/2 + i
    for (uint32_t d = 0; d < n; d++)
      for (uint32_t i = 0; i + d < n; i++) w.out[static_cast<uint64_t>(i) * n + i + d] = packed[x++];
  }
  return RNAMC_OK;
}

// Boltzmann sampling: the reference-order inside sweep of every group (inside_only), then per
// group the sampling kernel (rnamc_sample.hip) on the same stream before the next group reuses the
// workspace, and its rows and log-weights copied out to the caller.
int rnamc_sample_batch(rnamc_ctx* c, uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
                       int uses_contra_model, int allows_short_hairpins, uint32_t n_samples,
                       uint64_t seed, uint8_t* structs, float* log_weights, float* log_partition) {
  return rnamc_sample_batch_constrained(c, n_seqs, bases, offsets, nullptr, 0, uses_contra_model,
                                        allows_short_hairpins, n_samples, seed, structs, log_weights,
                                        log_partition);
}

int rnamc_sample_batch_constrained(rnamc_ctx* c, uint32_t n_seqs, const uint8_t* bases,
                                   const uint64_t* offsets, const char* constraints,
                                   uint32_t max_bp_span, int uses_contra_model,
                                   int allows_short_hairpins, uint32_t n_samples, uint64_t seed,
                                   uint8_t* structs, float* log_weights, float* log_partition) {
  if (!c || !offsets || (n_seqs && !bases)) return RNAMC_ERR_INVALID_ARG;
  if (n_seqs == 0) return RNAMC_OK;
  if (int rc = check_records(n_seqs, bases, offsets)) return rc;
  ConsCall cons;
  if (int rc = cons.prepare(n_seqs, offsets, constraints, max_bp_span)) return rc;
  if (n_samples == 0) return RNAMC_OK;
  if (!structs) return RNAMC_ERR_INVALID_ARG;
  StagedCall sc(c, false);
  if (int rc = sc.stage(c, "rnamc_sample_batch", n_seqs, bases, offsets, cons)) return rc;
  const bool contra = uses_contra_model != 0;
  WalkStage walk{c, "rnamc_sample_batch", launch_sample, contra, n_seqs, n_samples, seed, offsets, structs,
                 log_weights, false, nullptr};
  if (int rc = walk.init()) return rc;
  GroupHooks hooks;
  hooks.before = [&](size_t g, float** out_base) -> int {
    if (g == 0)
      if (int rc = walk.size_buffers()) return rc;
    return group_triangles(c, g, out_base);
  };
  hooks.after = [&](size_t, uint32_t first, uint32_t count) -> int { return walk.run(first, count); };
  sc.opts.inside_only = true;  // the reference-order sweep whatever summation_mode says
  const int rc = run_batch_mode(c, n_seqs, c->st_bases, sc.doff.data(), contra, allows_short_hairpins != 0,
                                nullptr, nullptr, c->st_logz, c->own_stream, sc.opts, &hooks);
  return sc.finish(c, rc, n_seqs, log_partition);
}

// ln Z alone: the reference-order inside sweep of every group (inside_only: no outside sweep) and
// the finalize kernel that writes sums_external[0][n-1] -- the launches the sampler makes before it
// samples, so the value is rnamc_bpp_batch's log_partition in summation_mode 0 bit for bit.
int rnamc_log_partition_batch(rnamc_ctx* c, uint32_t n_seqs, const uint8_t* bases,
                              const uint64_t* offsets, const char* constraints, uint32_t max_bp_span,
                              int uses_contra_model, int allows_short_hairpins, float* log_partition) {
  if (!c || !offsets || (n_seqs && (!bases || !log_partition))) return RNAMC_ERR_INVALID_ARG;
  if (n_seqs == 0) return RNAMC_OK;
  if (int rc = check_records(n_seqs, bases, offsets)) return rc;
  ConsCall cons;
  if (int rc = cons.prepare(n_seqs, offsets, constraints, max_bp_span)) return rc;
  StagedCall sc(c, false);
  if (int rc = sc.stage(c, "rnamc_log_partition_batch", n_seqs, bases, offsets, cons)) return rc;
  GroupHooks hooks;
  hooks.before = [&](size_t g, float** out_base) -> int { return group_triangles(c, g, out_base); };
  hooks.after = [](size_t, uint32_t, uint32_t) -> int { return RNAMC_OK; };
  sc.opts.inside_only = true;  // the reference-order sweep whatever summation_mode says
  const int rc = run_batch_mode(c, n_seqs, c->st_bases, sc.doff.data(), uses_contra_model != 0,
                                allows_short_hairpins != 0, nullptr, nullptr, c->st_logz, c->own_stream, sc.opts,
                                &hooks);
  return sc.finish(c, rc, n_seqs, log_partition);
}

// Maximum-score structure: the max-plus inside sweep of every group (maxplus, run_batch), then per
// group the argmax traceback (rnamc_mfe.hip) on the same stream before the next group reuses the
// workspace, and its rows and scores copied out to the caller.
int rnamc_mfe_batch(rnamc_ctx* c, uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
                    int uses_contra_model, int allows_short_hairpins, uint8_t* structs, float* scores,
                    float* dp_scores) {
  return rnamc_mfe_batch_constrained(c, n_seqs, bases, offsets, nullptr, 0, uses_contra_model,
                                     allows_short_hairpins, structs, scores, dp_scores);
}

int rnamc_mfe_batch_constrained(rnamc_ctx* c, uint32_t n_seqs, const uint8_t* bases,
                                const uint64_t* offsets, const char* constraints, uint32_t max_bp_span,
                                int uses_contra_model, int allows_short_hairpins, uint8_t* structs,
                                float* scores, float* dp_scores) {
  if (!c || !offsets || (n_seqs && !bases)) return RNAMC_ERR_INVALID_ARG;
  if (n_seqs == 0) return RNAMC_OK;
  if (int rc = check_records(n_seqs, bases, offsets)) return rc;
  if (!structs) return RNAMC_ERR_INVALID_ARG;
  ConsCall cons;
  if (int rc = cons.prepare(n_seqs, offsets, constraints, max_bp_span)) return rc;
  StagedCall sc(c, false);
  if (int rc = sc.stage(c, "rnamc_mfe_batch", n_seqs, bases, offsets, cons, false)) return rc;
  const bool contra = uses_contra_model != 0;
  // (one walk per sequence: its traceback)
  WalkStage walk{c, "rnamc_mfe_batch", launch_mfe_trace, contra, n_seqs, 1, 0, offsets, structs, scores, true,
                 dp_scores};
  if (int rc = walk.init()) return rc;
  GroupHooks hooks;
  hooks.before = [&](size_t g, float**) -> int { return g == 0 ? walk.size_buffers() : RNAMC_OK; };
  hooks.after = [&](size_t, uint32_t first, uint32_t count) -> int { return walk.run(first, count); };
  sc.opts.inside_only = sc.opts.maxplus = true;  // run_batch whatever summation_mode says
  const int rc = run_batch_mode(c, n_seqs, c->st_bases, sc.doff.data(), contra, allows_short_hairpins != 0,
                                nullptr, nullptr, nullptr, c->own_stream, sc.opts, &hooks);
  return sc.finish(c, rc, n_seqs, nullptr);
}

int rnamc_durbin_batch(rnamc_ctx* c, const rnamc_align_scores* scores, uint32_t n_seqs,
                       const uint8_t* bases, const uint64_t* offsets, uint32_t n_pairs,
                       const uint32_t* pair_a, const uint32_t* pair_b, float* match_probs,
                       const uint64_t* out_offsets) {
  if (!c || !scores || !offsets || (n_seqs && !bases) ||
      (n_pairs && (!pair_a || !pair_b || !match_probs || !out_offsets)))
    return RNAMC_ERR_INVALID_ARG;
  if (n_pairs == 0) return RNAMC_OK;
  // real bases inside, anything (PSEUDO_BASE) at the two ends, which are never scored
  if (int rc = check_records(n_seqs, bases, offsets, 1)) return rc;
  std::lock_guard<std::mutex> lock(c->mu);
  DeviceGuard guard(c->device);
  if (!guard.ok) return RNAMC_ERR_NO_DEVICE;
  hipStream_t st = c->own_stream;
  const uint64_t base_lo = offsets[0], base_hi = offsets[n_seqs];
  DevBuf<uint8_t> d_bases;
  DevBuf<DurbinPair> d_pairs;
  DevBuf<float> d_out;
  // declared after the buffers, so run before they are released: whatever still uses them is done
  struct Drain {
    hipStream_t st;
    ~Drain() { (void)hipStreamSynchronize(st); }
  } drain{st};
  HIPCHK(d_bases.replace_exact(std::max<uint64_t>(base_hi - base_lo, 1)));
  HIPCHK(hipMemcpyAsync(d_bases, bases + base_lo, base_hi - base_lo, hipMemcpyHostToDevice, st));
  // pairs in chunks whose six matrices per pair fit the workspace budget
  const uint64_t ws_cap = static_cast<uint64_t>(std::max<int64_t>(c->group_ws_bytes, 1)) / 4;
  std::vector<DurbinPair> chunk;
  std::vector<float> h_out;
  for (uint32_t p0 = 0; p0 < n_pairs;) {
    chunk.clear();
    uint64_t ws = 0, out = 0;
    uint32_t max_cells = 0, p = p0;
    for (; p < n_pairs; p++) {
      if (pair_a[p] >= n_seqs || pair_b[p] >= n_seqs) return RNAMC_ERR_INVALID_ARG;
      DurbinPair dp{};
      dp.n1 = static_cast<uint32_t>(offsets[pair_a[p] + 1] - offsets[pair_a[p]]);
      dp.n2 = static_cast<uint32_t>(offsets[pair_b[p] + 1] - offsets[pair_b[p]]);
      const uint64_t cells = static_cast<uint64_t>(dp.n1) * dp.n2;
      // (k_durbin_probs indexes pairs through blockIdx.y: at most 65535 per launch)
      if (!chunk.empty() && (ws + 6 * cells > ws_cap || chunk.size() >= 65535u)) break;
      dp.a_off = offsets[pair_a[p]] - base_lo;
      dp.b_off = offsets[pair_b[p]] - base_lo;
      dp.ws_off = ws;
      dp.out_off = out;
      chunk.push_back(dp);
      ws += 6 * cells;
      out += cells;
      max_cells = static_cast<uint32_t>(std::min<uint64_t>(std::max<uint64_t>(max_cells, cells), 0xFFFFFFFFull));
    }
    if (int rc = ensure_ws(c, ws)) return rc;
    // (the chunk before is copied out: nothing uses its buffers)
    HIPCHK(d_pairs.replace_exact(chunk.size()));
    HIPCHK(d_out.replace_exact(out));
    HIPCHK(hipMemcpyAsync(d_pairs, chunk.data(), chunk.size() * sizeof(DurbinPair), hipMemcpyHostToDevice, st));
    launch_durbin(d_pairs, static_cast<uint32_t>(chunk.size()), max_cells, d_bases, c->d_ws, d_out,
                  *scores, st);
    HIPCHK(hipGetLastError());
    // one D2H per chunk, scattered on the host (a FASTA of many short records makes tens of
    // thousands of pairs: one copy each would cost more than the sweeps)
    try {
      h_out.resize(out);
    } catch (...) {
      return RNAMC_ERR_OOM;
    }
    HIPCHK(hipMemcpyAsync(h_out.data(), d_out, out * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (size_t x = 0; x < chunk.size(); x++)
      std::memcpy(match_probs + out_offsets[p0 + x], h_out.data() + chunk[x].out_off,
                  static_cast<uint64_t>(chunk[x].n1) * chunk[x].n2 * sizeof(float));
    p0 = p;
  }
  return RNAMC_OK;
}

}  // extern "C"
