// rnamc_entries_centroid.cpp — the centroid-fold entries of the C ABI: rnamc_centroid_fold_multi on a
// caller's triangle, and rnamc_centroid_fold_batch (bpp sweep and centroid stage group by group).
#include "rnamc_entries.h"

using namespace rnamc;

extern "C" {

int rnamc_centroid_fold_multi(rnamc_ctx* c, const float* bpp_packed, uint32_t n,
                              const float* centroid_thresholds, uint32_t n_thresholds,
                              uint32_t* pairs_out, uint32_t max_pairs, uint32_t* n_pairs,
                              float* expect_accuracy) {
  if (!c || !bpp_packed || !centroid_thresholds || !n_pairs || n == 0 || n_thresholds == 0)
    return RNAMC_ERR_INVALID_ARG;
  if (n > RNAMC_MAX_SEQ_LEN) return RNAMC_ERR_SEQ_TOO_LONG;
  if (n_thresholds > 65535u) return RNAMC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(c->mu);
  DeviceGuard guard(c->device);
  if (!guard.ok) return RNAMC_ERR_NO_DEVICE;
  hipStream_t st = c->own_stream;
  const uint32_t ld = ((n + 31u) & ~31u) + 32u;
  const uint64_t msz = ((static_cast<uint64_t>(ld) * n + 63ull) & ~63ull) + 64ull;
  const uint64_t tri = rnamc_bpp_len(n);
  // workspace: per threshold two matrices, then the bpp triangle and the thresholds
  const uint64_t mats = 2ull * msz * n_thresholds;
  const uint64_t need = mats + ((tri + 63ull) & ~63ull) + ((n_thresholds + 63ull) & ~63ull);
  HIPCHK(hipStreamSynchronize(st));
  int rc = ensure_ws(c, need);
  if (rc) return rc;
  float* d_m = c->d_ws;
  float* d_bpp = d_m + mats;
  float* d_g = d_bpp + ((tri + 63ull) & ~63ull);
  HIPCHK(hipMemsetAsync(d_m, 0, mats * sizeof(float), st));  // M = 0 below and on the diagonal
  HIPCHK(hipMemcpyAsync(d_bpp, bpp_packed, tri * sizeof(float), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemcpyAsync(d_g, centroid_thresholds, n_thresholds * sizeof(float), hipMemcpyHostToDevice, st));
  CentroidBatch a{};
  a.bpp = d_bpp;
  a.m = d_m;
  a.gammas = d_g;
  a.n = n;
  a.ld = ld;
  a.msz = msz;
  for (uint32_t d = 1; d < n; d++) launch_centroid(a, d, n_thresholds, st);
  HIPCHK(hipGetLastError());
  // the row-major matrices back to the host; traceback per threshold on host threads
  std::vector<float> host;
  try {
    host.resize(static_cast<size_t>(msz) * n_thresholds);
  } catch (...) {
    (void)hipStreamSynchronize(st);
    return RNAMC_ERR_OOM;
  }
  for (uint32_t g = 0; g < n_thresholds; g++)
    HIPCHK(hipMemcpyAsync(host.data() + static_cast<size_t>(g) * msz, d_m + 2ull * msz * g,
                          msz * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  auto prob = [&](uint32_t i, uint32_t j) { return bpp_packed[rnamc_bpp_index(n, i, j)]; };
  std::atomic<uint32_t> next{0};
  auto work = [&]() {
    for (;;) {
      const uint32_t g = next.fetch_add(1);
      if (g >= n_thresholds) return;
      const float* m = host.data() + static_cast<size_t>(g) * msz;
      auto M = [&](size_t r, size_t col) { return m[r * ld + col]; };
      n_pairs[g] = centroid_traceback(n, centroid_thresholds[g], M, prob,
                                      pairs_out ? pairs_out + static_cast<size_t>(g) * 2u * max_pairs : nullptr,
                                      max_pairs);
      if (expect_accuracy) expect_accuracy[g] = M(0, n - 1);
    }
  };
  const unsigned hw = std::max(1u, std::min<unsigned>({16u, std::thread::hardware_concurrency(), n_thresholds}));
  std::vector<std::thread> pool;
  for (unsigned t = 1; t < hw; t++) {
    try {
      pool.emplace_back(work);
    } catch (...) {
      break;
    }
  }
  work();
  for (auto& t : pool) t.join();
  return RNAMC_OK;
}

}  // extern "C"

namespace rnamc {

int CentroidStage::init(rnamc_ctx* c, const char* entry) {
  who = entry;
  HIPCHK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
  return RNAMC_OK;
}

int CentroidStage::run(rnamc_ctx* c, const float* d_bpp, const CentroidSeq* seqs, uint32_t count,
                       const float* gammas, uint32_t ng, const CentroidEmit& emit) {
  hipStream_t st = c->own_stream;
  uint64_t budget = c->ws_floats;
  if (c->centroid_chunk_bytes > 0)
    budget = std::min<uint64_t>(budget, static_cast<uint64_t>(c->centroid_chunk_bytes) / 4);
  // Exact shortcut: with p_max the sequence's largest probability, fl(g * p_max) - 1 <= 0 makes every
  // pair candidate ((0 + g*p) - 1) <= 0 (rounding is monotone), so by induction over the diagonals
  // every M stays 0: the fold is empty, its accuracy +0.  p_max comes from the device triangle; such
  // items (every threshold <= 1 of the reference's grid unless a probability rounds above 1) are
  // answered here and never reach the fill.
  try {
    items.clear();
    for (uint32_t x = 0; x < count; x++) {
      CentroidItem it{};
      it.bpp_off = seqs[x].bpp_off;
      it.n = seqs[x].n;
      items.push_back(it);
    }
    h_acc.resize(count);
    ids.clear();
  } catch (const std::exception&) {
    set_last_error(std::string(who) + ": no host memory for a group");
    return RNAMC_ERR_OOM;
  }
  HIPCHK(c->cf_acc.grow(count));
  HIPCHK(c->cf_items.upload(items.data(), count, st));
  launch_centroid_pmax(c->cf_items, d_bpp, c->cf_acc, count, st);
  launches++;
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h_acc.data(), c->cf_acc, count * sizeof(float), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  try {
    for (uint32_t x = 0; x < count; x++) {
      const float p_max = h_acc[x];
      for (uint32_t gi = 0; gi < ng; gi++) {
        const float g = gammas[gi];
        const float prod = g * p_max;
        const float cand = prod - 1.f;
        const bool empty = !std::isnan(g) && (!(p_max >= -0.5f) || cand <= 0.f);
        if (!empty) {
          ids.push_back(static_cast<uint64_t>(x) * ng + gi);
          continue;
        }
        emit(x, gi, nullptr, 0u, 0.f);
      }
    }
  } catch (const std::exception&) {
    set_last_error(std::string(who) + ": no host memory for a group");
    return RNAMC_ERR_OOM;
  }
  const uint64_t total_items = ids.size();
  uint64_t done = 0;
  while (done < total_items) {
    // items in (sequence, threshold) order: longest sequence first
    try {
      items.clear();
      item_seq.clear();
      uint64_t m_floats = 0, row_bytes = 0;
      while (done + items.size() < total_items && items.size() < 65535u) {
        const uint64_t id = ids[done + items.size()];
        const uint32_t x = static_cast<uint32_t>(id / ng);
        const uint64_t need = centroid_item_floats(seqs[x].n);
        if (!items.empty() && m_floats + need > budget) break;
        CentroidItem it{};
        it.m_off = m_floats;
        it.bpp_off = seqs[x].bpp_off;
        it.row_off = row_bytes;
        it.n = seqs[x].n;
        it.gamma = gammas[id % ng];
        items.push_back(it);
        item_seq.push_back(x);
        m_floats += need;
        row_bytes += seqs[x].n;
      }
      h_rows.resize(row_bytes);
      h_np.resize(items.size());
      h_acc.resize(items.size());
    } catch (const std::exception&) {
      set_last_error(std::string(who) + ": no host memory for a chunk");
      return RNAMC_ERR_OOM;
    }
    const uint32_t ni = static_cast<uint32_t>(items.size());
    const uint32_t cmax = items[0].n;
    const uint64_t row_bytes = h_rows.size();
    const uint32_t waves = waves_of(cus, ni, cmax);
    HIPCHK(c->cf_np.grow(ni));
    HIPCHK(c->cf_acc.grow(ni));
    HIPCHK(c->sm_rows.grow(row_bytes));
    HIPCHK(c->sm_stack.grow(static_cast<uint64_t>(waves) * (cmax + 1ull)));
    HIPCHK(c->cf_items.upload(items.data(), ni, st));
    CentroidChunk a{};
    a.items = c->cf_items;
    a.bpp = d_bpp;
    a.m = c->d_ws;
    a.rows = c->sm_rows;
    a.n_pairs = c->cf_np;
    a.expect_accuracy = c->cf_acc;
    a.stack = c->sm_stack;
    a.n_items = ni;
    a.stack_cap = cmax + 1u;
    launch_centroid_batch_init(a, cmax, st);
    uint32_t active = ni;  // items with n > d: a prefix that only shrinks
    for (uint32_t d = 1; d < cmax; d++) {
      while (active > 0 && items[active - 1].n <= d) active--;
      launch_centroid_batch(a, d, active, cmax, st);
    }
    launch_centroid_trace(a, waves, st);
    launches += cmax + 1ull;
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(h_rows.data(), c->sm_rows, row_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_np.data(), c->cf_np, ni * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(h_acc.data(), c->cf_acc, ni * sizeof(float), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (uint32_t x = 0; x < ni; x++) {
      if (h_np[x] == 0xffffffffu) {
        set_last_error(std::string(who) + ": traceback stack overflow");
        return RNAMC_ERR_HIP;
      }
      emit(item_seq[x], static_cast<uint32_t>(ids[done + x] % ng), h_rows.data() + items[x].row_off, h_np[x],
           h_acc[x]);
    }
    done += ni;
  }
  return RNAMC_OK;
}

// rnamc_centroid_fold_batch behind both of its entries: the bpp sweep of the context's summation
// mode, group by group, and per group the centroid stage (rnamc_centroid_batch.hip) on the group's
// device-resident triangles before the next group reuses the workspace.  Sequence s writes its rows
// at structs + n_thresholds * place.base(s) and its per-threshold results at index place.idx(s) *
// n_thresholds (log_partition at place.idx(s)): the pool's shards address the caller's arrays with them.
int centroid_fold_batch_core(rnamc_ctx* c, uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
                             const char* constraints, uint32_t max_bp_span, int uses_contra_model,
                             int allows_short_hairpins, const float* gammas, uint32_t ng, uint8_t* structs,
                             const Place& place, uint32_t* n_pairs, float* expect_accuracy,
                             float* log_partition, float* bpp, const uint64_t* out_offsets) {
  ConsCall cons;
  if (int rc = cons.prepare(n_seqs, offsets, constraints, max_bp_span)) return rc;
  StagedCall sc(c, false);
  if (int rc = sc.stage(c, "rnamc_centroid_fold_batch", n_seqs, bases, offsets, cons)) return rc;
  CentroidStage stage;
  if (int rc = stage.init(c, "rnamc_centroid_fold_batch")) return rc;
  std::vector<CentroidSeq> seqs;
  std::vector<float> h_logz;
  try {  // nothing may throw across the C boundary
    h_logz.resize(n_seqs);
  } catch (const std::exception&) {
    set_last_error("rnamc_centroid_fold_batch: no host memory");
    return RNAMC_ERR_OOM;
  }
  hipStream_t st = c->own_stream;  // (a call with hooks never takes the two-stream route of the tree order)
  GroupHooks hooks;
  // (the group's triangles stay on the device, at group-local offsets)
  hooks.before = [&](size_t g, float** out_base) -> int { return group_triangles(c, g, out_base); };
  hooks.after = [&](size_t, uint32_t first, uint32_t count) -> int {
    // the group's sweep and finalize kernel are enqueued on `st`: its DP workspace is dead, the
    // (max,+) triangles of a chunk of items live there
    try {
      seqs.clear();
      for (uint32_t x = first; x < first + count; x++) seqs.push_back(CentroidSeq{c->descs[x].out_off, c->descs[x].n});
    } catch (const std::exception&) {
      set_last_error("rnamc_centroid_fold_batch: no host memory for a group");
      return RNAMC_ERR_OOM;
    }
    const int rc = stage.run(c, c->st_out[0], seqs.data(), count, gammas, ng,
                             [&](uint32_t x, uint32_t gi, const uint8_t* row, uint32_t np, float acc) {
                               const SeqDesc& sd = c->descs[first + x];
                               const uint32_t s = sd.batch_idx;
                               uint8_t* to = structs + ng * place.base(s, offsets) + uint64_t{gi} * sd.n;
                               if (row) std::memcpy(to, row, sd.n); else std::memset(to, '.', sd.n);
                               const uint64_t r = static_cast<uint64_t>(place.idx(s)) * ng + gi;
                               if (n_pairs) n_pairs[r] = np;
                               if (expect_accuracy) expect_accuracy[r] = acc;
                             });
    if (rc) return rc;
    if (bpp) {
      for (uint32_t x = first; x < first + count; x++) {
        const SeqDesc& sd = c->descs[x];
        HIPCHK(hipMemcpyAsync(bpp + out_offsets[sd.batch_idx], c->st_out[0] + sd.out_off,
                              rnamc_bpp_len(sd.n) * sizeof(float), hipMemcpyDeviceToHost, st));
      }
      HIPCHK(hipStreamSynchronize(st));
    }
    return RNAMC_OK;
  };
  int rc = run_batch_mode(c, n_seqs, c->st_bases, sc.doff.data(), uses_contra_model != 0,
                          allows_short_hairpins != 0, nullptr, nullptr, c->st_logz, st, sc.opts, &hooks);
  c->stats.launches_other += stage.launches;
  rc = sc.finish(c, rc, n_seqs, log_partition ? h_logz.data() : nullptr);
  if (rc) return rc;
  if (log_partition)
    for (uint32_t s = 0; s < n_seqs; s++) log_partition[place.idx(s)] = h_logz[s];
  return RNAMC_OK;
}

// argument checks shared by rnamc_centroid_fold_batch and rnamc_centroid_fold_batch_multi: nothing
// of the context or pool is read before they pass
int centroid_fold_batch_check(uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
                              const float* gammas, uint32_t ng, const uint8_t* structs, const float* bpp,
                              const uint64_t* out_offsets) {
  if (!offsets || ng == 0 || ng > 65535u || !gammas || (bpp == nullptr) != (out_offsets == nullptr) ||
      (n_seqs && (!bases || !structs)))
    return RNAMC_ERR_INVALID_ARG;
  return check_records(n_seqs, bases, offsets);
}

}  // namespace rnamc

extern "C" {

int rnamc_centroid_fold_batch(rnamc_ctx* c, uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
                              const char* constraints, uint32_t max_bp_span, int uses_contra_model,
                              int allows_short_hairpins, const float* centroid_thresholds,
                              uint32_t n_thresholds, uint8_t* structs, uint32_t* n_pairs,
                              float* expect_accuracy, float* log_partition, float* bpp,
                              const uint64_t* out_offsets) {
  if (!c) return RNAMC_ERR_INVALID_ARG;
  if (int rc = centroid_fold_batch_check(n_seqs, bases, offsets, centroid_thresholds, n_thresholds, structs,
                                         bpp, out_offsets))
    return rc;
  if (n_seqs == 0) return RNAMC_OK;
  return centroid_fold_batch_core(c, n_seqs, bases, offsets, constraints, max_bp_span, uses_contra_model,
                                  allows_short_hairpins, centroid_thresholds, n_thresholds, structs, Place(), n_pairs,
                                  expect_accuracy, log_partition, bpp, out_offsets);
}

}  // extern "C"
