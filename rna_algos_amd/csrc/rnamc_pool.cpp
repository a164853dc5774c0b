// rnamc_pool.cpp — the batch entry over SEVERAL devices behind the C ABI.
//
// The reference fans a FASTA out over all cores inside the binary, one pool task per record
// (src/bin/mccaskill_algo.rs:58-93, src/bin/centroid_fold.rs:119-132).  The drop-in's
// equivalent is one device context + one host thread per GPU: the batch is cut into as many
// shards as there are contexts, every shard runs through rnamc_bpp_batch of its own context
// (H2D, sweeps, D2H on that device's streams) and writes straight into the caller's host
// triangles.  Sequences are independent and never split: there is no
// collective and no device-to-device traffic.
//
// Shards are contiguous bands of the cost-sorted batch with equal total cost under the
// measured model of one sweep (a * n(n^2-1)/6 + b * n^2: the Theta(n^3) folds plus the
// Theta(496 n^2) 2-loop blocks), so every device's lock-step groups hold
// sequences of similar length and stay large on every diagonal.
#include <algorithm>
#include <cstring>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include <hip/hip_runtime.h>

#include "rnamc_ctx.h"
#include "rnamc_internal.h"

struct rnamc_pool {
  std::vector<rnamc_ctx*> ctxs;
  std::vector<int> devices;
  std::mutex mu;  // one batch at a time per pool
};

namespace {

double sweep_cost(uint64_t n) {
  const double x = static_cast<double>(n);
  return RNAMC_COST_S_PER_CELL_K * (x * (x * x - 1.0) / 6.0) + RNAMC_COST_S_PER_N2 * x * x;
}

// shard of every sequence: bands of the cost-sorted order (longest first, stable) with equal
// total cost; cut k lies at the first position whose running cost reaches k / n_shards of the
// total (the position itself goes to the next band, as numpy.searchsorted(side="left") cuts)
void plan(uint32_t n_seqs, const uint64_t* offsets, uint32_t n_shards, uint32_t* shard_of_seq,
          std::vector<uint32_t>* order_out) {
  n_shards = std::min(n_shards, std::max(n_seqs, 1u));  // fewer sequences than shards: one each
  std::vector<uint32_t> order(n_seqs);
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    return (offsets[a + 1] - offsets[a]) > (offsets[b + 1] - offsets[b]);
  });
  std::vector<double> csum(n_seqs);
  double run = 0.0;
  for (uint32_t x = 0; x < n_seqs; x++) {
    run += sweep_cost(offsets[order[x] + 1] - offsets[order[x]]);
    csum[x] = run;
  }
  std::vector<uint32_t> cuts;
  for (uint32_t k = 1; k < n_shards; k++) {
    uint32_t cut = static_cast<uint32_t>(
        std::lower_bound(csum.begin(), csum.end(), run * static_cast<double>(k) / n_shards) - csum.begin());
    // no empty band while there are sequences to give (a few sequences of very different cost:
    // one per device beats two idle devices)
    if (n_seqs >= n_shards) {
      const uint32_t lo = (cuts.empty() ? 0u : cuts.back()) + 1u, hi = n_seqs - (n_shards - k);
      cut = std::min(std::max(cut, lo), hi);
    }
    cuts.push_back(cut);
  }
  uint32_t shard = 0;
  for (uint32_t x = 0; x < n_seqs; x++) {
    while (shard + 1 < n_shards && cuts[shard] <= x) shard++;  // past every cut at or before x
    shard_of_seq[order[x]] = shard;
  }
  if (order_out) *order_out = std::move(order);
}

}  // namespace

extern "C" {

int rnamc_sweep_cost(uint32_t count, const uint64_t* lengths, double* cost_s) {
  if (count && (!lengths || !cost_s)) return RNAMC_ERR_INVALID_ARG;
  for (uint32_t x = 0; x < count; x++) cost_s[x] = sweep_cost(lengths[x]);
  return RNAMC_OK;
}

int rnamc_shard_plan(uint32_t n_seqs, const uint64_t* offsets, uint32_t n_shards,
                     uint32_t* shard_of_seq) {
  if (!offsets || !shard_of_seq || n_shards == 0) return RNAMC_ERR_INVALID_ARG;
  for (uint32_t s = 0; s < n_seqs; s++)
    if (offsets[s + 1] < offsets[s]) return RNAMC_ERR_INVALID_ARG;
  if (n_seqs) plan(n_seqs, offsets, n_shards, shard_of_seq, nullptr);
  return RNAMC_OK;
}

int rnamc_pool_create(const rnamc_params* params, const int* devices, uint32_t n_devices,
                      uint64_t workspace_bytes, rnamc_pool** out) {
  if (!params || !out || (n_devices && !devices)) return RNAMC_ERR_INVALID_ARG;
  *out = nullptr;
  std::vector<int> devs;
  if (n_devices == 0) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
      rnamc::set_last_error("no HIP device visible: librnamc has no CPU fallback");
      return RNAMC_ERR_NO_DEVICE;
    }
    for (int d = 0; d < count; d++) devs.push_back(d);
  } else {
    devs.assign(devices, devices + n_devices);
  }
  rnamc_pool* p = new (std::nothrow) rnamc_pool();
  if (!p) return RNAMC_ERR_OOM;
  for (int d : devs) {
    rnamc_ctx* c = nullptr;
    const int rc = rnamc_ctx_create(params, d, workspace_bytes, &c);
    if (rc) {
      rnamc_pool_destroy(p);
      return rc;
    }
    p->ctxs.push_back(c);
    p->devices.push_back(d);
  }
  *out = p;
  return RNAMC_OK;
}

void rnamc_pool_destroy(rnamc_pool* p) {
  if (!p) return;
  for (rnamc_ctx* c : p->ctxs) rnamc_ctx_destroy(c);
  delete p;
}

uint32_t rnamc_pool_size(const rnamc_pool* p) { return p ? static_cast<uint32_t>(p->ctxs.size()) : 0u; }

rnamc_ctx* rnamc_pool_ctx(rnamc_pool* p, uint32_t idx) {
  return (p && idx < p->ctxs.size()) ? p->ctxs[idx] : nullptr;
}

int rnamc_pool_set_params(rnamc_pool* p, const rnamc_params* params) {
  if (!p || !params) return RNAMC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(p->mu);
  for (rnamc_ctx* c : p->ctxs)
    if (int rc = rnamc_ctx_set_params(c, params)) return rc;
  return RNAMC_OK;
}

int rnamc_pool_set(rnamc_pool* p, const char* name, int64_t value) {
  if (!p || !name) return RNAMC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(p->mu);
  for (rnamc_ctx* c : p->ctxs)
    if (int rc = rnamc_ctx_set(c, name, value)) return rc;
  return RNAMC_OK;
}

int rnamc_bpp_batch_multi(rnamc_pool* p, uint32_t n_seqs, const uint8_t* bases,
                          const uint64_t* offsets, int uses_contra_model,
                          int allows_short_hairpins, float* bpp, const uint64_t* out_offsets,
                          float* log_partition) {
  return rnamc_bpp_batch_multi_constrained(p, n_seqs, bases, offsets, nullptr, 0, uses_contra_model,
                                           allows_short_hairpins, bpp, out_offsets, log_partition);
}

int rnamc_bpp_batch_multi_constrained(rnamc_pool* p, uint32_t n_seqs, const uint8_t* bases,
                                      const uint64_t* offsets, const char* constraints,
                                      uint32_t max_bp_span, int uses_contra_model,
                                      int allows_short_hairpins, float* bpp,
                                      const uint64_t* out_offsets, float* log_partition) {
  if (!p || p->ctxs.empty() || !offsets || !out_offsets || (n_seqs && (!bases || !bpp)))
    return RNAMC_ERR_INVALID_ARG;
  if (n_seqs == 0) return RNAMC_OK;
  // the whole batch is validated before any device sees a part of it: one bad record fails the
  // call with its status and nothing is computed (the reference panics before its pool starts
  // for bad bytes, src/bin/mccaskill_algo.rs:50-56)
  for (uint32_t s = 0; s < n_seqs; s++) {
    if (offsets[s + 1] < offsets[s]) return RNAMC_ERR_INVALID_ARG;
    const uint64_t n = offsets[s + 1] - offsets[s];
    if (n == 0) return RNAMC_ERR_EMPTY_SEQ;
    if (n > RNAMC_MAX_SEQ_LEN) return RNAMC_ERR_SEQ_TOO_LONG;
    for (uint64_t x = offsets[s]; x < offsets[s + 1]; x++)
      if (bases[x] > 3) return RNAMC_ERR_INVALID_BASE;
  }
  if (constraints) {  // (the span limit needs no check)
    std::vector<int32_t> words;
    for (uint32_t s = 0; s < n_seqs; s++) {
      const uint32_t n = static_cast<uint32_t>(offsets[s + 1] - offsets[s]);
      uint32_t bad = 0;
      const char* why = "";
      int rc = RNAMC_OK;
      try {  // nothing may throw across the C boundary
        words.resize(2ull * n);
        rc = rnamc::compile_constraint(constraints + (offsets[s] - offsets[0]), n, words.data(), &bad, &why);
      } catch (const std::exception&) {
        rnamc::set_last_error("constraints: no host memory");
        return RNAMC_ERR_OOM;
      }
      if (rc) {
        rnamc::set_last_error("constraint of record " + std::to_string(s) + ", position " +
                              std::to_string(bad) + ": " + why);
        return rc;
      }
    }
  }
  std::lock_guard<std::mutex> lock(p->mu);
  const uint32_t n_shards = static_cast<uint32_t>(std::min<size_t>(p->ctxs.size(), n_seqs));
  std::vector<uint32_t> shard_of(n_seqs), order;
  plan(n_seqs, offsets, n_shards, shard_of.data(), &order);
  struct Shard {
    std::vector<uint32_t> members;  // batch indices, longest first
    std::vector<uint8_t> bases;
    std::vector<char> cons;  // the members' constraint strings (when the call has them)
    std::vector<uint64_t> offsets, out_offsets;
    std::vector<float> logz;
    int status = RNAMC_OK;
    std::string error;
  };
  std::vector<Shard> shards(n_shards);
  for (uint32_t x = 0; x < n_seqs; x++) shards[shard_of[order[x]]].members.push_back(order[x]);
  for (Shard& sh : shards) {
    uint64_t total = 0;
    for (uint32_t s : sh.members) total += offsets[s + 1] - offsets[s];
    sh.bases.resize(total);
    if (constraints) sh.cons.resize(total);
    sh.offsets.assign(1, 0);
    for (uint32_t s : sh.members) {
      const uint64_t n = offsets[s + 1] - offsets[s];
      std::memcpy(sh.bases.data() + sh.offsets.back(), bases + offsets[s], n);
      if (constraints) std::memcpy(sh.cons.data() + sh.offsets.back(), constraints + (offsets[s] - offsets[0]), n);
      sh.offsets.push_back(sh.offsets.back() + n);
      sh.out_offsets.push_back(out_offsets[s]);  // results go straight into the caller's triangles
    }
    sh.out_offsets.push_back(0);  // (entry n of the prefix form: unused by rnamc_bpp_batch)
    sh.logz.resize(sh.members.size());
  }
  auto work = [&](uint32_t k) {
    Shard& sh = shards[k];
    if (sh.members.empty()) return;
    sh.status = rnamc_bpp_batch_constrained(
        p->ctxs[k], static_cast<uint32_t>(sh.members.size()), sh.bases.data(), sh.offsets.data(),
        constraints ? sh.cons.data() : nullptr, max_bp_span, uses_contra_model, allows_short_hairpins, bpp,
        sh.out_offsets.data(), log_partition ? sh.logz.data() : nullptr);
    if (sh.status) sh.error = rnamc_last_error();  // (thread-local: carry it to the caller's thread)
  };
  std::vector<std::thread> pool;
  for (uint32_t k = 1; k < n_shards; k++) {
    try {
      pool.emplace_back(work, k);
    } catch (...) {  // no thread: this shard runs on the caller's thread below
      work(k);
    }
  }
  work(0);
  for (std::thread& t : pool) t.join();
  for (const Shard& sh : shards)
    if (sh.status) {
      rnamc::set_last_error(sh.error);
      return sh.status;
    }
  if (log_partition)
    for (const Shard& sh : shards)
      for (size_t x = 0; x < sh.members.size(); x++) log_partition[sh.members[x]] = sh.logz[x];
  return RNAMC_OK;
}

// rnamc_centroid_fold_batch over the pool: the shards of rnamc_bpp_batch_multi_constrained, each through
// its own context, rows, counts, accuracies, log partitions and triangles written straight into the
// caller's arrays.
int rnamc_centroid_fold_batch_multi(rnamc_pool* p, uint32_t n_seqs, const uint8_t* bases,
                                    const uint64_t* offsets, const char* constraints, uint32_t max_bp_span,
                                    int uses_contra_model, int allows_short_hairpins,
                                    const float* centroid_thresholds, uint32_t n_thresholds, uint8_t* structs,
                                    uint32_t* n_pairs, float* expect_accuracy, float* log_partition, float* bpp,
                                    const uint64_t* out_offsets) {
  if (!p) return RNAMC_ERR_INVALID_ARG;
  if (int rc = rnamc::centroid_fold_batch_check(n_seqs, bases, offsets, centroid_thresholds, n_thresholds,
                                                structs, bpp, out_offsets))
    return rc;
  if (p->ctxs.empty()) return RNAMC_ERR_INVALID_ARG;
  if (n_seqs == 0) return RNAMC_OK;
  if (constraints) {  // the whole batch before any device sees a part of it (the span limit needs no check)
    std::vector<int32_t> words;
    for (uint32_t s = 0; s < n_seqs; s++) {
      const uint32_t n = static_cast<uint32_t>(offsets[s + 1] - offsets[s]);
      uint32_t bad = 0;
      const char* why = "";
      int rc = RNAMC_OK;
      try {  // nothing may throw across the C boundary
        words.resize(2ull * n);
        rc = rnamc::compile_constraint(constraints + (offsets[s] - offsets[0]), n, words.data(), &bad, &why);
      } catch (const std::exception&) {
        rnamc::set_last_error("constraints: no host memory");
        return RNAMC_ERR_OOM;
      }
      if (rc) {
        rnamc::set_last_error("constraint of record " + std::to_string(s) + ", position " +
                              std::to_string(bad) + ": " + why);
        return rc;
      }
    }
  }
  std::lock_guard<std::mutex> lock(p->mu);
  const uint32_t n_shards = static_cast<uint32_t>(std::min<size_t>(p->ctxs.size(), n_seqs));
  std::vector<uint32_t> shard_of(n_seqs), order;
  plan(n_seqs, offsets, n_shards, shard_of.data(), &order);
  struct Shard {
    std::vector<uint32_t> members;  // batch indices, longest first
    std::vector<uint8_t> bases;
    std::vector<char> cons;
    std::vector<uint64_t> offsets, out_offsets, struct_offs;
    int status = RNAMC_OK;
    std::string error;
  };
  std::vector<Shard> shards(n_shards);
  for (uint32_t x = 0; x < n_seqs; x++) shards[shard_of[order[x]]].members.push_back(order[x]);
  for (Shard& sh : shards) {
    uint64_t total = 0;
    for (uint32_t s : sh.members) total += offsets[s + 1] - offsets[s];
    sh.bases.resize(total);
    if (constraints) sh.cons.resize(total);
    sh.offsets.assign(1, 0);
    for (uint32_t s : sh.members) {
      const uint64_t n = offsets[s + 1] - offsets[s];
      std::memcpy(sh.bases.data() + sh.offsets.back(), bases + offsets[s], n);
      if (constraints) std::memcpy(sh.cons.data() + sh.offsets.back(), constraints + (offsets[s] - offsets[0]), n);
      sh.offsets.push_back(sh.offsets.back() + n);
      sh.struct_offs.push_back(static_cast<uint64_t>(n_thresholds) * (offsets[s] - offsets[0]));
      if (bpp) sh.out_offsets.push_back(out_offsets[s]);
    }
  }
  auto work = [&](uint32_t k) {
    Shard& sh = shards[k];
    if (sh.members.empty()) return;
    // (the members themselves are the result indices: the shard writes the caller's arrays)
    sh.status = rnamc::centroid_fold_batch_core(
        p->ctxs[k], static_cast<uint32_t>(sh.members.size()), sh.bases.data(), sh.offsets.data(),
        constraints ? sh.cons.data() : nullptr, max_bp_span, uses_contra_model, allows_short_hairpins,
        centroid_thresholds, n_thresholds, structs, sh.struct_offs.data(), sh.members.data(), n_pairs,
        expect_accuracy, log_partition, bpp, bpp ? sh.out_offsets.data() : nullptr);
    if (sh.status) sh.error = rnamc_last_error();  // (thread-local: carry it to the caller's thread)
  };
  std::vector<std::thread> pool;
  for (uint32_t k = 1; k < n_shards; k++) {
    try {
      pool.emplace_back(work, k);
    } catch (...) {  // no thread: this shard runs on the caller's thread below
      work(k);
    }
  }
  work(0);
  for (std::thread& t : pool) t.join();
  for (const Shard& sh : shards)
    if (sh.status) {
      rnamc::set_last_error(sh.error);
      return sh.status;
    }
  return RNAMC_OK;
}

// rnamc_bpp_batch_sparse over the pool: the same shards, each through its own context; counts, starts,
// paired probabilities and log partitions go straight into the caller's arrays, and every group of
// every shard claims its part of the three list arrays from one cursor, so nothing is gathered.
int rnamc_bpp_batch_sparse_multi(rnamc_pool* p, uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
                                 const char* constraints, uint32_t max_bp_span, int uses_contra_model,
                                 int allows_short_hairpins, float min_prob, uint64_t* pair_start,
                                 uint64_t* pair_count, uint32_t* pair_i, uint32_t* pair_j, float* pair_prob,
                                 uint64_t pairs_cap, uint64_t* pairs_total, float* paired_prob,
                                 float* log_partition) {
  if (!p) return RNAMC_ERR_INVALID_ARG;
  if (int rc = rnamc::bpp_batch_sparse_check(n_seqs, bases, offsets, min_prob, pair_start, pair_count, pair_i,
                                             pair_j, pair_prob, pairs_total))
    return rc;
  *pairs_total = 0;
  // the whole batch before the pool is read or any device sees a part of it (the span limit needs no check)
  if (constraints && n_seqs) {
    std::vector<int32_t> words;
    for (uint32_t s = 0; s < n_seqs; s++) {
      const uint32_t n = static_cast<uint32_t>(offsets[s + 1] - offsets[s]);
      uint32_t bad = 0;
      const char* why = "";
      int rc = RNAMC_OK;
      try {  // nothing may throw across the C boundary
        words.resize(2ull * n);
        rc = rnamc::compile_constraint(constraints + (offsets[s] - offsets[0]), n, words.data(), &bad, &why);
      } catch (const std::exception&) {
        rnamc::set_last_error("constraints: no host memory");
        return RNAMC_ERR_OOM;
      }
      if (rc) {
        rnamc::set_last_error("constraint of record " + std::to_string(s) + ", position " +
                              std::to_string(bad) + ": " + why);
        return rc;
      }
    }
  }
  if (p->ctxs.empty()) return RNAMC_ERR_INVALID_ARG;
  if (n_seqs == 0) return RNAMC_OK;
  std::lock_guard<std::mutex> lock(p->mu);
  const uint32_t n_shards = static_cast<uint32_t>(std::min<size_t>(p->ctxs.size(), n_seqs));
  std::vector<uint32_t> shard_of(n_seqs), order;
  plan(n_seqs, offsets, n_shards, shard_of.data(), &order);
  struct Shard {
    std::vector<uint32_t> members;  // batch indices, longest first
    std::vector<uint8_t> bases;
    std::vector<char> cons;
    std::vector<uint64_t> offsets, pp_offs;
    int status = RNAMC_OK;
    std::string error;
  };
  std::vector<Shard> shards(n_shards);
  for (uint32_t x = 0; x < n_seqs; x++) shards[shard_of[order[x]]].members.push_back(order[x]);
  for (Shard& sh : shards) {
    uint64_t total = 0;
    for (uint32_t s : sh.members) total += offsets[s + 1] - offsets[s];
    sh.bases.resize(total);
    if (constraints) sh.cons.resize(total);
    sh.offsets.assign(1, 0);
    for (uint32_t s : sh.members) {
      const uint64_t n = offsets[s + 1] - offsets[s];
      std::memcpy(sh.bases.data() + sh.offsets.back(), bases + offsets[s], n);
      if (constraints) std::memcpy(sh.cons.data() + sh.offsets.back(), constraints + (offsets[s] - offsets[0]), n);
      sh.offsets.push_back(sh.offsets.back() + n);
      sh.pp_offs.push_back(offsets[s] - offsets[0]);
    }
  }
  std::atomic<uint64_t> cursor{0};
  auto work = [&](uint32_t k) {
    Shard& sh = shards[k];
    if (sh.members.empty()) return;
    // (the members themselves are the result indices: the shard writes the caller's arrays)
    sh.status = rnamc::bpp_batch_sparse_core(
        p->ctxs[k], static_cast<uint32_t>(sh.members.size()), sh.bases.data(), sh.offsets.data(),
        constraints ? sh.cons.data() : nullptr, max_bp_span, uses_contra_model, allows_short_hairpins, min_prob,
        sh.members.data(), sh.pp_offs.data(), pair_start, pair_count, pair_i, pair_j, pair_prob, pairs_cap,
        &cursor, paired_prob, log_partition);
    if (sh.status) sh.error = rnamc_last_error();  // (thread-local: carry it to the caller's thread)
  };
  std::vector<std::thread> pool;
  for (uint32_t k = 1; k < n_shards; k++) {
    try {
      pool.emplace_back(work, k);
    } catch (...) {  // no thread: this shard runs on the caller's thread below
      work(k);
    }
  }
  work(0);
  for (std::thread& t : pool) t.join();
  for (const Shard& sh : shards)
    if (sh.status) {
      rnamc::set_last_error(sh.error);
      return sh.status;
    }
  return rnamc::bpp_batch_sparse_finish(cursor.load(), pair_i != nullptr, pairs_cap, pairs_total);
}

// rnamc_context_profile_batch over the pool: the same shards, each through its own context; profiles
// and log partitions go straight into the caller's arrays.
int rnamc_context_profile_batch_multi(rnamc_pool* p, uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
                                      const char* constraints, uint32_t max_bp_span, int uses_contra_model,
                                      int allows_short_hairpins, float* profile, float* log_partition) {
  if (!p) return RNAMC_ERR_INVALID_ARG;
  if (int rc = rnamc::context_profile_check(n_seqs, bases, offsets, profile)) return rc;
  // the whole batch before the pool is read or any device sees a part of it (the span limit needs no check)
  if (constraints && n_seqs) {
    std::vector<int32_t> words;
    for (uint32_t s = 0; s < n_seqs; s++) {
      const uint32_t n = static_cast<uint32_t>(offsets[s + 1] - offsets[s]);
      uint32_t bad = 0;
      const char* why = "";
      int rc = RNAMC_OK;
      try {  // nothing may throw across the C boundary
        words.resize(2ull * n);
        rc = rnamc::compile_constraint(constraints + (offsets[s] - offsets[0]), n, words.data(), &bad, &why);
      } catch (const std::exception&) {
        rnamc::set_last_error("constraints: no host memory");
        return RNAMC_ERR_OOM;
      }
      if (rc) {
        rnamc::set_last_error("constraint of record " + std::to_string(s) + ", position " +
                              std::to_string(bad) + ": " + why);
        return rc;
      }
    }
  }
  if (p->ctxs.empty()) return RNAMC_ERR_INVALID_ARG;
  if (n_seqs == 0) return RNAMC_OK;
  std::lock_guard<std::mutex> lock(p->mu);
  const uint32_t n_shards = static_cast<uint32_t>(std::min<size_t>(p->ctxs.size(), n_seqs));
  std::vector<uint32_t> shard_of(n_seqs), order;
  plan(n_seqs, offsets, n_shards, shard_of.data(), &order);
  struct Shard {
    std::vector<uint32_t> members;  // batch indices, longest first
    std::vector<uint8_t> bases;
    std::vector<char> cons;
    std::vector<uint64_t> offsets, prof_offs;
    int status = RNAMC_OK;
    std::string error;
  };
  std::vector<Shard> shards(n_shards);
  for (uint32_t x = 0; x < n_seqs; x++) shards[shard_of[order[x]]].members.push_back(order[x]);
  for (Shard& sh : shards) {
    uint64_t total = 0;
    for (uint32_t s : sh.members) total += offsets[s + 1] - offsets[s];
    sh.bases.resize(total);
    if (constraints) sh.cons.resize(total);
    sh.offsets.assign(1, 0);
    for (uint32_t s : sh.members) {
      const uint64_t n = offsets[s + 1] - offsets[s];
      std::memcpy(sh.bases.data() + sh.offsets.back(), bases + offsets[s], n);
      if (constraints) std::memcpy(sh.cons.data() + sh.offsets.back(), constraints + (offsets[s] - offsets[0]), n);
      sh.offsets.push_back(sh.offsets.back() + n);
      sh.prof_offs.push_back(6ull * (offsets[s] - offsets[0]));
    }
  }
  auto work = [&](uint32_t k) {
    Shard& sh = shards[k];
    if (sh.members.empty()) return;
    // (the members themselves are the result indices: the shard writes the caller's arrays)
    sh.status = rnamc::context_profile_core(
        p->ctxs[k], static_cast<uint32_t>(sh.members.size()), sh.bases.data(), sh.offsets.data(),
        constraints ? sh.cons.data() : nullptr, max_bp_span, uses_contra_model, allows_short_hairpins,
        sh.members.data(), sh.prof_offs.data(), profile, log_partition);
    if (sh.status) sh.error = rnamc_last_error();  // (thread-local: carry it to the caller's thread)
  };
  std::vector<std::thread> pool;
  for (uint32_t k = 1; k < n_shards; k++) {
    try {
      pool.emplace_back(work, k);
    } catch (...) {  // no thread: this shard runs on the caller's thread below
      work(k);
    }
  }
  work(0);
  for (std::thread& t : pool) t.join();
  for (const Shard& sh : shards)
    if (sh.status) {
      rnamc::set_last_error(sh.error);
      return sh.status;
    }
  return RNAMC_OK;
}

// rnamc_bpp_windowed over the pool: the window list cut into shards (equal windows: contiguous bands of
// equal size), each context accumulating its shard into its own integer sums and counters; these are added
// on the host — integer adds, any order — and the pool's first context finalises the totals: the bits of
// the single-context entry.
int rnamc_bpp_windowed_multi(rnamc_pool* p, const uint8_t* bases, uint64_t n, const char* constraint,
                             uint32_t window, uint32_t stride, uint32_t max_bp_span, int uses_contra_model,
                             int allows_short_hairpins, float* band_prob, float* paired_prob,
                             float* window_log_partition) {
  if (!p) return RNAMC_ERR_INVALID_ARG;
  rnamc::WindowPlan wp;
  if (int rc = rnamc::bpp_windowed_check(bases, n, constraint, window, stride, max_bp_span, band_prob, &wp))
    return rc;
  if (p->ctxs.empty()) return RNAMC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(p->mu);
  const uint32_t n_shards = static_cast<uint32_t>(std::min<uint64_t>(p->ctxs.size(), wp.n_windows));
  const uint64_t cells = static_cast<uint64_t>(wp.band) * wp.n;
  struct Shard {
    uint64_t first = 0, count = 0;
    std::vector<int64_t> sum;
    std::vector<uint32_t> cnt;
    int status = RNAMC_OK;
    std::string error;
  };
  std::vector<Shard> shards(n_shards);
  try {  // nothing may throw across the C boundary
    // the plan of rnamc_shard_plan over the windows as records of w bases (the list's order is kept)
    const uint32_t nw = static_cast<uint32_t>(wp.n_windows);  // (n < 2^31: it fits)
    std::vector<uint64_t> offs(static_cast<size_t>(nw) + 1);
    for (uint64_t x = 0; x <= nw; x++) offs[x] = x * wp.w;
    std::vector<uint32_t> shard_of(nw);
    plan(nw, offs.data(), n_shards, shard_of.data(), nullptr);
    for (uint32_t x = 0; x < nw; x++) {
      Shard& sh = shards[shard_of[x]];
      if (sh.count == 0) sh.first = x;
      sh.count++;
    }
    if (n_shards > 1)
      for (Shard& sh : shards) {
        sh.sum.resize(cells);
        sh.cnt.resize(cells);
      }
  } catch (const std::exception&) {
    rnamc::set_last_error("rnamc_bpp_windowed_multi: no host memory");
    return RNAMC_ERR_OOM;
  }
  auto work = [&](uint32_t k) {
    Shard& sh = shards[k];
    rnamc_ctx* c = p->ctxs[k];
    std::unique_lock<std::mutex> ctx_lock(c->mu);
    rnamc::DeviceGuard guard(c->device);
    if (!guard.ok) {
      sh.status = RNAMC_ERR_NO_DEVICE;
      return;
    }
    sh.status = rnamc::bpp_windowed_accumulate(c, wp, bases, constraint, sh.first, sh.count, uses_contra_model,
                                               allows_short_hairpins, window_log_partition);
    if (sh.status == RNAMC_OK && n_shards > 1)
      sh.status = rnamc::bpp_windowed_fetch(c, wp, sh.sum.data(), sh.cnt.data());
    if (sh.status) {
      sh.error = rnamc_last_error();  // (thread-local: carry it to the caller's thread)
      (void)hipStreamSynchronize(c->own_stream);
    }
  };
  std::vector<std::thread> pool;
  for (uint32_t k = 1; k < n_shards; k++) {
    try {
      pool.emplace_back(work, k);
    } catch (...) {  // no thread: this shard runs on the caller's thread below
      work(k);
    }
  }
  work(0);
  for (std::thread& t : pool) t.join();
  for (const Shard& sh : shards)
    if (sh.status) {
      rnamc::set_last_error(sh.error);
      return sh.status;
    }
  for (uint32_t k = 1; k < n_shards; k++)
    for (uint64_t x = 0; x < cells; x++) {
      shards[0].sum[x] += shards[k].sum[x];
      shards[0].cnt[x] += shards[k].cnt[x];
    }
  rnamc_ctx* c = p->ctxs[0];
  std::unique_lock<std::mutex> ctx_lock(c->mu);
  rnamc::DeviceGuard guard(c->device);
  if (!guard.ok) return RNAMC_ERR_NO_DEVICE;
  return rnamc::bpp_windowed_finish(c, wp, n_shards > 1 ? shards[0].sum.data() : nullptr,
                                    n_shards > 1 ? shards[0].cnt.data() : nullptr, band_prob, paired_prob);
}

// rnamc_bpp_alignment over the pool: the rows cut into shards by the plan of rnamc_shard_plan over their
// ungapped lengths, each context accumulating its shard into its own integer sums and counters; these
// are added on the host — integer adds, any order — and the pool's first context averages the totals
// and folds them: the bits of the single-context entry.
int rnamc_bpp_alignment_multi(rnamc_pool* p, uint32_t n_rows, uint32_t n_cols, const uint8_t* rows,
                              uint32_t max_bp_span, int uses_contra_model, int allows_short_hairpins,
                              const float* centroid_thresholds, uint32_t n_thresholds, float* bpp,
                              float* col_paired, uint8_t* structs, uint32_t* n_pairs, float* expect_accuracy,
                              float* log_partition, uint32_t* row_len) {
  if (!p) return RNAMC_ERR_INVALID_ARG;
  rnamc::AlignRows all;
  if (int rc = rnamc::bpp_alignment_check(n_rows, n_cols, rows, centroid_thresholds, n_thresholds, structs,
                                          n_pairs, expect_accuracy, &all))
    return rc;
  if (p->ctxs.empty()) return RNAMC_ERR_INVALID_ARG;
  if (row_len)
    for (uint32_t s = 0; s < n_rows; s++) row_len[s] = static_cast<uint32_t>(all.offsets[s + 1] - all.offsets[s]);
  std::lock_guard<std::mutex> lock(p->mu);
  const uint32_t n_shards = static_cast<uint32_t>(std::min<size_t>(p->ctxs.size(), n_rows));
  const uint64_t cells = rnamc_bpp_len(n_cols);
  struct Shard {
    rnamc::AlignRows rows;
    std::vector<int64_t> sum;
    std::vector<uint32_t> cnt;
    int status = RNAMC_OK;
    std::string error;
  };
  std::vector<Shard> shards(n_shards);
  try {  // nothing may throw across the C boundary
    if (n_shards > 1) {
      std::vector<uint32_t> shard_of(n_rows), order;
      plan(n_rows, all.offsets.data(), n_shards, shard_of.data(), &order);
      for (Shard& sh : shards) {
        sh.rows.n_cols = n_cols;
        sh.rows.offsets.assign(1, 0);
        sh.sum.resize(cells);
        sh.cnt.resize(cells);
      }
      for (uint32_t x = 0; x < n_rows; x++) {  // longest first inside every shard
        const uint32_t s = order[x];
        rnamc::AlignRows& r = shards[shard_of[s]].rows;
        r.bases.insert(r.bases.end(), all.bases.begin() + all.offsets[s], all.bases.begin() + all.offsets[s + 1]);
        r.maps.insert(r.maps.end(), all.maps.begin() + all.offsets[s], all.maps.begin() + all.offsets[s + 1]);
        r.offsets.push_back(r.bases.size());
        r.row_idx.push_back(s);
      }
    }
  } catch (const std::exception&) {
    rnamc::set_last_error("rnamc_bpp_alignment_multi: no host memory");
    return RNAMC_ERR_OOM;
  }
  auto work = [&](uint32_t k) {
    Shard& sh = shards[k];
    rnamc_ctx* c = p->ctxs[k];
    std::unique_lock<std::mutex> ctx_lock(c->mu);
    rnamc::DeviceGuard guard(c->device);
    if (!guard.ok) {
      sh.status = RNAMC_ERR_NO_DEVICE;
      return;
    }
    sh.status = rnamc::bpp_alignment_accumulate(c, n_shards > 1 ? sh.rows : all, max_bp_span, uses_contra_model,
                                                allows_short_hairpins, log_partition);
    if (sh.status == RNAMC_OK && n_shards > 1)
      sh.status = rnamc::bpp_alignment_fetch(c, n_cols, sh.sum.data(), sh.cnt.data());
    if (sh.status) {
      sh.error = rnamc_last_error();  // (thread-local: carry it to the caller's thread)
      (void)hipStreamSynchronize(c->own_stream);
    }
  };
  std::vector<std::thread> pool;
  for (uint32_t k = 1; k < n_shards; k++) {
    try {
      pool.emplace_back(work, k);
    } catch (...) {  // no thread: this shard runs on the caller's thread below
      work(k);
    }
  }
  work(0);
  for (std::thread& t : pool) t.join();
  for (const Shard& sh : shards)
    if (sh.status) {
      rnamc::set_last_error(sh.error);
      return sh.status;
    }
  for (uint32_t k = 1; k < n_shards; k++)
    for (uint64_t x = 0; x < cells; x++) {
      shards[0].sum[x] += shards[k].sum[x];
      shards[0].cnt[x] += shards[k].cnt[x];
    }
  rnamc_ctx* c = p->ctxs[0];
  std::unique_lock<std::mutex> ctx_lock(c->mu);
  rnamc::DeviceGuard guard(c->device);
  if (!guard.ok) return RNAMC_ERR_NO_DEVICE;
  return rnamc::bpp_alignment_finish(c, n_rows, n_cols, n_shards > 1 ? shards[0].sum.data() : nullptr,
                                     n_shards > 1 ? shards[0].cnt.data() : nullptr, centroid_thresholds,
                                     n_thresholds, bpp, col_paired, structs, n_pairs, expect_accuracy);
}

// rnamc_mutant_scan over the pool: the mutant list cut into shards (equal records: contiguous bands of
// equal size); every context folds the wild type itself and scans its shard straight into the caller's
// arrays.  Per-mutant integers, nothing summed across devices: the bits of the single-context entry.
int rnamc_mutant_scan_multi(rnamc_pool* p, const uint8_t* bases, uint32_t n, const char* constraint,
                            uint32_t max_bp_span, int uses_contra_model, int allows_short_hairpins,
                            const uint32_t* positions, uint32_t n_positions, float* log_partition,
                            int64_t* pair_dist2_q, float* max_dp, uint32_t* max_i, uint32_t* max_j,
                            float* paired_prob, float* wt_log_partition, float* wt_paired_prob) {
  if (!p) return RNAMC_ERR_INVALID_ARG;
  uint64_t total = 0;
  if (int rc = rnamc::mutant_scan_check(bases, n, constraint, positions, n_positions, log_partition, &total))
    return rc;
  if (p->ctxs.empty()) return RNAMC_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lock(p->mu);
  const uint32_t nm = static_cast<uint32_t>(total);  // (below 2^32: checked)
  const uint32_t n_shards = static_cast<uint32_t>(std::min<uint64_t>(p->ctxs.size(), std::max(nm, 1u)));
  struct Shard {
    uint64_t first = 0, count = 0;
    int status = RNAMC_OK;
    std::string error;
  };
  std::vector<Shard> shards(n_shards);
  try {  // nothing may throw across the C boundary
    // the plan of rnamc_shard_plan over the mutants as records of n bases (the list's order is kept)
    std::vector<uint64_t> offs(static_cast<size_t>(nm) + 1);
    for (uint64_t x = 0; x <= nm; x++) offs[x] = x * n;
    std::vector<uint32_t> shard_of(nm);
    if (nm) plan(nm, offs.data(), n_shards, shard_of.data(), nullptr);
    for (uint32_t x = 0; x < nm; x++) {
      Shard& sh = shards[shard_of[x]];
      if (sh.count == 0) sh.first = x;
      sh.count++;
    }
  } catch (const std::exception&) {
    rnamc::set_last_error("rnamc_mutant_scan_multi: no host memory");
    return RNAMC_ERR_OOM;
  }
  auto work = [&](uint32_t k) {
    Shard& sh = shards[k];
    if (k != 0 && sh.count == 0) return;
    rnamc_ctx* c = p->ctxs[k];
    std::unique_lock<std::mutex> ctx_lock(c->mu);
    rnamc::DeviceGuard guard(c->device);
    if (!guard.ok) {
      sh.status = RNAMC_ERR_NO_DEVICE;
      return;
    }
    // (the wild type's outputs come from the first shard alone: every context computes the same bits)
    sh.status = rnamc::mutant_scan_core(c, bases, n, constraint, max_bp_span, uses_contra_model,
                                        allows_short_hairpins, positions, sh.first, sh.count, log_partition,
                                        pair_dist2_q, max_dp, max_i, max_j, paired_prob,
                                        k == 0 ? wt_log_partition : nullptr, k == 0 ? wt_paired_prob : nullptr);
    if (sh.status) {
      sh.error = rnamc_last_error();  // (thread-local: carry it to the caller's thread)
      (void)hipStreamSynchronize(c->own_stream);
    }
  };
  std::vector<std::thread> pool;
  for (uint32_t k = 1; k < n_shards; k++) {
    try {
      pool.emplace_back(work, k);
    } catch (...) {  // no thread: this shard runs on the caller's thread below
      work(k);
    }
  }
  work(0);
  for (std::thread& t : pool) t.join();
  for (const Shard& sh : shards)
    if (sh.status) {
      rnamc::set_last_error(sh.error);
      return sh.status;
    }
  return RNAMC_OK;
}

}  // extern "C"
