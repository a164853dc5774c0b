// rnamc_shards.h — what the pool entries (rnamc_pool.cpp) share, on the host alone: the cost model and
// the shard plan, the validation of a batch's constraint strings, the shards of a batch of records
// and of a list of equal records, the threads that run them, and the sum of their integer
// accumulators.  Nothing here touches a device: rnamc_internal.h and the standard library.
#ifndef RNAMC_SHARDS_H
#define RNAMC_SHARDS_H

#include <algorithm>
#include <cstring>
#include <functional>
#include <numeric>
#include <thread>

#include "rnamc_internal.h"

namespace rnamc {

inline double sweep_cost(uint64_t n) {
  const double x = static_cast<double>(n);
  return RNAMC_COST_S_PER_CELL_K * (x * (x * x - 1.0) / 6.0) + RNAMC_COST_S_PER_N2 * x * x;
}

// shard of every sequence: bands of the cost-sorted order (longest first, stable) with equal
// total cost; cut k lies at the first position whose running cost reaches k / n_shards of the
// total (the position itself goes to the next band, as numpy.searchsorted(side="left") cuts)
inline void plan(uint32_t n_seqs, const uint64_t* offsets, uint32_t n_shards, uint32_t* shard_of_seq,
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

inline int no_host_memory(const char* who) {
  set_last_error(std::string(who) + ": no host memory");
  return RNAMC_ERR_OOM;
}

// The constraint strings of a batch (laid out like its bases) compiled record by record: into
// words + 2 * (offsets[s] - offsets[0]) for a caller that keeps them (ConsCall, rnamc_entries.h),
// into scratch with words == NULL.  The first bad record fails the call, named in rnamc_last_error.
inline int compile_constraints(uint32_t n_seqs, const uint64_t* offsets, const char* strings, int32_t* words) {
  std::vector<int32_t> scratch;
  for (uint32_t s = 0; s < n_seqs; s++) {
    const uint64_t off = offsets[s] - offsets[0];
    const uint32_t n = static_cast<uint32_t>(offsets[s + 1] - offsets[s]);
    uint32_t bad = 0;
    const char* why = "";
    int rc = RNAMC_OK;
    try {  // nothing may throw across the C boundary
      if (!words) scratch.resize(2ull * n);
      rc = compile_constraint(strings + off, n, words ? words + 2 * off : scratch.data(), &bad, &why);
    } catch (const std::exception&) {
      return no_host_memory("constraints");
    }
    if (rc) {
      set_last_error("constraint of record " + std::to_string(s) + ", position " + std::to_string(bad) + ": " +
                     why);
      return rc;
    }
  }
  return RNAMC_OK;
}

// A pool entry validates the whole batch before any device sees a part of it: one bad record fails
// the call with its status and nothing is computed (the span limit needs no check).
inline int check_constraints(uint32_t n_seqs, const uint64_t* offsets, const char* strings) {
  return strings ? compile_constraints(n_seqs, offsets, strings, nullptr) : RNAMC_OK;
}

// A batch of records cut into the shards of `plan`, at most one per record, none empty.  A shard is
// a batch of its own (bases, constraint bytes and offsets gathered, longest record first) that also
// knows where its records lie in the caller's: place() hands both to a core, which then writes the
// caller's arrays.
struct RecordShards {
  struct Shard {
    std::vector<uint32_t> members;  // the caller's indices, longest first
    std::vector<uint8_t> bases;
    std::vector<char> cons;  // the members' constraint strings (when the call has them)
    std::vector<uint64_t> offsets, base_off;  // of the gathered bases; of member x in the caller's
    std::vector<uint64_t> out_offsets;  // the members' entries of the caller's (a call that has them)
    uint32_t count() const { return static_cast<uint32_t>(members.size()); }
    const char* constraints() const { return cons.empty() ? nullptr : cons.data(); }
    Place place() const { return Place{members.data(), base_off.data()}; }
  };
  std::vector<Shard> shards;

  int build(const char* who, uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
            const char* constraints, uint32_t n_shards, const uint64_t* out_offsets = nullptr) {
    try {  // nothing may throw across the C boundary
      n_shards = std::min(n_shards, std::max(n_seqs, 1u));
      std::vector<uint32_t> shard_of(n_seqs), order;
      plan(n_seqs, offsets, n_shards, shard_of.data(), &order);
      shards.assign(n_shards, Shard());
      for (uint32_t x = 0; x < n_seqs; x++) shards[shard_of[order[x]]].members.push_back(order[x]);
      for (Shard& sh : shards) {
        uint64_t total = 0;
        for (uint32_t s : sh.members) total += offsets[s + 1] - offsets[s];
        sh.bases.resize(total);
        if (constraints) sh.cons.resize(total);
        sh.offsets.assign(1, 0);
        for (uint32_t s : sh.members) {
          const uint64_t n = offsets[s + 1] - offsets[s], at = sh.offsets.back();
          sh.base_off.push_back(offsets[s] - offsets[0]);
          std::memcpy(sh.bases.data() + at, bases + offsets[s], n);
          if (constraints) std::memcpy(sh.cons.data() + at, constraints + sh.base_off.back(), n);
          sh.offsets.push_back(at + n);
          if (out_offsets) sh.out_offsets.push_back(out_offsets[s]);
        }
        sh.out_offsets.push_back(0);  // (entry n of the prefix form: unused by rnamc_bpp_batch)
      }
    } catch (const std::exception&) {
      return no_host_memory(who);
    }
    return RNAMC_OK;
  }
};

// A list of `count` equal records cut into shards: the plan over records of rec_len bases, which
// keeps the list's order, so shard k is the contiguous band [first, first + count).  At most one
// shard per record, and one (empty) for an empty list.
struct ListBand {
  uint64_t first = 0, count = 0;
};
inline int list_shards(const char* who, uint32_t count, uint64_t rec_len, uint32_t n_shards,
                       std::vector<ListBand>* bands) {
  try {  // nothing may throw across the C boundary
    bands->assign(std::min(n_shards, std::max(count, 1u)), ListBand());
    std::vector<uint64_t> offs(static_cast<size_t>(count) + 1);
    for (uint64_t x = 0; x <= count; x++) offs[x] = x * rec_len;
    std::vector<uint32_t> shard_of(count);
    plan(count, offs.data(), static_cast<uint32_t>(bands->size()), shard_of.data(), nullptr);
    for (uint32_t x = 0; x < count; x++) {
      ListBand& b = (*bands)[shard_of[x]];
      if (b.count == 0) b.first = x;
      b.count++;
    }
  } catch (const std::exception&) {
    return no_host_memory(who);
  }
  return RNAMC_OK;
}

// work(k) for every shard: shards 1.. on threads of their own, shard 0 (and any shard no thread
// could be made for) on the caller's.  The first failing shard's status is the call's, and its
// rnamc_last_error — thread-local, read on the shard's thread — becomes the caller's.
inline int run_shards(const char* who, uint32_t n_shards, const std::function<int(uint32_t)>& work) {
  std::vector<int> status;
  std::vector<std::string> error;
  try {  // nothing may throw across the C boundary
    status.assign(n_shards, RNAMC_OK);
    error.resize(n_shards);
  } catch (const std::exception&) {
    return no_host_memory(who);
  }
  auto run = [&](uint32_t k) {
    status[k] = work(k);
    if (status[k]) error[k] = rnamc_last_error();
  };
  std::vector<std::thread> threads;
  for (uint32_t k = 1; k < n_shards; k++) {
    try {
      threads.emplace_back(run, k);
    } catch (...) {  // no thread: this shard runs on the caller's thread
      run(k);
    }
  }
  if (n_shards) run(0);
  for (std::thread& t : threads) t.join();
  for (uint32_t k = 0; k < n_shards; k++)
    if (status[k]) {
      set_last_error(error[k]);
      return status[k];
    }
  return RNAMC_OK;
}

// The integer accumulators of the shards of an averaging entry on the host: every shard's context
// fetches its own into sum_of(k) / cnt_of(k), reduce() adds them into shard 0's — integer adds, any
// order — and the pool's first context finishes from total_sum() / total_cnt().  One shard holds
// nothing (every pointer NULL): its context finishes from its own accumulators.
struct ShardSums {
  std::vector<std::vector<int64_t>> sum;
  std::vector<std::vector<uint32_t>> cnt;

  int init(const char* who, uint32_t n_shards, uint64_t cells) {
    if (n_shards < 2) return RNAMC_OK;
    try {  // nothing may throw across the C boundary
      sum.resize(n_shards);
      cnt.resize(n_shards);
      for (uint32_t k = 0; k < n_shards; k++) {
        sum[k].resize(cells);
        cnt[k].resize(cells);
      }
    } catch (const std::exception&) {
      return no_host_memory(who);
    }
    return RNAMC_OK;
  }
  int64_t* sum_of(uint32_t k) { return sum.empty() ? nullptr : sum[k].data(); }
  uint32_t* cnt_of(uint32_t k) { return cnt.empty() ? nullptr : cnt[k].data(); }
  void reduce() {
    for (size_t k = 1; k < sum.size(); k++)
      for (size_t x = 0; x < sum[0].size(); x++) {
        sum[0][x] += sum[k][x];
        cnt[0][x] += cnt[k][x];
      }
  }
  const int64_t* total_sum() { return sum_of(0); }
  const uint32_t* total_cnt() { return cnt_of(0); }
};

}  // namespace rnamc

#endif
