// shards_host_check.cpp — the host-only pieces behind the pool entries (rna_algos_amd/csrc/rnamc_shards.h)
// driven without a device: RecordShards against a direct recomputation from the plan's assignment,
// run_shards' first-failure rule, and the message of check_constraints.  Built with the address and
// undefined-behaviour sanitizers and run as a plain program by tests/test_shards_cpu.py; every plan it
// used goes to stdout ("plan <n_shards> <lengths> <shard of every record>") for the test to hold
// against rnamc_shard_plan.
#include <atomic>
#include <cstdio>
#include <string>

#include "../rna_algos_amd/csrc/rnamc_shards.h"

using namespace rnamc;

static int g_fails = 0;
#define CHECK(cond)                                                  \
  do {                                                               \
    if (!(cond)) {                                                   \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
      g_fails++;                                                     \
    }                                                                \
  } while (0)

static uint64_t g_lcg = 20240607u;
static uint32_t lcg() {
  g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
  return static_cast<uint32_t>(g_lcg >> 33);
}

static void check_record_shards(uint32_t n, uint32_t n_shards, bool with_cons) {
  // records of 1 .. 64 bases behind 5 bytes that belong to nobody (offsets[0] != 0), the last as long
  // as the first (a tie whatever the generator gives)
  std::vector<uint64_t> offsets(n + 1, 5), out_offsets(n);
  for (uint32_t s = 0; s < n; s++) offsets[s + 1] = offsets[s] + 1 + lcg() % 64;
  if (n >= 2) offsets[n] = offsets[n - 1] + (offsets[1] - offsets[0]);
  const uint64_t total = offsets[n] - offsets[0];
  std::vector<uint8_t> bases(offsets[n]);
  std::vector<char> cons(total);
  for (uint8_t& b : bases) b = static_cast<uint8_t>(lcg() % 4);
  for (char& ch : cons) ch = ".x()<>"[lcg() % 6];  // (gathered, not compiled: any bytes)
  for (uint32_t s = 0; s < n; s++) out_offsets[s] = 1000 + 7ull * s;

  RecordShards rs;
  CHECK(rs.build("check", n, bases.data(), offsets.data(), with_cons ? cons.data() : nullptr, n_shards,
                 with_cons ? out_offsets.data() : nullptr) == RNAMC_OK);
  const uint32_t want_shards = std::min(n_shards, std::max(n, 1u));
  CHECK(rs.shards.size() == want_shards);
  if (rs.shards.size() != want_shards) return;

  std::vector<uint32_t> shard_of(n);
  plan(n, offsets.data(), n_shards, shard_of.data(), nullptr);
  std::printf(n ? "plan %u" : "plan %u - -", n_shards);
  for (uint32_t s = 0; s < n; s++) std::printf("%c%llu", s ? ',' : ' ', (unsigned long long)(offsets[s + 1] - offsets[s]));
  for (uint32_t s = 0; s < n; s++) std::printf("%c%u", s ? ',' : ' ', shard_of[s]);
  std::printf("\n");

  for (uint32_t k = 0; k < want_shards; k++) {
    // the records with shard_of == k, longest first, ties in the batch's order
    std::vector<uint32_t> members;
    for (uint32_t s = 0; s < n; s++)
      if (shard_of[s] == k) members.push_back(s);
    std::stable_sort(members.begin(), members.end(), [&](uint32_t a, uint32_t b) {
      return offsets[a + 1] - offsets[a] > offsets[b + 1] - offsets[b];
    });
    std::vector<uint8_t> want_bases;
    std::vector<char> want_cons;
    std::vector<uint64_t> want_offsets(1, 0), want_base_off, want_out;
    for (uint32_t s : members) {
      want_bases.insert(want_bases.end(), bases.begin() + offsets[s], bases.begin() + offsets[s + 1]);
      if (with_cons)
        want_cons.insert(want_cons.end(), cons.begin() + (offsets[s] - offsets[0]),
                         cons.begin() + (offsets[s + 1] - offsets[0]));
      want_offsets.push_back(want_bases.size());
      want_base_off.push_back(offsets[s] - offsets[0]);
      if (with_cons) want_out.push_back(out_offsets[s]);
    }
    want_out.push_back(0);
    const RecordShards::Shard& sh = rs.shards[k];
    CHECK(n == 0 || !sh.members.empty());  // the entries hand every shard to a context as it is
    CHECK(sh.members == members);
    CHECK(sh.count() == members.size());
    CHECK(sh.bases == want_bases);
    CHECK(sh.cons == want_cons);
    CHECK((sh.constraints() != nullptr) == (with_cons && !members.empty()));
    CHECK(sh.offsets == want_offsets);
    CHECK(sh.base_off == want_base_off);
    CHECK(sh.out_offsets == want_out);
    const Place pl = sh.place();
    for (uint32_t x = 0; x < sh.count(); x++) {
      CHECK(pl.idx(x) == members[x]);
      CHECK(pl.base(x, sh.offsets.data()) == want_base_off[x]);
    }
  }
  // the identity placement of a context entry
  const Place id;
  for (uint32_t s = 0; s < n; s++) CHECK(id.idx(s) == s && id.base(s, offsets.data()) == offsets[s] - offsets[0]);
}

static void check_list_shards() {
  for (uint32_t n_shards : {1u, 2u, 3u, 8u})
    for (uint32_t count : {0u, 1u, 2u, 7u, 33u}) {
      std::vector<ListBand> bands;
      CHECK(list_shards("check", count, 24, n_shards, &bands) == RNAMC_OK);
      CHECK(bands.size() == std::min(n_shards, std::max(count, 1u)));
      std::vector<uint64_t> offs(count + 1);
      for (uint32_t x = 0; x <= count; x++) offs[x] = 24ull * x;
      std::vector<uint32_t> shard_of(count);
      plan(count, offs.data(), n_shards, shard_of.data(), nullptr);
      uint64_t next = 0;
      for (uint32_t k = 0; k < bands.size(); k++) {
        CHECK(count == 0 || bands[k].count > 0);
        if (bands[k].count) CHECK(bands[k].first == next);
        for (uint64_t x = bands[k].first; x < bands[k].first + bands[k].count; x++) CHECK(shard_of[x] == k);
        next += bands[k].count;
      }
      CHECK(next == count);
    }
}

static void check_run_shards() {
  set_last_error("stale");
  std::atomic<uint32_t> ran{0};
  const std::thread::id caller = std::this_thread::get_id();
  bool zero_on_caller = false;
  const int rc = run_shards("check", 4, [&](uint32_t k) -> int {
    ran |= 1u << k;
    if (k == 0) zero_on_caller = std::this_thread::get_id() == caller;
    if (k < 2) return RNAMC_OK;
    set_last_error("shard " + std::to_string(k) + " failed");
    return k == 2 ? RNAMC_ERR_INVALID_BASE : RNAMC_ERR_HIP;
  });
  CHECK(ran == 15u);
  CHECK(zero_on_caller);
  CHECK(rc == RNAMC_ERR_INVALID_BASE);
  CHECK(std::string(rnamc_last_error()) == "shard 2 failed");
  CHECK(run_shards("check", 3, [](uint32_t) { return RNAMC_OK; }) == RNAMC_OK);
  // the first shard fails too: its status and text win
  CHECK(run_shards("check", 3, [](uint32_t k) -> int {
          set_last_error("shard " + std::to_string(k));
          return k ? RNAMC_ERR_HIP : RNAMC_ERR_EMPTY_SEQ;
        }) == RNAMC_ERR_EMPTY_SEQ);
  CHECK(std::string(rnamc_last_error()) == "shard 0");
}

static void check_shard_sums() {
  ShardSums one, three;
  CHECK(one.init("check", 1, 10) == RNAMC_OK);
  CHECK(one.sum_of(0) == nullptr && one.cnt_of(0) == nullptr && one.total_sum() == nullptr);
  one.reduce();
  CHECK(three.init("check", 3, 10) == RNAMC_OK);
  for (uint32_t k = 0; k < 3; k++)
    for (uint32_t x = 0; x < 10; x++) {
      three.sum_of(k)[x] = -1000 * static_cast<int64_t>(k + 1) + x;
      three.cnt_of(k)[x] = 10 * k + x;
    }
  three.reduce();
  for (uint32_t x = 0; x < 10; x++) {
    CHECK(three.total_sum()[x] == -6000 + 3 * static_cast<int64_t>(x));
    CHECK(three.total_cnt()[x] == 30 + 3 * x);
  }
}

static void check_check_constraints() {
  const uint64_t offsets[5] = {3, 9, 13, 21, 25};  // (constraint strings are laid out from offsets[0])
  const std::string good = std::string("(....)") + "<>.x" + ".((..))." + "....";
  const std::string bad = std::string("(....)") + "<>.x" + ".(.((..)" + "....";
  CHECK(check_constraints(4, offsets, nullptr) == RNAMC_OK);
  CHECK(check_constraints(4, offsets, good.c_str()) == RNAMC_OK);
  set_last_error("");
  CHECK(check_constraints(4, offsets, bad.c_str()) == RNAMC_ERR_INVALID_ARG);
  CHECK(std::string(rnamc_last_error()) == "constraint of record 2, position 3: '(' without a matching ')'");
  // compiled into the caller's words, the same loop reports the same record
  std::vector<int32_t> words(2 * 22, -1);
  CHECK(compile_constraints(4, offsets, good.c_str(), words.data()) == RNAMC_OK);
  CHECK(words[2 * 0] == 5 && words[2 * 5] == 0);  // the pair of record 0
  set_last_error("");
  CHECK(compile_constraints(4, offsets, bad.c_str(), words.data()) == RNAMC_ERR_INVALID_ARG);
  CHECK(std::string(rnamc_last_error()) == "constraint of record 2, position 3: '(' without a matching ')'");
}

int main() {
  for (uint32_t n_shards : {1u, 2u, 3u, 8u})
    for (uint32_t n : {0u, 1u, 2u, 7u, 33u})
      for (bool with_cons : {false, true}) check_record_shards(n, n_shards, with_cons);
  check_list_shards();
  check_run_shards();
  check_shard_sums();
  check_check_constraints();
  std::printf(g_fails ? "FAILED %d\n" : "OK\n", g_fails);
  return g_fails ? 1 : 0;
}
