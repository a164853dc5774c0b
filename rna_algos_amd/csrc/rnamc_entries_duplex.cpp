// rnamc_entries_duplex.cpp — rnamc_duplex_batch and rnamc_duplex_score (include/rnamc.h, DESIGN.md
// section 19): a list of strand pairs cut into chunks that fit "group_ws_bytes", every chunk swept
// line by line (rnamc_duplex.hip), one copy per chunk back to the host; and the host scorer of one
// duplex.
#include <unordered_map>

#include "rnamc_entries.h"

using namespace rnamc;

namespace rnamc {

int duplex_batch_check(uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets, uint32_t n_pairs,
                       const uint32_t* pair_a, const uint32_t* pair_b, const float* match_probs,
                       const uint64_t* out_offsets, const float* bound_a, const float* bound_b,
                       const uint64_t* bound_offsets, const uint8_t* structs, const uint64_t* struct_offsets) {
  if (!offsets || (n_seqs && !bases) || (n_pairs && (!pair_a || !pair_b))) return RNAMC_ERR_INVALID_ARG;
  if ((match_probs && !out_offsets) || ((bound_a || bound_b) && !bound_offsets) || (structs && !struct_offsets))
    return RNAMC_ERR_INVALID_ARG;
  if (int rc = check_records(n_seqs, bases, offsets)) return rc;
  for (uint32_t p = 0; p < n_pairs; p++)
    if (pair_a[p] >= n_seqs || pair_b[p] >= n_seqs) {
      set_last_error("rnamc_duplex_batch: pair " + std::to_string(p) + " names a record past the end");
      return RNAMC_ERR_INVALID_ARG;
    }
  return RNAMC_OK;
}

int duplex_batch_core(rnamc_ctx* c, const uint8_t* bases, const uint64_t* offsets, uint32_t first,
                      uint32_t count, const uint32_t* pair_a, const uint32_t* pair_b, int uses_contra_model,
                      float* match_probs, const uint64_t* out_offsets, float* bound_a, float* bound_b,
                      const uint64_t* bound_offsets, float* log_partition, uint8_t* structs,
                      const uint64_t* struct_offsets, float* best_scores) {
  const char* who = "rnamc_duplex_batch";
  const bool want_bound = bound_a || bound_b, want_best = structs || best_scores;
  const bool need_g = match_probs || want_bound, need_f = need_g || log_partition;
  // workspace floats per cell: F and G are f64, the max-plus matrix f32
  const uint64_t n_mat = (need_f ? 2u : 0u) + (need_g ? 2u : 0u) + (want_best ? 1u : 0u);
  if (count == 0 || n_mat == 0) return RNAMC_OK;
  // the records the band names, gathered: a device holds nothing else of the batch
  std::unordered_map<uint32_t, uint64_t> local;
  std::vector<uint8_t> h_bases;
  std::vector<DuplexPair> chunk;
  std::vector<DuplexRes> h_res;
  std::vector<float> h_out;
  std::vector<uint8_t> h_structs;
  auto len_of = [&](uint32_t s) { return static_cast<uint32_t>(offsets[s + 1] - offsets[s]); };
  try {  // nothing may throw across the C boundary
    for (uint32_t p = first; p < first + count; p++)
      for (uint32_t s : {pair_a[p], pair_b[p]})
        if (local.emplace(s, h_bases.size()).second)
          h_bases.insert(h_bases.end(), bases + offsets[s], bases + offsets[s + 1]);
  } catch (const std::exception&) {
    return no_host_memory(who);
  }
  // a pair that cannot fit the chunk budget fails the call before anything is launched
  const uint64_t ws_cap = static_cast<uint64_t>(std::max<int64_t>(c->group_ws_bytes, 1)) / sizeof(float);
  for (uint32_t p = first; p < first + count; p++) {
    const uint64_t cells = static_cast<uint64_t>(len_of(pair_a[p])) * len_of(pair_b[p]);
    if (n_mat * cells + 1u > ws_cap) {
      set_last_error(std::string(who) + ": pair " + std::to_string(p) + " needs " +
                     std::to_string((n_mat * cells + 1u) * sizeof(float)) + " bytes of workspace, group_ws_bytes is " +
                     std::to_string(c->group_ws_bytes));
      return RNAMC_ERR_OOM;
    }
  }
  std::lock_guard<std::mutex> lock(c->mu);
  DeviceGuard guard(c->device);
  if (!guard.ok) return RNAMC_ERR_NO_DEVICE;
  hipStream_t st = c->own_stream;
  // whatever happens, nothing of this call still runs when its host buffers go
  struct Drain {
    hipStream_t st;
    ~Drain() { (void)hipStreamSynchronize(st); }
  } drain{st};
  HIPCHK(hipStreamSynchronize(st));
  HIPCHK(c->st_bases.upload(h_bases.data(), h_bases.size(), st));
  for (uint32_t p0 = first; p0 < first + count;) {
    chunk.clear();
    uint64_t ws = 0, probs = 0, bounds = 0, sbytes = 0, max_cells = 0;
    uint32_t max_a = 0, max_b = 0, max_bases = 0, p = p0;
    try {
      for (; p < first + count; p++) {
        DuplexPair dp{};
        dp.na = len_of(pair_a[p]);
        dp.nb = len_of(pair_b[p]);
        const uint64_t cells = static_cast<uint64_t>(dp.na) * dp.nb;
        // (the kernels index pairs through a grid dimension: at most 65535 a launch)
        if (!chunk.empty() && (ws + n_mat * cells + 1u > ws_cap || chunk.size() >= 65535u)) break;
        dp.a_off = local[pair_a[p]];
        dp.b_off = local[pair_b[p]];
        if (need_f) dp.f_off = ws, ws += 2u * cells;
        if (need_g) dp.g_off = ws, ws += 2u * cells;
        if (want_best) dp.m_off = ws, ws += cells;
        ws += ws & 1u;  // (the next pair's f64 matrices start on an even float)
        dp.prob_off = probs;
        if (match_probs) probs += cells;
        dp.bound_off = bounds;
        if (want_bound) bounds += dp.na + dp.nb;
        dp.struct_off = sbytes;
        if (structs) sbytes += dp.na + dp.nb;
        chunk.push_back(dp);
        max_a = std::max(max_a, dp.na);
        max_b = std::max(max_b, dp.nb);
        max_cells = std::max(max_cells, cells);
        max_bases = std::max(max_bases, dp.na + dp.nb);
      }
      // (the bound probabilities sit behind the match probabilities in one staged array)
      for (DuplexPair& dp : chunk) dp.bound_off += probs;
      h_res.resize(chunk.size());
      h_out.resize(probs + bounds);
      h_structs.resize(sbytes);
    } catch (const std::exception&) {
      return no_host_memory(who);
    }
    const uint32_t m = static_cast<uint32_t>(chunk.size());
    if (int rc = ensure_ws(c, ws)) return rc;
    HIPCHK(c->dx_pairs.upload(chunk.data(), m, st));
    HIPCHK(c->dx_res.grow(m));
    HIPCHK(c->dx_out.grow(std::max<uint64_t>(probs + bounds, 1)));
    HIPCHK(c->dx_structs.grow(std::max<uint64_t>(sbytes, 1)));
    DuplexChunk ch{};
    ch.pairs = c->dx_pairs;
    ch.bases = c->st_bases;
    ch.ws = c->d_ws;
    ch.params = c->d_params;
    ch.res = c->dx_res;
    ch.probs = match_probs ? c->dx_out.get() : nullptr;
    ch.bound = want_bound ? c->dx_out.get() : nullptr;
    ch.structs = structs ? c->dx_structs.get() : nullptr;
    ch.n_pairs = m;
    // along the strand that makes fewer steps for the chunk (a tie: along A); the results do not
    // depend on it
    ch.by_col = max_b < max_a ? 1u : 0u;
    ch.contra = uses_contra_model != 0 ? 1u : 0u;
    const uint32_t steps = ch.by_col ? max_b : max_a, max_lane = ch.by_col ? max_a : max_b;
    if (need_f) {
      for (uint32_t s = 0; s < steps; s++) launch_duplex_step(ch, 0, s, max_lane, st);
      launch_duplex_reduce(ch, 0, st);
    }
    if (need_g) {
      for (uint32_t s = 0; s < steps; s++) launch_duplex_step(ch, 1, s, max_lane, st);
      launch_duplex_probs(ch, max_cells, max_bases, st);
    }
    if (want_best) {
      for (uint32_t s = 0; s < steps; s++) launch_duplex_step(ch, 2, s, max_lane, st);
      launch_duplex_reduce(ch, 2, st);
      if (structs) launch_duplex_trace(ch, st);
    }
    HIPCHK(hipGetLastError());
    // one copy of each kind per chunk, scattered on the host
    HIPCHK(hipMemcpyAsync(h_res.data(), c->dx_res, m * sizeof(DuplexRes), hipMemcpyDeviceToHost, st));
    if (probs + bounds)
      HIPCHK(hipMemcpyAsync(h_out.data(), c->dx_out, (probs + bounds) * sizeof(float), hipMemcpyDeviceToHost, st));
    if (sbytes) HIPCHK(hipMemcpyAsync(h_structs.data(), c->dx_structs, sbytes, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (uint32_t x = 0; x < m; x++) {
      const DuplexPair& dp = chunk[x];
      const uint32_t q = p0 + x;
      if (log_partition) log_partition[q] = static_cast<float>(h_res[x].log_z);
      if (best_scores) best_scores[q] = h_res[x].best;
      if (match_probs)
        std::memcpy(match_probs + out_offsets[q], h_out.data() + dp.prob_off,
                    static_cast<uint64_t>(dp.na) * dp.nb * sizeof(float));
      if (bound_a) std::memcpy(bound_a + bound_offsets[q], h_out.data() + dp.bound_off, dp.na * sizeof(float));
      if (bound_b)
        std::memcpy(bound_b + bound_offsets[q] + dp.na, h_out.data() + dp.bound_off + dp.na, dp.nb * sizeof(float));
      if (structs) std::memcpy(structs + struct_offsets[q], h_structs.data() + dp.struct_off, dp.na + dp.nb);
    }
    p0 = p;
  }
  return RNAMC_OK;
}

namespace {

// the three parts of a duplex's log weight in f64 over the f32 loop scores of `M`, on S = A || B and
// R = B || A
template <class Model>
double duplex_log_weight(const Model& M, const rnamc_params& P, bool contra, const uint8_t* S, const uint8_t* R,
                         uint32_t na, uint32_t nb, uint32_t m, const uint32_t* ci, const uint32_t* cj) {
  const double ninf = -std::numeric_limits<double>::infinity();
  const uint32_t n = na + nb;
  for (uint32_t x = 0; x < m; x++)
    if (!canonical(S[ci[x]], S[na + cj[x]])) return ninf;
  double w = M.accessible(S, n, ci[0], na + cj[0]);
  for (uint32_t x = 0; x + 1 < m; x++) {
    const uint32_t a = ci[x + 1] - ci[x] - 1, b = cj[x] - cj[x + 1] - 1;
    if (a + b > RNAMC_MAX_2LOOP_LEN) return ninf;
    w += static_cast<double>(M.twoloop(S, ci[x], na + cj[x], ci[x + 1], na + cj[x + 1]));
  }
  const uint32_t i = ci[m - 1], j = cj[m - 1];
  w += static_cast<double>(M.accessible(R, n, j, nb + i));
  // (the chain has counted the last pair's base-pair score already)
  if (contra) w -= static_cast<double>(P.contra.basepair_scores[R[j]][R[nb + i]]);
  return w;
}

}  // namespace

}  // namespace rnamc

extern "C" {

int rnamc_duplex_batch(rnamc_ctx* c, uint32_t n_seqs, const uint8_t* bases, const uint64_t* offsets,
                       uint32_t n_pairs, const uint32_t* pair_a, const uint32_t* pair_b,
                       int uses_contra_model, float* match_probs, const uint64_t* out_offsets,
                       float* bound_a, float* bound_b, const uint64_t* bound_offsets,
                       float* log_partition, uint8_t* structs, const uint64_t* struct_offsets,
                       float* best_scores) {
  if (!c) return RNAMC_ERR_INVALID_ARG;
  if (int rc = duplex_batch_check(n_seqs, bases, offsets, n_pairs, pair_a, pair_b, match_probs, out_offsets,
                                  bound_a, bound_b, bound_offsets, structs, struct_offsets))
    return rc;
  if (n_pairs == 0) return RNAMC_OK;
  return duplex_batch_core(c, bases, offsets, 0, n_pairs, pair_a, pair_b, uses_contra_model, match_probs,
                           out_offsets, bound_a, bound_b, bound_offsets, log_partition, structs, struct_offsets,
                           best_scores);
}

int rnamc_duplex_score(const rnamc_params* params, const uint8_t* a, uint32_t n_a, const uint8_t* b,
                       uint32_t n_b, uint32_t n_chain, const uint32_t* chain_i, const uint32_t* chain_j,
                       int uses_contra_model, double* log_weight) {
  if (!params || !a || !b || !chain_i || !chain_j || !log_weight) return RNAMC_ERR_INVALID_ARG;
  if (params->abi_version != RNAMC_ABI_VERSION || params->struct_bytes != sizeof(rnamc_params))
    return RNAMC_ERR_INVALID_ARG;
  if (n_a == 0 || n_b == 0) return RNAMC_ERR_EMPTY_SEQ;
  if (n_a > RNAMC_MAX_SEQ_LEN || n_b > RNAMC_MAX_SEQ_LEN) return RNAMC_ERR_SEQ_TOO_LONG;
  for (uint32_t x = 0; x < n_a; x++)
    if (a[x] > 3) return RNAMC_ERR_INVALID_BASE;
  for (uint32_t x = 0; x < n_b; x++)
    if (b[x] > 3) return RNAMC_ERR_INVALID_BASE;
  if (n_chain == 0) return RNAMC_ERR_INVALID_ARG;
  for (uint32_t x = 0; x < n_chain; x++) {
    if (chain_i[x] >= n_a || chain_j[x] >= n_b) return RNAMC_ERR_INVALID_ARG;
    if (x && !(chain_i[x] > chain_i[x - 1] && chain_j[x] < chain_j[x - 1])) return RNAMC_ERR_INVALID_ARG;
  }
  std::vector<uint8_t> S, R;
  try {  // nothing may throw across the C boundary
    S.assign(a, a + n_a);
    S.insert(S.end(), b, b + n_b);
    R.assign(b, b + n_b);
    R.insert(R.end(), a, a + n_a);
  } catch (const std::exception&) {
    return no_host_memory("rnamc_duplex_score");
  }
  const bool contra = uses_contra_model != 0;
  // (the Turner scorer's hairpin table is never read: a duplex has no hairpin)
  *log_weight = contra ? duplex_log_weight(Contra{params->contra}, *params, true, S.data(), R.data(), n_a, n_b,
                                           n_chain, chain_i, chain_j)
                       : duplex_log_weight(Turner{params->turner, nullptr}, *params, false, S.data(), R.data(), n_a,
                                           n_b, n_chain, chain_i, chain_j);
  return RNAMC_OK;
}

}  // extern "C"
