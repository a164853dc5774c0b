// rna_algos/mccaskill_algo.hpp — C++ host-side mirror of the reference crate's
// `mccaskill_algo`, `utils` (the part this path uses) and `centroid_fold` modules
// over the C ABI of librnamc.so (include/rnamc.h).  Header-only, C++17.
//
// The reference is a Rust library; its toolchain is absent from this build
// environment, so the host layer above the C ABI is written in C++ with the
// reference's names, argument meaning and error behaviour (a non-zero status
// throws where the reference panics).  Reference items mirrored:
//   src/mccaskill_algo.rs:247-255  pub fn mccaskill_algo<T>(seq, uses_contra_model,
//                                  allows_short_hairpins, fold_score_sets)
//                                  -> (SparseProbMat<T>, FoldScores<T>)
//   src/mccaskill_algo.rs:24-211   impl FoldScoreSets { new, accumulate, transfer }
//   src/utils.rs:45-89,562-577     PosPair, SparseProbMat, Prob, Seq, bytes2seq
//   src/centroid_fold.rs:4-7,25    CentroidFold<T>, centroid_fold<T>
#ifndef RNA_ALGOS_MCCASKILL_ALGO_HPP
#define RNA_ALGOS_MCCASKILL_ALGO_HPP

#include <algorithm>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../rnamc.h"

namespace rna_algos {

using Prob = float;
using Score = float;
using Base = uint8_t;               // codes A,C,G,U = 0,1,2,3 (usize in the reference)
using Seq = std::vector<Base>;
template <class T>
using PosPair = std::pair<T, T>;
template <class T>
using PosQuad = std::tuple<T, T, T, T>;

struct PosPairHash {
  template <class T>
  size_t operator()(const std::pair<T, T>& p) const noexcept {
    return (static_cast<size_t>(p.first) << 32) ^ static_cast<size_t>(p.second);
  }
};
template <class T>
using SparseProbMat = std::unordered_map<PosPair<T>, Prob, PosPairHash>;
template <class T>
using SparseScoreMat = std::unordered_map<PosPair<T>, Score, PosPairHash>;

constexpr Prob EPSILON = 0.001f;
constexpr Prob PROB_BOUND_LOWER = -EPSILON;
constexpr Prob PROB_BOUND_UPPER = 1.f + EPSILON;

struct RnamcError : std::runtime_error {
  int status;
  RnamcError(int st) : std::runtime_error(std::string("rnamc: ") + rnamc_strerror(st) + " (" +
                                          rnamc_last_error() + ")"), status(st) {}
};
inline void check(int st) {
  if (st != RNAMC_OK) throw RnamcError(st);  // the reference panics
}

// bytes2seq, src/utils.rs:562-577
inline Seq bytes2seq(const std::string& x) {
  Seq y(x.size());
  check(rnamc_bytes2seq(reinterpret_cast<const uint8_t*>(x.data()), x.size(), y.data()));
  return y;
}

// FoldScoreSets, src/utils.rs:91-119.  `contra` carries the fields of the reference
// struct under their own names; `turner` the constants the reference reads from
// rna-ss-params directly.
struct FoldScoreSets {
  std::unique_ptr<rnamc_params> p{new rnamc_params};
  explicit FoldScoreSets(Score init_val = 0.f) { check(rnamc_params_new(init_val, p.get())); }
  static FoldScoreSets new_(Score init_val) { return FoldScoreSets(init_val); }
  static FoldScoreSets synthetic(uint64_t seed) {
    FoldScoreSets f;
    check(rnamc_params_synthetic(seed, f.p.get()));
    return f;
  }
  static FoldScoreSets load(const std::string& path) {
    FoldScoreSets f;
    check(rnamc_params_load(path.c_str(), f.p.get()));
    return f;
  }
  void accumulate() { check(rnamc_fold_score_sets_accumulate(&p->contra)); }
  // transfer(): the "compiled" tables come from `src` (a table file or the synthetic set)
  void transfer(const FoldScoreSets& src) {
    p->turner = src.p->turner;
    p->table_id = src.p->table_id;
    check(rnamc_fold_score_sets_transfer(&p->contra, &src.p->contra));
  }
  rnamc_fold_score_sets& contra() { return p->contra; }
  rnamc_turner_scores& turner() { return p->turner; }
};

// FoldScores<T>, src/mccaskill_algo.rs:13-19 — side products no in-crate caller reads, so
// mccaskill_algo leaves them empty unless asked (with_fold_scores); fold_scores<T> fills
// them through rnamc_fold_scores.  twoloop_scores is keyed by quad_key(i,j,k,l).
inline uint64_t quad_key(uint64_t i, uint64_t j, uint64_t k, uint64_t l) {
  return (i << 48) | (j << 32) | (k << 16) | l;
}
template <class T>
struct FoldScores {
  SparseScoreMat<T> hairpin_scores;
  std::unordered_map<uint64_t, Score> twoloop_scores;
  SparseScoreMat<T> multibranch_close_scores;
  SparseScoreMat<T> accessible_scores;
};

// One device context per FoldScoreSets (tables uploaded once).
class Context {
 public:
  explicit Context(const FoldScoreSets& f, int device = -1) {
    check(rnamc_ctx_create(f.p.get(), device, 0, &ctx_));
  }
  ~Context() { rnamc_ctx_destroy(ctx_); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  rnamc_ctx* get() const { return ctx_; }

 private:
  rnamc_ctx* ctx_ = nullptr;
};

template <class T>
SparseProbMat<T> unpack(const float* packed, uint32_t n) {
  SparseProbMat<T> m;
  size_t x = 0;
  for (uint32_t d = 0; d < n; d++)
    for (uint32_t i = 0; i + d < n; i++, x++)
      if (packed[x] >= -0.5f) m.emplace(PosPair<T>(static_cast<T>(i), static_cast<T>(i + d)), packed[x]);
  return m;
}

// the four maps the reference's inside pass fills (src/mccaskill_algo.rs:302-304, 320,
// 333-338 / 407-409, 431, 457-462)
template <class T>
FoldScores<T> fold_scores(const Context& ctx, const Seq& seq, bool uses_contra_model,
                          bool allows_short_hairpins) {
  const uint32_t n = static_cast<uint32_t>(seq.size());
  const uint64_t len = rnamc_bpp_len(n);
  std::vector<float> hp(len ? len : 1), mb(hp.size()), ac(hp.size());
  uint64_t count = 0;
  check(rnamc_fold_scores(ctx.get(), seq.data(), n, uses_contra_model, allows_short_hairpins,
                          hp.data(), mb.data(), ac.data(), nullptr, 0, &count));
  std::vector<rnamc_twoloop_score> tl(count ? count : 1);
  check(rnamc_fold_scores(ctx.get(), seq.data(), n, uses_contra_model, allows_short_hairpins,
                          nullptr, nullptr, nullptr, tl.data(), count, &count));
  FoldScores<T> out;
  uint64_t x = 0;
  for (uint32_t d = 0; d < n; d++)
    for (uint32_t i = 0; i + d < n; i++, x++) {
      const PosPair<T> key{static_cast<T>(i), static_cast<T>(i + d)};
      if (hp[x] == hp[x]) out.hairpin_scores.emplace(key, hp[x]);
      if (mb[x] == mb[x]) out.multibranch_close_scores.emplace(key, mb[x]);
      if (ac[x] == ac[x]) out.accessible_scores.emplace(key, ac[x]);
    }
  out.twoloop_scores.reserve(count);
  for (uint64_t e = 0; e < count; e++)
    out.twoloop_scores.emplace(quad_key(tl[e].i, tl[e].j, tl[e].k, tl[e].l), tl[e].score);
  return out;
}

// FoldSums<T>, src/mccaskill_algo.rs:3-11: the value of the reference's first stage
// (get_fold_sums / get_fold_sums_contra, 282 / 380), through rnamc_fold_sums (inside sweep alone)
using SumMat = std::vector<std::vector<Score>>;
template <class T>
struct FoldSums {
  SumMat sums_external;
  SumMat sums_rightmost_basepairs_external;
  SumMat sums_rightmost_basepairs_multibranch;
  SparseScoreMat<T> sums_close;
  SparseScoreMat<T> sums_accessible;
  SumMat sums_multibranch;
  SumMat sums_1ormore_basepairs;
};
template <class T>
FoldSums<T> get_fold_sums(const Context& ctx, const Seq& seq, bool uses_contra_model,
                          bool allows_short_hairpins) {
  const uint32_t n = static_cast<uint32_t>(seq.size());
  std::vector<std::vector<float>> m(7, std::vector<float>(static_cast<size_t>(n) * n + 1));
  check(rnamc_fold_sums(ctx.get(), seq.data(), n, uses_contra_model, allows_short_hairpins,
                        m[0].data(), m[1].data(), m[2].data(), m[3].data(), m[4].data(), m[5].data(),
                        m[6].data()));
  auto rows = [n](const std::vector<float>& v) {
    SumMat out(n);
    for (uint32_t i = 0; i < n; i++) out[i].assign(v.begin() + static_cast<size_t>(i) * n, v.begin() + static_cast<size_t>(i + 1) * n);
    return out;
  };
  auto sparse = [n](const std::vector<float>& v) {
    SparseScoreMat<T> out;  // finite sums only, as the reference inserts them (332-338 / 456-462)
    for (uint32_t i = 0; i < n; i++)
      for (uint32_t j = i; j < n; j++) {
        const float x = v[static_cast<size_t>(i) * n + j];
        if (x - x == 0.f) out.emplace(PosPair<T>(static_cast<T>(i), static_cast<T>(j)), x);
      }
    return out;
  };
  return {rows(m[0]), rows(m[1]), rows(m[2]), sparse(m[3]), sparse(m[4]), rows(m[5]), rows(m[6])};
}

// mccaskill_algo, src/mccaskill_algo.rs:247-280
template <class T>
std::pair<SparseProbMat<T>, FoldScores<T>> mccaskill_algo(const Context& ctx, const Seq& seq,
                                                          bool uses_contra_model,
                                                          bool allows_short_hairpins,
                                                          bool with_fold_scores = false) {
  const uint32_t n = static_cast<uint32_t>(seq.size());
  const uint64_t offsets[2] = {0, n};
  const uint64_t out_offsets[2] = {0, rnamc_bpp_len(n)};
  std::vector<float> packed(rnamc_bpp_len(n) ? rnamc_bpp_len(n) : 1);
  float logz = 0.f;
  check(rnamc_bpp_batch(ctx.get(), 1, seq.data(), offsets, uses_contra_model, allows_short_hairpins,
                        packed.data(), out_offsets, &logz));
  return {unpack<T>(packed.data(), n),
          with_fold_scores ? fold_scores<T>(ctx, seq, uses_contra_model, allows_short_hairpins)
                           : FoldScores<T>()};
}

// the whole FASTA at once (what src/bin/mccaskill_algo.rs:64-93 does on a thread pool)
template <class T>
std::vector<SparseProbMat<T>> mccaskill_algo_batch(const Context& ctx, const std::vector<Seq>& seqs,
                                                   bool uses_contra_model,
                                                   bool allows_short_hairpins) {
  std::vector<uint64_t> off(seqs.size() + 1, 0), ooff(seqs.size() + 1, 0);
  for (size_t s = 0; s < seqs.size(); s++) {
    off[s + 1] = off[s] + seqs[s].size();
    ooff[s + 1] = ooff[s] + rnamc_bpp_len(static_cast<uint32_t>(seqs[s].size()));
  }
  std::vector<Base> bases(off.back());
  for (size_t s = 0; s < seqs.size(); s++) std::copy(seqs[s].begin(), seqs[s].end(), bases.begin() + off[s]);
  std::vector<float> packed(ooff.back() ? ooff.back() : 1);
  check(rnamc_bpp_batch(ctx.get(), static_cast<uint32_t>(seqs.size()), bases.data(), off.data(),
                        uses_contra_model, allows_short_hairpins, packed.data(), ooff.data(), nullptr));
  std::vector<SparseProbMat<T>> out;
  for (size_t s = 0; s < seqs.size(); s++)
    out.push_back(unpack<T>(packed.data() + ooff[s], static_cast<uint32_t>(seqs[s].size())));
  return out;
}

// mccaskill_algo_batch keeping only the pairs with p >= min_prob (finite, >= 0; 0 keeps every key),
// compacted on the device (rnamc_bpp_batch_sparse): the dense triangles never reach the host.  The
// lists are sized at a few entries per nucleotide (capped at the cells that can pair); a call that
// reports more is repeated once with the exact total.
template <class T>
std::vector<SparseProbMat<T>> mccaskill_algo_batch_sparse(const Context& ctx, const std::vector<Seq>& seqs,
                                                          bool uses_contra_model, bool allows_short_hairpins,
                                                          float min_prob) {
  std::vector<uint64_t> off(seqs.size() + 1, 0);
  uint64_t most = 0;
  for (size_t s = 0; s < seqs.size(); s++) {
    off[s + 1] = off[s] + seqs[s].size();
    most += rnamc_bpp_len(static_cast<uint32_t>(seqs[s].size())) - seqs[s].size();
  }
  std::vector<Base> bases(off.back());
  for (size_t s = 0; s < seqs.size(); s++) std::copy(seqs[s].begin(), seqs[s].end(), bases.begin() + off[s]);
  std::vector<uint64_t> start(seqs.size() + 1), count(seqs.size() + 1);
  std::vector<uint32_t> pi, pj;
  std::vector<float> pp;
  uint64_t cap = std::max<uint64_t>(std::min<uint64_t>(4 * off.back(), most), 1), total = 0;
  for (int attempt = 0; attempt < 2; attempt++) {
    pi.resize(cap);
    pj.resize(cap);
    pp.resize(cap);
    const int st = rnamc_bpp_batch_sparse(ctx.get(), static_cast<uint32_t>(seqs.size()), bases.data(), off.data(),
                                          nullptr, 0, uses_contra_model, allows_short_hairpins, min_prob,
                                          start.data(), count.data(), pi.data(), pj.data(), pp.data(), cap, &total,
                                          nullptr, nullptr);
    if (st != RNAMC_OK && attempt == 0 && total > cap) {
      cap = total;
      continue;
    }
    check(st);
    break;
  }
  std::vector<SparseProbMat<T>> out(seqs.size());
  for (size_t s = 0; s < seqs.size(); s++)
    for (uint64_t x = start[s]; x < start[s] + count[s]; x++)
      out[s].emplace(PosPair<T>(static_cast<T>(pi[x]), static_cast<T>(pj[x])), pp[x]);
  return out;
}

// Structural context profiles (rnamc_context_profile_batch; CapR's profile): per record six rows of
// n floats, row-major, in the order bulge, exterior, hairpin, internal, multibranch, stem.
inline std::vector<std::vector<float>> context_profile_batch(const Context& ctx, const std::vector<Seq>& seqs,
                                                             bool uses_contra_model, bool allows_short_hairpins) {
  std::vector<uint64_t> off(seqs.size() + 1, 0);
  for (size_t s = 0; s < seqs.size(); s++) off[s + 1] = off[s] + seqs[s].size();
  std::vector<Base> bases(off.back());
  for (size_t s = 0; s < seqs.size(); s++) std::copy(seqs[s].begin(), seqs[s].end(), bases.begin() + off[s]);
  std::vector<float> prof(6 * off.back() + 1);
  check(rnamc_context_profile_batch(ctx.get(), static_cast<uint32_t>(seqs.size()), bases.data(), off.data(), nullptr,
                                    0, uses_contra_model, allows_short_hairpins, prof.data(), nullptr));
  std::vector<std::vector<float>> out(seqs.size());
  for (size_t s = 0; s < seqs.size(); s++) out[s].assign(prof.begin() + 6 * off[s], prof.begin() + 6 * off[s + 1]);
  return out;
}

// Windowed local folding of one sequence of any length below 2^31 (rnamc_bpp_windowed; no counterpart
// in the reference): every window of `window` bases (starts 0, stride, 2 stride, ..., and a last window
// ending at the sequence's end) folded with max_bp_span (0: no limit), each pair's probability averaged
// over the windows that contain it.  band[i * band_width + d] is pair (i, i + d), -1 where no window had it.
struct WindowedBpp {
  std::vector<float> band, paired_prob, window_log_partition;
  std::vector<uint64_t> starts;
  uint32_t band_width = 0;
};
inline WindowedBpp mccaskill_algo_windowed(const Context& ctx, const Seq& seq, uint32_t window, uint32_t stride,
                                           uint32_t max_bp_span, bool uses_contra_model,
                                           bool allows_short_hairpins) {
  WindowedBpp r;
  uint64_t n_windows = 0;
  check(rnamc_window_plan(seq.size(), window, stride, max_bp_span, &n_windows, &r.band_width, nullptr, 0));
  r.starts.resize(n_windows);
  check(rnamc_window_plan(seq.size(), window, stride, max_bp_span, &n_windows, &r.band_width, r.starts.data(),
                          n_windows));
  r.band.resize(seq.size() * r.band_width);
  r.paired_prob.resize(seq.size());
  r.window_log_partition.resize(n_windows);
  check(rnamc_bpp_windowed(ctx.get(), seq.data(), seq.size(), nullptr, window, stride, max_bp_span,
                           uses_contra_model, allows_short_hairpins, r.band.data(), r.paired_prob.data(),
                           r.window_log_partition.data()));
  return r;
}
// the same over a pool's devices: rnamc_bpp_windowed_multi (same arguments, a rnamc_pool* first)

// Alignment folding (rnamc_bpp_alignment; the consumer of the reference's read_align_* readers): the rows
// of an alignment (n_rows x n_cols codes, row-major: 0..3 a base, 4 = PSEUDO_BASE a gap) folded without
// their gaps, the pair probabilities averaged per COLUMN pair over all rows on the device, one
// gamma-centroid fold of the averaged matrix per threshold.  bpp is the packed diagonal-major triangle
// over the columns (rnamc_bpp_index(n_cols, ci, cj); -1 where no row had the pair).
struct AlignmentBpp {
  uint32_t n_cols = 0;
  std::vector<float> bpp, col_paired, expect_accuracy, log_partition;
  std::vector<std::string> folds;  // one dot-bracket string over the columns per threshold
  std::vector<uint32_t> n_pairs, row_len;
};
inline AlignmentBpp alignment_fold(const Context& ctx, const std::vector<uint8_t>& rows, uint32_t n_rows,
                                   uint32_t n_cols, bool uses_contra_model, bool allows_short_hairpins,
                                   const std::vector<float>& centroid_thresholds = {}, uint32_t max_bp_span = 0) {
  if (rows.size() != static_cast<size_t>(n_rows) * n_cols) check(RNAMC_ERR_INVALID_ARG);
  AlignmentBpp r;
  r.n_cols = n_cols;
  const uint32_t ng = static_cast<uint32_t>(centroid_thresholds.size());
  r.bpp.resize(rnamc_bpp_len(n_cols));
  r.col_paired.resize(n_cols);
  r.expect_accuracy.resize(ng);
  r.n_pairs.resize(ng);
  r.log_partition.resize(n_rows);
  r.row_len.resize(n_rows);
  std::vector<uint8_t> structs(static_cast<size_t>(ng) * n_cols);
  check(rnamc_bpp_alignment(ctx.get(), n_rows, n_cols, rows.data(), max_bp_span, uses_contra_model,
                            allows_short_hairpins, ng ? centroid_thresholds.data() : nullptr, ng, r.bpp.data(),
                            r.col_paired.data(), ng ? structs.data() : nullptr, ng ? r.n_pairs.data() : nullptr,
                            ng ? r.expect_accuracy.data() : nullptr, r.log_partition.data(), r.row_len.data()));
  for (uint32_t g = 0; g < ng; g++)
    r.folds.emplace_back(reinterpret_cast<const char*>(structs.data()) + static_cast<size_t>(g) * n_cols, n_cols);
  return r;
}
// the same over a pool's devices: rnamc_bpp_alignment_multi (same arguments, a rnamc_pool* first)

// Point-mutation scan of one sequence (rnamc_mutant_scan; no counterpart in the reference): every
// single-base mutant of `positions` (empty: every base; three mutants per position, base codes ascending
// without the wild type's) folded and its pair-probability matrix compared with the wild type's on the
// device.  dist2_q is the squared Euclidean distance in units of 2^-44, max_i = max_j = 0xffffffff where
// no pair moved, paired_prob holds one row of seq.size() per mutant.
struct MutantScan {
  std::vector<uint32_t> pos, max_i, max_j;
  std::vector<uint8_t> base;
  std::vector<float> log_partition, max_dp, paired_prob, wt_paired_prob;
  std::vector<int64_t> dist2_q;
  float wt_log_partition = 0.f;
  double dist2(size_t m) const { return static_cast<double>(dist2_q[m]) / 17592186044416.0; }  // 2^44
};
inline MutantScan mutant_scan(const Context& ctx, const Seq& seq, bool uses_contra_model, bool allows_short_hairpins,
                              const std::vector<uint32_t>& positions = {}, uint32_t max_bp_span = 0,
                              const char* constraint = nullptr) {
  MutantScan r;
  const uint32_t n = static_cast<uint32_t>(seq.size());
  const uint32_t* pos = positions.empty() ? nullptr : positions.data();
  const uint32_t n_pos = static_cast<uint32_t>(positions.size());
  uint64_t m = 0;
  check(rnamc_mutant_plan(seq.data(), n, pos, n_pos, &m, nullptr, nullptr, 0));
  r.pos.resize(m);
  r.base.resize(m);
  check(rnamc_mutant_plan(seq.data(), n, pos, n_pos, &m, r.pos.data(), r.base.data(), m));
  r.log_partition.resize(m ? m : 1);
  r.dist2_q.resize(m);
  r.max_dp.resize(m);
  r.max_i.resize(m);
  r.max_j.resize(m);
  r.paired_prob.resize(m * n);
  r.wt_paired_prob.resize(n);
  check(rnamc_mutant_scan(ctx.get(), seq.data(), n, constraint, max_bp_span, uses_contra_model, allows_short_hairpins,
                          pos, n_pos, r.log_partition.data(), r.dist2_q.data(), r.max_dp.data(), r.max_i.data(),
                          r.max_j.data(), r.paired_prob.data(), &r.wt_log_partition, r.wt_paired_prob.data()));
  r.log_partition.resize(m);
  return r;
}
// the same over a pool's devices: rnamc_mutant_scan_multi (same arguments, a rnamc_pool* first)

// Boltzmann sampling (rnamc_sample_batch; no counterpart in the reference): n_samples structures
// per sequence, each drawn with probability exp(log_weight) / exp(log_partition).  Sample t of
// sequence s is a pure function of (tables, sequence, flags, seed, s, t).
struct SampledStructure {
  std::string dot_bracket;
  Score log_weight = 0.f;
};
struct SampleSet {
  std::vector<std::vector<SampledStructure>> samples;  // [sequence][sample]
  std::vector<Score> log_partition;                     // sums_external[0][n-1] per sequence
};
inline SampleSet sample_structures_batch(const Context& ctx, const std::vector<Seq>& seqs,
                                         uint32_t n_samples, bool uses_contra_model,
                                         bool allows_short_hairpins, uint64_t seed = 0) {
  std::vector<uint64_t> off(seqs.size() + 1, 0);
  for (size_t s = 0; s < seqs.size(); s++) off[s + 1] = off[s] + seqs[s].size();
  std::vector<Base> bases(off.back() ? off.back() : 1);
  for (size_t s = 0; s < seqs.size(); s++) std::copy(seqs[s].begin(), seqs[s].end(), bases.begin() + off[s]);
  std::vector<uint8_t> rows(std::max<uint64_t>(off.back() * n_samples, 1));
  std::vector<float> weights(std::max<size_t>(seqs.size() * n_samples, 1));
  SampleSet out;
  out.log_partition.assign(seqs.size(), 0.f);
  check(rnamc_sample_batch(ctx.get(), static_cast<uint32_t>(seqs.size()), bases.data(), off.data(),
                           uses_contra_model, allows_short_hairpins, n_samples, seed, rows.data(),
                           weights.data(), out.log_partition.empty() ? nullptr : out.log_partition.data()));
  out.samples.resize(seqs.size());
  for (size_t s = 0; s < seqs.size(); s++) {
    const size_t n = seqs[s].size();
    for (uint32_t t = 0; t < n_samples; t++) {
      const char* r = reinterpret_cast<const char*>(rows.data() + n_samples * off[s] + t * n);
      out.samples[s].push_back({std::string(r, n), weights[s * n_samples + t]});
    }
  }
  return out;
}
inline std::vector<SampledStructure> sample_structures(const Context& ctx, const Seq& seq,
                                                       uint32_t n_samples, bool uses_contra_model,
                                                       bool allows_short_hairpins, uint64_t seed = 0) {
  return std::move(sample_structures_batch(ctx, {seq}, n_samples, uses_contra_model,
                                           allows_short_hairpins, seed).samples[0]);
}

// log Boltzmann weight of one structure (rnamc_structure_score, host only): -inf outside the
// model's structure space
inline double structure_score(const FoldScoreSets& f, const Seq& seq, const std::string& dot_bracket,
                              bool uses_contra_model, bool allows_short_hairpins) {
  double w = 0;
  check(rnamc_structure_score(f.p.get(), seq.data(), static_cast<uint32_t>(seq.size()),
                              dot_bracket.c_str(), uses_contra_model, allows_short_hairpins, &w));
  return w;
}

// Maximum-score structure (rnamc_mfe_batch; no counterpart in the reference): MFE under Turner,
// the Viterbi parse under CONTRAfold.  score = the f32 sum of the structure's loop scores (compare
// structure_score), dp_score = the max-plus sweep's value.
struct MfeStructure {
  std::string dot_bracket;
  Score score = 0.f;
  Score dp_score = 0.f;
};
inline std::vector<MfeStructure> mfe_fold_batch(const Context& ctx, const std::vector<Seq>& seqs,
                                                bool uses_contra_model, bool allows_short_hairpins) {
  std::vector<uint64_t> off(seqs.size() + 1, 0);
  for (size_t s = 0; s < seqs.size(); s++) off[s + 1] = off[s] + seqs[s].size();
  std::vector<Base> bases(off.back() ? off.back() : 1);
  for (size_t s = 0; s < seqs.size(); s++) std::copy(seqs[s].begin(), seqs[s].end(), bases.begin() + off[s]);
  std::vector<uint8_t> rows(std::max<uint64_t>(off.back(), 1));
  std::vector<float> scores(std::max<size_t>(seqs.size(), 1)), dp(std::max<size_t>(seqs.size(), 1));
  check(rnamc_mfe_batch(ctx.get(), static_cast<uint32_t>(seqs.size()), bases.data(), off.data(),
                        uses_contra_model, allows_short_hairpins, rows.data(), scores.data(), dp.data()));
  std::vector<MfeStructure> out(seqs.size());
  for (size_t s = 0; s < seqs.size(); s++) {
    out[s].dot_bracket.assign(reinterpret_cast<const char*>(rows.data() + off[s]), seqs[s].size());
    out[s].score = scores[s];
    out[s].dp_score = dp[s];
  }
  return out;
}
inline MfeStructure mfe_fold(const Context& ctx, const Seq& seq, bool uses_contra_model,
                             bool allows_short_hairpins) {
  return std::move(mfe_fold_batch(ctx, {seq}, uses_contra_model, allows_short_hairpins)[0]);
}

// CentroidFold<T>, src/centroid_fold.rs:4-7
template <class T>
struct CentroidFold {
  std::vector<PosPair<T>> basepair_pos_pairs;
  Score expect_accuracy = 0.f;
};

// centroid_fold, src/centroid_fold.rs:25-105
template <class T>
CentroidFold<T> centroid_fold(const SparseProbMat<T>& basepair_probs, size_t seq_len,
                              Prob centroid_threshold) {
  const uint32_t n = static_cast<uint32_t>(seq_len);
  std::vector<float> packed(rnamc_bpp_len(n), -1.0f);
  for (const auto& kv : basepair_probs)
    packed[rnamc_bpp_index(n, static_cast<uint32_t>(kv.first.first), static_cast<uint32_t>(kv.first.second))] = kv.second;
  std::vector<uint32_t> pairs(2 * (n / 2 + 1));
  uint32_t np = 0;
  CentroidFold<T> f;
  check(rnamc_centroid_fold(packed.data(), n, centroid_threshold, pairs.data(), n / 2 + 1, &np,
                            &f.expect_accuracy));
  for (uint32_t x = 0; x < np; x++)
    f.basepair_pos_pairs.emplace_back(static_cast<T>(pairs[2 * x]), static_cast<T>(pairs[2 * x + 1]));
  return f;
}

}  // namespace rna_algos

#endif
