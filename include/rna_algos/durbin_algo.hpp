// rna_algos/durbin_algo.hpp — C++ host-side mirror of the reference crate's `durbin_algo`
// module over the C ABI of librnamc.so (include/rnamc.h).  Header-only, C++17.
// Reference items mirrored:
//   src/durbin_algo.rs:4-14    pub struct AlignScores { ... }
//   src/durbin_algo.rs:25-58   impl AlignScores { new, transfer }
//   src/durbin_algo.rs:73-77   pub fn durbin_algo(seq_pair, align_scores) -> ProbMat
//   src/utils.rs:83,122        ProbMat, PSEUDO_BASE
// Sequences carry PSEUDO_BASE at both ends, as the reference's callers build them
// (tests/tests.rs:53-55).
#ifndef RNA_ALGOS_DURBIN_ALGO_HPP
#define RNA_ALGOS_DURBIN_ALGO_HPP

#include <utility>
#include <vector>

#include "mccaskill_algo.hpp"

namespace rna_algos {

constexpr Base PSEUDO_BASE = 4;  // U + 1, src/utils.rs:122
using Probs = std::vector<Prob>;
using ProbMat = std::vector<Probs>;
using SeqPair = std::pair<const Seq*, const Seq*>;

// AlignScores: the C struct has the reference's fields under their own names
struct AlignScores : rnamc_align_scores {
  explicit AlignScores(Score init_val = 0.f) { check(rnamc_align_scores_new(init_val, this)); }
  static AlignScores new_(Score init_val) { return AlignScores(init_val); }
  void transfer() { check(rnamc_align_scores_transfer(this)); }
};

// every pair of `pairs` (indices into `seqs`) in one device batch: what
// src/bin/durbin_algo.rs:55-75 does with one pool task per pair
inline std::vector<ProbMat> durbin_algo_batch(const Context& ctx, const std::vector<Seq>& seqs,
                                              const std::vector<std::pair<size_t, size_t>>& pairs,
                                              const AlignScores& align_scores) {
  std::vector<uint8_t> bases;
  std::vector<uint64_t> offsets{0}, out_offsets{0};
  for (const Seq& s : seqs) {
    bases.insert(bases.end(), s.begin(), s.end());
    offsets.push_back(bases.size());
  }
  std::vector<uint32_t> pa, pb;
  for (const auto& p : pairs) {
    pa.push_back(static_cast<uint32_t>(p.first));
    pb.push_back(static_cast<uint32_t>(p.second));
    out_offsets.push_back(out_offsets.back() + seqs[p.first].size() * seqs[p.second].size());
  }
  std::vector<float> flat(out_offsets.back() ? out_offsets.back() : 1);
  check(rnamc_durbin_batch(ctx.get(), &align_scores, static_cast<uint32_t>(seqs.size()), bases.data(),
                           offsets.data(), static_cast<uint32_t>(pairs.size()), pa.data(), pb.data(),
                           flat.data(), out_offsets.data()));
  std::vector<ProbMat> out;
  for (size_t x = 0; x < pairs.size(); x++) {
    const size_t n1 = seqs[pairs[x].first].size(), n2 = seqs[pairs[x].second].size();
    ProbMat m(n1, Probs(n2));
    for (size_t i = 0; i < n1; i++)
      for (size_t j = 0; j < n2; j++) m[i][j] = flat[out_offsets[x] + i * n2 + j];
    out.push_back(std::move(m));
  }
  return out;
}

// durbin_algo, src/durbin_algo.rs:73-77
inline ProbMat durbin_algo(const Context& ctx, const SeqPair& seq_pair, const AlignScores& align_scores) {
  return durbin_algo_batch(ctx, {*seq_pair.first, *seq_pair.second}, {{0, 1}}, align_scores)[0];
}

// ---- pairwise alignment off the match probabilities (include/rnamc.h: rnamc_match_align,
// rnamc_match_align_mats, rnamc_durbin_align_batch).  Indices are ProbMat coordinates.

// the gamma-centroid alignment of one ProbMat on the host: rnamc_match_align
struct MatchAlignment {
  std::vector<int> mate;  // per row of the ProbMat: its matched column, or -1
  uint32_t n_matched = 0;
  float expect_accuracy = 0.f;
};
inline MatchAlignment match_align(const ProbMat& probs, float gamma) {
  const size_t n1 = probs.size(), n2 = n1 ? probs[0].size() : 0;
  std::vector<float> flat;
  for (const Probs& row : probs) flat.insert(flat.end(), row.begin(), row.end());
  MatchAlignment out;
  out.mate.resize(n1);
  check(rnamc_match_align(flat.data(), static_cast<uint32_t>(n1), static_cast<uint32_t>(n2), gamma,
                          out.mate.data(), &out.n_matched, &out.expect_accuracy));
  return out;
}

// what the device stage makes of one pair: the listed cells (p > 0 and p >= min_prob, row-major),
// the per-base marginals, one alignment per gamma
struct PairAlignment {
  std::vector<uint32_t> i, j;
  Probs p, row_matched, col_matched;
  std::vector<MatchAlignment> alignments;
};

namespace detail {
// the output arguments both entries end on, and how a pair's results are cut out of them
struct MatchOutputs {
  std::vector<uint32_t> mi, mj, n_matched;
  Probs mp, accuracy, matched;
  std::vector<int> mate;
  std::vector<uint64_t> start, count, mate_off{0}, marg_off{0};
  uint64_t total = 0;
  size_t ng;
  MatchOutputs(const std::vector<std::pair<size_t, size_t>>& shapes, size_t n_gammas)
      : start(shapes.size()), count(shapes.size()), ng(n_gammas) {
    for (const auto& s : shapes) {
      mate_off.push_back(mate_off.back() + ng * s.first);
      marg_off.push_back(marg_off.back() + s.first + s.second);
    }
    mate.resize(mate_off.back() + 1);
    matched.resize(marg_off.back() + 1);
    n_matched.resize(shapes.size() * ng + 1);
    accuracy.resize(shapes.size() * ng + 1);
  }
  void room(uint64_t cap) {
    mi.resize(cap + 1);
    mj.resize(cap + 1);
    mp.resize(cap + 1);
  }
  PairAlignment cut(size_t x, size_t n1, size_t n2) const {
    PairAlignment r;
    r.i.assign(mi.begin() + start[x], mi.begin() + start[x] + count[x]);
    r.j.assign(mj.begin() + start[x], mj.begin() + start[x] + count[x]);
    r.p.assign(mp.begin() + start[x], mp.begin() + start[x] + count[x]);
    r.row_matched.assign(matched.begin() + marg_off[x], matched.begin() + marg_off[x] + n1);
    r.col_matched.assign(matched.begin() + marg_off[x] + n1, matched.begin() + marg_off[x + 1]);
    for (size_t g = 0; g < ng; g++) {
      MatchAlignment a;
      a.mate.assign(mate.begin() + mate_off[x] + g * n1, mate.begin() + mate_off[x] + (g + 1) * n1);
      a.n_matched = n_matched[x * ng + g];
      a.expect_accuracy = accuracy[x * ng + g];
      r.alignments.push_back(std::move(a));
    }
    return r;
  }
};
}  // namespace detail

// rnamc_durbin_align_batch: the pair-HMM of durbin_algo_batch, then the stage off the device-resident
// ProbMats; no dense matrix reaches the host.  A first call counts, the second has room.
inline std::vector<PairAlignment> pair_align_batch(const Context& ctx, const std::vector<Seq>& seqs,
                                                   const std::vector<std::pair<size_t, size_t>>& pairs,
                                                   const AlignScores& align_scores, const std::vector<float>& gammas,
                                                   float min_prob) {
  std::vector<uint8_t> bases;
  std::vector<uint64_t> offsets{0};
  for (const Seq& s : seqs) {
    bases.insert(bases.end(), s.begin(), s.end());
    offsets.push_back(bases.size());
  }
  std::vector<uint32_t> pa, pb;
  std::vector<std::pair<size_t, size_t>> shapes;
  for (const auto& p : pairs) {
    pa.push_back(static_cast<uint32_t>(p.first));
    pb.push_back(static_cast<uint32_t>(p.second));
    shapes.emplace_back(seqs[p.first].size(), seqs[p.second].size());
  }
  detail::MatchOutputs o(shapes, gammas.size());
  auto call = [&](bool lists, uint64_t cap) {
    return rnamc_durbin_align_batch(
        ctx.get(), &align_scores, static_cast<uint32_t>(seqs.size()), bases.data(), offsets.data(),
        static_cast<uint32_t>(pairs.size()), pa.data(), pb.data(), min_prob, gammas.data(),
        static_cast<uint32_t>(gammas.size()), lists ? o.mi.data() : nullptr, lists ? o.mj.data() : nullptr,
        lists ? o.mp.data() : nullptr, cap, o.start.data(), o.count.data(), &o.total, o.mate.data(),
        o.mate_off.data(), o.n_matched.data(), o.accuracy.data(), o.matched.data(), o.marg_off.data(), nullptr,
        nullptr);
  };
  check(call(false, 0));
  o.room(o.total);
  check(call(true, o.total));
  std::vector<PairAlignment> out;
  for (size_t x = 0; x < pairs.size(); x++) out.push_back(o.cut(x, shapes[x].first, shapes[x].second));
  return out;
}

// rnamc_match_align_mats: the same stage over the caller's dense matrices
inline std::vector<PairAlignment> match_align_mats(const Context& ctx, const std::vector<ProbMat>& mats,
                                                   const std::vector<float>& gammas, float min_prob) {
  std::vector<uint32_t> n1, n2;
  std::vector<uint64_t> offs{0};
  std::vector<float> flat;
  std::vector<std::pair<size_t, size_t>> shapes;
  for (const ProbMat& m : mats) {
    shapes.emplace_back(m.size(), m.empty() ? 0 : m[0].size());
    n1.push_back(static_cast<uint32_t>(shapes.back().first));
    n2.push_back(static_cast<uint32_t>(shapes.back().second));
    for (const Probs& row : m) flat.insert(flat.end(), row.begin(), row.end());
    offs.push_back(flat.size());
  }
  detail::MatchOutputs o(shapes, gammas.size());
  auto call = [&](bool lists, uint64_t cap) {
    return rnamc_match_align_mats(ctx.get(), static_cast<uint32_t>(mats.size()), n1.data(), n2.data(), flat.data(),
                                  offs.data(), min_prob, gammas.data(), static_cast<uint32_t>(gammas.size()),
                                  lists ? o.mi.data() : nullptr, lists ? o.mj.data() : nullptr,
                                  lists ? o.mp.data() : nullptr, cap, o.start.data(), o.count.data(), &o.total,
                                  o.mate.data(), o.mate_off.data(), o.n_matched.data(), o.accuracy.data(),
                                  o.matched.data(), o.marg_off.data());
  };
  check(call(false, 0));
  o.room(o.total);
  check(call(true, o.total));
  std::vector<PairAlignment> out;
  for (size_t x = 0; x < mats.size(); x++) out.push_back(o.cut(x, shapes[x].first, shapes[x].second));
  return out;
}

}  // namespace rna_algos

#endif
