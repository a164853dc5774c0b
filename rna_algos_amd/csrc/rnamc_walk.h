// rnamc_walk.h — the top-down walker of the inside grammar, shared by the Boltzmann sampler
// (rnamc_sample.hip) and the maximum-score traceback (rnamc_mfe.hip).  One wave walks one
// structure; the caller supplies the decision (which candidate of a cell is taken).
//
// Grammar (the reference's inside recurrences, src/mccaskill_algo.rs:282-378 / 380-516, walked
// top-down; DESIGN.md section 9 has the table).  A pending cell is one of
//   X(j)    sums_external[0][j]             (start: X(n-1); j < 0 ends)
//   E(k,j)  sums_rightmost_basepairs_external, rightmost pair (k, l) of the exterior
//   C(i,j)  sums_close: what the pair (i, j) closes
//   M(i,j)  sums_multibranch: >= 2 branches inside a multiloop
//   O(i,j)  sums_1ormore_basepairs: >= 1 branch inside a multiloop
//   R(k,j)  the multiloop's rightmost branch (k, l) (Turner: = E; CONTRAfold: the _multibranch sums)
// At every cell one candidate term is picked and the local loop score of that term
// (rnamc_scoring.h) is added to the structure's score.
//
// Pending cells live on a per-wave stack in global scratch (intervals on it are disjoint and
// non-empty, so depth <= n).  Every lane writes the same stack entries and marks: each lane reads
// back only what it wrote itself (program order), no fence needed.
#ifndef RNAMC_WALK_H
#define RNAMC_WALK_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "rnamc_device.h"
#include "rnamc_scoring.h"

namespace rnamc {
namespace walk {

enum Cell : uint32_t { CX = 0, CE = 1, CC = 2, CM = 3, CO = 4, CR = 5 };

__device__ __forceinline__ uint64_t enc(uint32_t type, uint32_t i, uint32_t j) {
  return (static_cast<uint64_t>(type) << 32) | (static_cast<uint64_t>(i) << 16) | j;
}

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

__device__ __forceinline__ uint64_t ballot64(bool p) { return static_cast<uint64_t>(__ballot(p)); }

constexpr int kCache = 8;  // register-held steps of 64 candidates

// The 2-loop candidates of C(i,j) in the reference's order (k ascending, l descending): a = k-i-1
// and b = j-l-1 over the triangle a + b <= L, L = min(30, j-i-3); row a starts at a(2L+3-a)/2.
__device__ __forceinline__ void twoloop_ab(uint32_t L, uint32_t t, uint32_t& a, uint32_t& b) {
  const int q = 2 * static_cast<int>(L) + 3;
  int x = static_cast<int>((static_cast<float>(q) -
                            sqrtf(static_cast<float>(q * q - 8 * static_cast<int>(t)))) * 0.5f);
  x = x < 0 ? 0 : (x > static_cast<int>(L) ? static_cast<int>(L) : x);
  auto row = [q](int y) { return y * (q - y) / 2; };
  while (x > 0 && row(x) > static_cast<int>(t)) x--;
  while (x < static_cast<int>(L) && row(x + 1) <= static_cast<int>(t)) x++;
  a = static_cast<uint32_t>(x);
  b = t - static_cast<uint32_t>(row(x));
}

template <bool CONTRA>
struct ModelOf;
template <>
struct ModelOf<false> {
  static __device__ __forceinline__ Turner make(const SampleBatch& a) {
    return Turner{a.params->turner, a.hp_init};
  }
};
template <>
struct ModelOf<true> {
  static __device__ __forceinline__ Contra make(const SampleBatch& a) {
    return Contra{a.params->contra};
  }
};

// Candidates of the cells, read from the inside matrices of one sequence (diag-major).
template <bool CONTRA>
struct Grammar {
  using Model = typename std::conditional<CONTRA, Contra, Turner>::type;
  Model M;
  const rnamc_params* P;
  const uint8_t* s;
  uint32_t n;
  const float *qb, *qa, *z, *q1, *zre, *qm, *zrm;

  __device__ __forceinline__ uint64_t tri(uint32_t i, uint32_t j) const {
    const uint64_t d = j - i;
    return d * n - d * (d - 1ull) / 2ull + i;
  }
  __device__ __forceinline__ uint32_t twoloop_L(uint32_t i, uint32_t j) const {
    return min(static_cast<uint32_t>(RNAMC_MAX_2LOOP_LEN), j - i - 3u);
  }
  // candidates of a cell
  __device__ __forceinline__ uint32_t count(uint32_t type, uint32_t i, uint32_t j) const {
    switch (type) {
      case CX: return j + 1u;
      case CE: case CR: return j - i;
      case CC: {
        if (j - i < 3u) return 2u;
        const uint32_t L = twoloop_L(i, j);
        return 2u + (L + 1u) * (L + 2u) / 2u;
      }
      case CM: return j - i - 1u;
      default: return j - i + 1u;  // CO
    }
  }
  // term of candidate x (the value the reference folded into the cell's sum)
  __device__ __forceinline__ float term(uint32_t type, uint32_t i, uint32_t j, uint32_t x) const {
    switch (type) {
      case CX:
        if (x == 0u)
          return CONTRA ? P->contra.external_score_unpair * static_cast<float>(j + 1u) : 0.f;
        return zre[tri(x - 1u, j)] + (x == 1u ? 0.f : z[tri(0u, x - 2u)]);
      case CE:
      case CR: {
        const uint32_t l = i + 1u + x;
        const float v = qa[tri(i, l)];
        if (!CONTRA) return v;
        const rnamc_fold_score_sets& f = P->contra;
        return type == CE ? v + f.external_score_basepair + f.external_score_unpair * static_cast<float>(j - l)
                          : v + f.multibranch_score_basepair +
                                f.multibranch_score_unpair * static_cast<float>(j - l);
      }
      case CC: {
        const uint32_t last = count(CC, i, j) - 1u;
        if (x == 0u) {
          if (CONTRA && j - i - 1u > RNAMC_MAX_LOOP_LEN) return kNegInf;
          return M.hairpin(s, n, i, j);
        }
        if (x == last) {
          if (j - i < 2u) return kNegInf;
          return qm[tri(i + 1u, j - 1u)] + M.mbclose(s, n, i, j);
        }
        uint32_t a, b;
        twoloop_ab(twoloop_L(i, j), x - 1u, a, b);
        const uint32_t k = i + 1u + a, l = j - 1u - b;
        const float v = qb[tri(k, l)];
        if (!(v > kNegInf)) return kNegInf;
        return v + M.twoloop(s, i, j, k, l);
      }
      case CM: {
        const uint32_t k = i + 1u + x;
        if (CONTRA) return q1[tri(i, k - 1u)] + zrm[tri(k, j)];
        return q1[tri(i, k - 1u)] + (zre[tri(k, j)] + P->turner.coeff_num_branches);
      }
      default: {  // CO
        if (x == j - i) return qm[tri(i, j)];
        const uint32_t k = i + x;
        if (CONTRA)
          return x == 0u ? zrm[tri(i, j)]
                         : zrm[tri(k, j)] + P->contra.multibranch_score_unpair * static_cast<float>(x);
        return zre[tri(k, j)] + P->turner.coeff_num_branches;
      }
    }
  }
};

// The grammar of descriptor sd, over the matrices of its workspace.
template <bool CONTRA>
__device__ __forceinline__ Grammar<CONTRA> grammar_of(const SampleBatch& a, const SeqDesc& sd) {
  Grammar<CONTRA> sm{ModelOf<CONTRA>::make(a), a.params, a.bases + sd.seq_off, sd.n};
  const float* base = a.workspace + sd.ws_off;
  sm.qb = base + static_cast<uint64_t>(M_QB) * sd.tri_pad;
  sm.qa = base + static_cast<uint64_t>(M_QA) * sd.tri_pad;
  sm.z = base + static_cast<uint64_t>(M_Z) * sd.tri_pad;
  sm.q1 = base + static_cast<uint64_t>(M_Q1D) * sd.tri_pad;
  sm.zre = base + static_cast<uint64_t>(M_ZRE) * sd.tri_pad;
  sm.qm = base + static_cast<uint64_t>(M_QM) * sd.tri_pad;
  sm.zrm = base + static_cast<uint64_t>(M_ZRM) * sd.tri_pad;
  return sm;
}

// Walk one structure of the sequence into row (n bytes '(' ')' '.').  pick(type, i, j, cnt,
// decision index) returns the candidate taken, or -1 when there is none.  Returns the f32 sum of
// the local scores, or NaN when the walk failed (stack overflow, no candidate, runaway).
template <bool CONTRA, class Pick>
__device__ __forceinline__ float walk_structure(const Grammar<CONTRA>& sm, uint8_t* row, uint64_t* stack,
                                                uint32_t stack_cap, uint32_t lane, Pick&& pick) {
  const uint32_t n = sm.n;
  const rnamc_params* P = sm.P;
  for (uint32_t p = lane; p < n; p += 64u) row[p] = '.';
  float lw = 0.f;
  uint32_t sp = 0, dec = 0;
  bool bad = false;
  auto push = [&](uint32_t type, uint32_t i, uint32_t j) {
    if (sp >= stack_cap) {
      bad = true;
      return;
    }
    stack[sp++] = enc(type, i, j);
  };
  auto mark = [&](uint32_t i, uint32_t j) {
    row[i] = '(';
    row[j] = ')';
  };
  push(CX, 0u, n - 1u);
  const uint32_t max_dec = 4u * n + 16u;  // every decision ends a cell of a disjoint interval
  while (sp > 0 && !bad) {
    const uint64_t e = stack[--sp];
    const uint32_t type = static_cast<uint32_t>(e >> 32);
    const uint32_t i = static_cast<uint32_t>(e >> 16) & 0xFFFFu, j = static_cast<uint32_t>(e) & 0xFFFFu;
    if (dec >= max_dec) {
      bad = true;
      break;
    }
    const uint32_t cnt = sm.count(type, i, j);
    const int c = pick(type, i, j, cnt, dec++);
    if (c < 0) {
      bad = true;
      break;
    }
    const uint32_t y = static_cast<uint32_t>(c);
    switch (type) {
      case CX:
        if (y == 0u) {
          if (CONTRA) lw += P->contra.external_score_unpair * static_cast<float>(j + 1u);
        } else {
          const uint32_t k = y - 1u;
          if (k >= 1u) push(CX, 0u, k - 1u);
          push(CE, k, j);
        }
        break;
      case CE:
      case CR: {
        const uint32_t l = i + 1u + y;
        float sc = sm.M.accessible(sm.s, n, i, l);
        if (CONTRA) {
          const rnamc_fold_score_sets& f = P->contra;
          sc = type == CE ? sc + f.external_score_basepair + f.external_score_unpair * static_cast<float>(j - l)
                          : sc + f.multibranch_score_basepair +
                                f.multibranch_score_unpair * static_cast<float>(j - l);
        }
        lw += sc;
        mark(i, l);
        push(CC, i, l);
        break;
      }
      case CC:
        if (y == 0u) {
          lw += sm.M.hairpin(sm.s, n, i, j);
        } else if (y == cnt - 1u) {
          lw += sm.M.mbclose(sm.s, n, i, j);
          push(CM, i + 1u, j - 1u);
        } else {
          uint32_t aa, bb;
          twoloop_ab(sm.twoloop_L(i, j), y - 1u, aa, bb);
          const uint32_t k = i + 1u + aa, l = j - 1u - bb;
          lw += sm.M.twoloop(sm.s, i, j, k, l);
          mark(k, l);
          push(CC, k, l);
        }
        break;
      case CM: {
        const uint32_t k = i + 1u + y;
        if (!CONTRA) lw += P->turner.coeff_num_branches;
        push(CO, i, k - 1u);
        push(CR, k, j);
        break;
      }
      default:  // CO
        if (y == j - i) {
          push(CM, i, j);
        } else {
          if (CONTRA) {
            if (y > 0u) lw += P->contra.multibranch_score_unpair * static_cast<float>(y);
          } else {
            lw += P->turner.coeff_num_branches;
          }
          push(CR, i + y, j);
        }
        break;
    }
  }
  return bad ? __builtin_nanf("") : lw;
}

}  // namespace walk
}  // namespace rnamc

#endif
