// rnamc_mfe.hip — maximum-score structure (MFE under Turner, the Viterbi parse under CONTRAfold):
// the inside recurrences in the (max, +) semiring, then an argmax traceback with the sampler's
// walker (rnamc_walk.h).  DESIGN.md section 10.
//
// Sweep: one launch per anti-diagonal d over all sequences of a group, one lane per cell (i, j),
// lanes of a wave on consecutive i.  Every operand of a cell lies on a lower diagonal or in the
// same cell, so within the lane:
//   QM(i,j) = max_{k=i+1..j-1} Q1(i,k-1) + R(k,j)   R = ZRE + C (Turner) | ZRM (CONTRAfold)
//   ZRE(i,j) = max(ZRE(i,j-1) [+ ext_unpair], QA(i,j) [+ ext_bp])      (ZRM alike, multibranch)
//   U(i,j)   = max(U(i+1,j) [+ mb_unpair], ZRE(i,j) + C [ZRM(i,j)])    column prefix, slot M_W
//   Q1(i,j)  = max(U(i,j), QM(i,j))
//   Z(0,j)   = max(all unpaired, max_k ZRE(k,j) + Z(0,k-1))            the wave of cell (0, d)
// (the prefix forms hold in any semiring: the terms of ZRE(i,j) are those of ZRE(i,j-1) plus one
// unpaired base, those of U(i,j) those of U(i+1,j) plus one).  QM is the only cubic term: at every
// step t = k - i the lanes read Q1 of diagonal t-1 and R of diagonal d-t at consecutive floats.
// The closing-pair cells C(i,j) (hairpin, the <= 496 2-loops, QM(i+1,j-1) + mbclose) need only
// diagonals <= d-2: the launch of diagonal d holds those of diagonal d+1, a lane per cell of
// k_compact's canonical lists, beside the sums of diagonal d.  QA = C + accessible.
//
// Max is exact, so a cell's value does not depend on the order of its candidates; the prefix
// forms under CONTRAfold round differently from the candidate expressions (one unpaired term at a
// time), which the traceback never relies on: it recomputes each candidate from the stored
// matrices, takes the wave maximum and picks the first candidate equal to it.
//
// Plain vector loads and stores only; -ffp-contract=off, no fast-math (-inf is data).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rnamc_device.h"
#include "rnamc_scoring.h"
#include "rnamc_walk.h"

namespace rnamc {
namespace {

using namespace walk;

// v_max_f32 without the sNaN-quieting canonicalisation hipcc adds in front of fmaxf (operands
// here are finite or -inf, never NaN)
__device__ __forceinline__ float vmax(float a, float b) {
  float r;
  asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

constexpr uint32_t kU = 16;  // QM steps whose loads are in flight together
constexpr uint32_t kB = 8;   // 2-loop candidates evaluated together

__device__ __forceinline__ uint32_t tri_off(uint32_t n, uint32_t d) {  // start of diagonal d
  return d * n - (d * (d - 1u)) / 2u;
}

template <bool CONTRA>
struct ModelOfB;
template <>
struct ModelOfB<false> {
  static __device__ __forceinline__ Turner make(const DeviceBatch& b) {
    return Turner{b.params->turner, b.hp_init};
  }
};
template <>
struct ModelOfB<true> {
  static __device__ __forceinline__ Contra make(const DeviceBatch& b) {
    return Contra{b.params->contra};
  }
};

// The sums of cell (i, i+d): QM, ZRE (ZRM), U, Q1, and Z(0,d) by the wave that holds i = 0.
template <bool CONTRA>
__device__ __forceinline__ void mfe_sums(const DeviceBatch& b, uint32_t seq, uint32_t part, uint32_t d) {
  const SeqDesc sd = b.seqs[seq];
  const uint32_t n = sd.n;
  if (d >= n) return;
  const uint32_t cells = n - d;
  const uint32_t tid = threadIdx.x, lane = tid & 63u;
  const uint32_t i0 = __builtin_amdgcn_readfirstlane(part * blockDim.x + (tid & ~63u));
  if (i0 >= cells) return;  // (wave-uniform)
  const uint32_t i = i0 + lane;
  const bool valid = i < cells;
  const uint32_t ic = valid ? i : cells - 1u;  // lanes past the diagonal compute a copy, store nothing
  float* base = b.workspace + sd.ws_off;
  const uint64_t tp = sd.tri_pad;
  float* __restrict__ q1 = base + M_Q1D * tp;
  float* __restrict__ zre = base + M_ZRE * tp;
  float* __restrict__ zrm = base + M_ZRM * tp;
  float* __restrict__ qm = base + M_QM * tp;
  float* __restrict__ uu = base + M_W * tp;
  float* __restrict__ z = base + M_Z * tp;
  const float* __restrict__ qa = base + M_QA * tp;
  const float C = b.params->turner.coeff_num_branches;
  const float* __restrict__ r = CONTRA ? zrm : zre;

  // QM: t = k - i = 1 .. d-1; Q1(i,k-1) on diagonal t-1, R(k,j) on diagonal d-t.  The loads of
  // kU steps are issued before their maxima, so that kU pairs of loads are in flight at a time.
  float m = kNegInf;
  const uint32_t steps = d >= 1u ? d - 1u : 0u;
  auto term = [&](float a, float x) { return CONTRA ? a + x : a + (x + C); };
  uint32_t t = 1;
  for (; t + kU <= steps + 1u; t += kU) {
    float a[kU], x[kU];
#pragma unroll
    for (uint32_t w = 0; w < kU; w++) {
      a[w] = q1[tri_off(n, t + w - 1u) + ic];
      x[w] = r[tri_off(n, d - t - w) + ic + t + w];
    }
#pragma unroll
    for (uint32_t w = 0; w < kU; w++) m = vmax(m, term(a[w], x[w]));
  }
  for (; t <= steps; t++) m = vmax(m, term(q1[tri_off(n, t - 1u) + ic], r[tri_off(n, d - t) + ic + t]));
  const uint32_t od = tri_off(n, d) + ic;
  const float va = qa[od];
  float zr_ext, zr_mb, u;
  if (!CONTRA) {
    const float zp = d >= 1u ? zre[tri_off(n, d - 1u) + ic] : kNegInf;
    const float up = d >= 1u ? uu[tri_off(n, d - 1u) + ic + 1u] : kNegInf;
    zr_ext = vmax(zp, va);
    zr_mb = zr_ext;
    u = vmax(up, zr_ext + C);
  } else {
    const rnamc_fold_score_sets& f = b.params->contra;
    const float eun = f.external_score_unpair, mun = f.multibranch_score_unpair;
    const uint32_t op = d >= 1u ? tri_off(n, d - 1u) + ic : 0u;
    const float zp = d >= 1u ? zre[op] : kNegInf;
    const float zmp = d >= 1u ? zrm[op] : kNegInf;
    const float up = d >= 1u ? uu[op + 1u] : kNegInf;
    zr_ext = vmax(zp + eun, va + f.external_score_basepair);
    zr_mb = vmax(zmp + mun, va + f.multibranch_score_basepair);
    u = vmax(up + mun, zr_mb);
  }
  if (valid) {
    qm[od] = m;
    zre[od] = zr_ext;
    if (CONTRA) zrm[od] = zr_mb;
    uu[od] = u;
    q1[od] = vmax(u, m);
  }
  if (i0 == 0u) {
    // Z(0,d): candidate k = 0 is lane 0's own ZRE(0,d); k >= 1 read lower diagonals
    float e = lane == 0u ? zr_ext + 0.f : kNegInf;
    for (uint32_t k = 1u + lane; k < d; k += 64u) e = vmax(e, zre[tri_off(n, d - k) + k] + z[tri_off(n, k - 1u)]);
    e = wave_max(e);
    const float unp = CONTRA ? b.params->contra.external_score_unpair * static_cast<float>(d + 1u) : 0.f;
    if (lane == 0u) z[tri_off(n, d)] = vmax(unp, e);
  }
}

// The closing-pair cell of listed entry t of diagonal d: C = QB and QA.
template <bool CONTRA>
__device__ __forceinline__ void mfe_pair(const DeviceBatch& b, uint32_t seq, uint32_t part, uint32_t d) {
  const SeqDesc sd = b.seqs[seq];
  const uint32_t n = sd.n;
  if (d >= n) return;
  if (!(b.allows_short_hairpins && CONTRA) && d + 1u < RNAMC_MIN_SPAN_HAIRPIN_CLOSE) return;
  const uint32_t* ccnt = reinterpret_cast<const uint32_t*>(b.workspace + sd.ccnt_off);
  const uint16_t* cidx = reinterpret_cast<const uint16_t*>(b.workspace + sd.cidx_off) + tri_off(n, d);
  const uint32_t cnt = ccnt[d];
  const uint32_t tid = threadIdx.x;
  const uint32_t t0 = __builtin_amdgcn_readfirstlane(part * blockDim.x + (tid & ~63u));
  if (t0 >= cnt) return;  // (wave-uniform)
  const uint32_t t = t0 + (tid & 63u);
  const uint32_t i = cidx[t < cnt ? t : t0];
  const uint32_t j = i + d;
  // a pair the constraint forbids is treated like one below the minimum span: lanes hold different
  // cells, so it joins the lane's flag (b.cons is uniform)
  const bool valid = t < cnt && (!b.cons || pair_allowed(b.cons + 2 * sd.seq_off, b.max_span, i, j));
  float* base = b.workspace + sd.ws_off;
  const uint64_t tp = sd.tri_pad;
  float* __restrict__ qb = base + M_QB * tp;
  float* __restrict__ qa = base + M_QA * tp;
  const float* __restrict__ qm = base + M_QM * tp;
  const uint8_t* s = b.bases + sd.seq_off;
  const auto M = ModelOfB<CONTRA>::make(b);
  float best = kNegInf;
  if (!CONTRA || d - 1u <= RNAMC_MAX_LOOP_LEN) best = M.hairpin(s, n, i, j);
  if (d >= 3u) {
    // enclosed pairs (k, l) = (i+1+a, j-1-bb), a + bb <= L: diagonal d-2-a-bb
    const uint32_t L = min(static_cast<uint32_t>(RNAMC_MAX_2LOOP_LEN), d - 3u);
    // kB candidates of a row at a time, evaluated unconditionally (lanes past the row's end
    // evaluate l = j-1 and are masked): their loads are issued together
    for (uint32_t a = 0; a <= L; a++) {
      const uint32_t k = i + 1u + a;
      for (uint32_t b0 = 0; b0 + a <= L; b0 += kB) {
        float v[kB];
#pragma unroll
        for (uint32_t w = 0; w < kB; w++) {
          const bool in = b0 + w + a <= L;
          const uint32_t l = j - 1u - (in ? b0 + w : 0u);
          const float x = qb[tri_off(n, l - k) + k] + M.twoloop(s, i, j, k, l);
          v[w] = in ? x : kNegInf;
        }
#pragma unroll
        for (uint32_t w = 0; w < kB; w++) best = vmax(best, v[w]);
      }
    }
  }
  if (d >= 2u) best = vmax(best, qm[tri_off(n, d - 2u) + i + 1u] + M.mbclose(s, n, i, j));
  if (valid && best > kNegInf) {
    const uint32_t o = tri_off(n, d) + i;
    qb[o] = best;
    qa[o] = best + M.accessible(s, n, i, j);
  }
}

// blocks [0, bs * ns): sums of diagonal d_s, sequence = block % ns; the rest: closing-pair cells
// of diagonal d_p, bp blocks per sequence over np sequences
template <bool CONTRA>
__global__ void __launch_bounds__(256) k_mfe(DeviceBatch b, uint32_t d_s, uint32_t d_p, uint32_t bs,
                                             uint32_t ns, uint32_t np) {
  const uint32_t blk = blockIdx.x;
  if (blk < bs * ns) {
    mfe_sums<CONTRA>(b, blk % ns, blk / ns, d_s);
  } else {
    const uint32_t r = blk - bs * ns;
    mfe_pair<CONTRA>(b, r % np, r / np, d_p);
  }
}

// argmax decision: pass 0 the wave maximum of the terms, pass 2 the first candidate equal to it;
// -1 when every term is -inf
template <class S>
__device__ int decide_max(const S& sm, uint32_t type, uint32_t i, uint32_t j, uint32_t cnt, uint32_t lane) {
  const uint32_t steps = (cnt + 63u) / 64u;
  auto val = [&](uint32_t st) {
    const uint32_t x = st * 64u + lane;
    return x < cnt ? sm.term(type, i, j, x) : kNegInf;
  };
  float cache[kCache];
  const bool cached = steps <= static_cast<uint32_t>(kCache);
  float mx = kNegInf;
  for (uint32_t st = 0; st < steps; st++) {
    const float v = val(st);
    mx = fmaxf(mx, v);
#pragma unroll
    for (int q = 0; q < kCache; q++)
      if (static_cast<uint32_t>(q) == st) cache[q] = v;
  }
  mx = wave_max(mx);
  if (!(mx > kNegInf)) return -1;
  int pick = -1;
  auto step_pick = [&](uint32_t st, float v) {
    const uint64_t hit = ballot64(v == mx);
    if (hit) pick = static_cast<int>(st * 64u + static_cast<uint32_t>(__ffsll(static_cast<long long>(hit)) - 1));
  };
  if (cached) {
#pragma unroll
    for (int st = 0; st < kCache; st++)
      if (pick < 0 && static_cast<uint32_t>(st) < steps) step_pick(st, cache[st]);
  } else {
    for (uint32_t st = 0; st < steps && pick < 0; st++) step_pick(st, val(st));
  }
  return pick;
}

template <bool CONTRA>
__global__ void __launch_bounds__(256) k_mfe_trace(SampleBatch a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u;
  const uint32_t n_waves = gridDim.x * (blockDim.x / 64u);
  uint64_t* stack = a.stack + static_cast<uint64_t>(wave) * a.stack_cap;
  for (uint32_t x = wave; x < a.nseq; x += n_waves) {
    const SeqDesc sd = a.seqs[x];
    const Grammar<CONTRA> sm = grammar_of<CONTRA>(a, sd);
    const float sc = walk_structure<CONTRA>(
        sm, a.rows + a.row_off[x], stack, a.stack_cap, lane,
        [&](uint32_t type, uint32_t i, uint32_t j, uint32_t cnt, uint32_t) {
          return decide_max(sm, type, i, j, cnt, lane);
        });
    if (lane == 0) {
      a.log_weights[x] = sc;
      if (a.dp_scores) a.dp_scores[x] = sm.z[sm.tri(0u, sd.n - 1u)];
    }
  }
}

}  // namespace

void launch_mfe_inside(const DeviceBatch& b, bool contra, uint32_t d_sums, uint32_t d_pair,
                       uint32_t max_n, uint32_t nseq, hipStream_t st) {
  // sequences active on a diagonal are a prefix of the group (longest first): the blocks of the
  // others exit at once, so ns = np = nseq is enough
  constexpr uint32_t kBlock = 256;
  const uint32_t bs = d_sums < max_n ? (max_n - d_sums + kBlock - 1) / kBlock : 0u;
  const uint32_t bp = d_pair < max_n ? (max_n - d_pair + kBlock - 1) / kBlock : 0u;
  if (nseq == 0 || bs + bp == 0) return;
  const dim3 g((bs + bp) * nseq);
  if (contra)
    hipLaunchKernelGGL(k_mfe<true>, g, dim3(kBlock), 0, st, b, d_sums, d_pair, bs, nseq, nseq);
  else
    hipLaunchKernelGGL(k_mfe<false>, g, dim3(kBlock), 0, st, b, d_sums, d_pair, bs, nseq, nseq);
}

void launch_mfe_trace(const SampleBatch& a, bool contra, uint32_t n_waves, hipStream_t st) {
  const uint32_t blocks = (n_waves + 3u) / 4u;
  if (contra)
    hipLaunchKernelGGL(k_mfe_trace<true>, dim3(blocks), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(k_mfe_trace<false>, dim3(blocks), dim3(256), 0, st, a);
}

}  // namespace rnamc
