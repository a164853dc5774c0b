// rnamc_sample.hip — Boltzmann sampling of secondary structures: the stochastic traceback
// (Ding & Lawrence) of the reference-order inside sweep that run_batch leaves in a group's
// workspace (the matrices of rnamc_internal.h, read in place).
//
// Grammar and walker: rnamc_walk.h (DESIGN.md section 9 has the table).  At every cell one
// term of the sum that produced it is picked, with weight exp(term - max)
// normalised over the terms themselves (the reference's fold is approximate: a stored sum is not
// exactly the sum of its parts), and the local loop score of that term (rnamc_scoring.h) is added
// to the sample's log-weight.
//
// Randomness: Philox4x32-10, key = seed, counter = (decision index, sample t, batch index s, 0);
// u = (word 0 >> 8) * 2^-24.  A sample is a pure function of tables, sequence, flags, seed, s
// and t — not of grouping, neighbours, knobs or device.
//
// Decision rule (bit-reproducible): candidates in a fixed order, 64 per wave step.  Pass 0: max.
// Pass 1: total = sum of exp(term - max), as a running sum of per-step inclusive wave scans.
// Pass 2: the first candidate of nonzero weight whose inclusive prefix (the same sums) exceeds
// u * total; if rounding leaves none, the last candidate with nonzero weight.  Decisions of at most 512
// candidates (every C cell: <= 498) keep their terms in registers; longer ones re-evaluate.
//
// Layout: one wave per (sequence, sample) pair, a grid-stride loop over the group's pairs; the
// pending cells live on a per-wave stack in global scratch (rnamc_walk.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <type_traits>

#include "rnamc_device.h"
#include "rnamc_scoring.h"
#include "rnamc_walk.h"

namespace rnamc {

// Philox4x32-10 (Salmon et al., SC'11), one 4-word block per decision.
RNAMC_HD uint32_t philox_u32(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
  uint32_t k0 = static_cast<uint32_t>(seed), k1 = static_cast<uint32_t>(seed >> 32);
  for (int r = 0; r < 10; r++) {
    const uint64_t p0 = static_cast<uint64_t>(0xD2511F53u) * c0;
    const uint64_t p1 = static_cast<uint64_t>(0xCD9E8D57u) * c2;
    const uint32_t h0 = static_cast<uint32_t>(p0 >> 32), l0 = static_cast<uint32_t>(p0);
    const uint32_t h1 = static_cast<uint32_t>(p1 >> 32), l1 = static_cast<uint32_t>(p1);
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

namespace {

using namespace walk;

__device__ __forceinline__ float wave_scan(float v, uint32_t lane) {  // inclusive, fixed order
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float y = __shfl_up(v, o, 64);
    if (lane >= static_cast<uint32_t>(o)) v += y;
  }
  return v;
}

// One decision; returns the chosen candidate, or -1 when every term is -inf.
template <class S>
__device__ int decide(const S& sm, uint32_t type, uint32_t i, uint32_t j, uint32_t cnt, float u,
                      uint32_t lane) {
  const uint32_t steps = (cnt + 63u) / 64u;
  auto val = [&](uint32_t st) {
    const uint32_t x = st * 64u + lane;
    return x < cnt ? sm.term(type, i, j, x) : kNegInf;
  };
  float cache[kCache];
  const bool cached = steps <= static_cast<uint32_t>(kCache);
  float mx = kNegInf;
  for (uint32_t st = 0; st < steps; st++) {  // (one evaluation site: terms are inlined once)
    const float v = val(st);
    mx = fmaxf(mx, v);
#pragma unroll
    for (int q = 0; q < kCache; q++)
      if (static_cast<uint32_t>(q) == st) cache[q] = v;
  }
  mx = wave_max(mx);
  if (!(mx > kNegInf)) return -1;
  auto weight = [&](float v) { return v > kNegInf ? expf(v - mx) : 0.f; };
  // pass 1: total and the last candidate with nonzero weight
  float run = 0.f;
  int last = -1;
  auto step_total = [&](uint32_t st, float v) {
    const float w = weight(v);
    const float p = wave_scan(w, lane);
    const uint64_t nz = ballot64(w > 0.f);
    if (nz) last = static_cast<int>(st * 64u + 63u - static_cast<uint32_t>(__clzll(nz)));
    run += __shfl(p, 63, 64);
  };
  if (cached) {
#pragma unroll
    for (int st = 0; st < kCache; st++)
      if (static_cast<uint32_t>(st) < steps) step_total(st, cache[st]);
  } else {
    for (uint32_t st = 0; st < steps; st++) step_total(st, val(st));
  }
  const float target = u * run;
  // pass 2: first inclusive prefix above the target.  The scan's prefixes are sums in different
  // orders and need not be monotone in f32: a candidate of weight 0 (a -inf term) can round above
  // its predecessor and above a target that lies between them, so only nonzero weights may hit.
  float run2 = 0.f;
  int pick = -1;
  auto step_pick = [&](uint32_t st, float v) {
    const float w = weight(v);
    const float p = run2 + wave_scan(w, lane);
    const uint64_t hit = ballot64(p > target && w > 0.f);
    if (hit) pick = static_cast<int>(st * 64u + static_cast<uint32_t>(__ffsll(static_cast<long long>(hit)) - 1));
    run2 = __shfl(p, 63, 64);
  };
  if (cached) {
#pragma unroll
    for (int st = 0; st < kCache; st++)
      if (pick < 0 && static_cast<uint32_t>(st) < steps) step_pick(st, cache[st]);
  } else {
    for (uint32_t st = 0; st < steps && pick < 0; st++) step_pick(st, val(st));
  }
  return pick >= 0 ? pick : last;
}

template <bool CONTRA>
__global__ void __launch_bounds__(256) k_sample(SampleBatch a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u;
  const uint32_t n_waves = gridDim.x * (blockDim.x / 64u);
  uint64_t* stack = a.stack + static_cast<uint64_t>(wave) * a.stack_cap;
  const uint64_t items = static_cast<uint64_t>(a.nseq) * a.n_samples;
  for (uint64_t item = wave; item < items; item += n_waves) {
    const uint32_t x = static_cast<uint32_t>(item / a.n_samples);
    const uint32_t t = static_cast<uint32_t>(item % a.n_samples);
    const SeqDesc sd = a.seqs[x];
    const Grammar<CONTRA> sm = grammar_of<CONTRA>(a, sd);
    uint8_t* row = a.rows + a.row_off[x] + static_cast<uint64_t>(t) * sd.n;
    const float lw = walk_structure<CONTRA>(
        sm, row, stack, a.stack_cap, lane,
        [&](uint32_t type, uint32_t i, uint32_t j, uint32_t cnt, uint32_t dec) {
          const uint32_t bits = philox_u32(a.seed, dec, t, sd.batch_idx, 0u);
          const float u = static_cast<float>(bits >> 8) * (1.0f / 16777216.0f);
          return decide(sm, type, i, j, cnt, u, lane);
        });
    if (lane == 0) a.log_weights[static_cast<uint64_t>(x) * a.n_samples + t] = lw;
  }
}

}  // namespace

void launch_sample(const SampleBatch& a, bool contra, uint32_t n_waves, hipStream_t st) {
  const uint32_t blocks = (n_waves + 3u) / 4u;
  if (contra)
    hipLaunchKernelGGL(k_sample<true>, dim3(blocks), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(k_sample<false>, dim3(blocks), dim3(256), 0, st, a);
}

}  // namespace rnamc
