// rnamc_mutant.hip — point-mutation scan (rnamc_mutant_scan): the packed
// triangles of a lock-step group of single-base mutants, each compared with the wild type's
// resident triangle of the same length, cell c against cell c.
//   k_mutant_compare  grid (strips of the triangle) x (mutants).  Per cell of span >= 1, with absent
//                     pairs read as 0: q = min(rint((a - b)^2 * 2^44), 2^45) in f64, summed as a 64-bit
//                     integer, and where |fa - fb| > 0 in f32 the key (bits(|fa - fb|) << 32) |
//                     (0xffffffff - c), whose maximum is the largest move at the smallest cell.  A
//                     lane keeps both over its cells of the strip in registers; lanes are joined
//                     across the wave by shuffles and across the four waves through LDS; the
//                     workgroup issues ONE atomicAdd and at most ONE atomicMax into the mutant's slot.
// Integer adds and maxima commute: the results do not depend on the order in which strips, groups,
// chunks or devices contribute.  The per-base paired probabilities of the scan are
// k_sparse_paired's (rnamc_sparse.hip).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rnamc_device.h"

namespace rnamc {

namespace {

constexpr uint32_t kBlock = 256u;  // threads of a workgroup (four waves); a strip is a multiple of it
constexpr double kQuantum = 17592186044416.0;      // 2^44
constexpr double kQuantumCap = 35184372088832.0;   // 2^45

__global__ void __launch_bounds__(kBlock) k_mutant_compare(const MutantItem* items, const float* __restrict__ wt,
                                                           const float* __restrict__ bpp, uint32_t n, uint64_t len,
                                                           uint32_t strip, unsigned long long* sum,
                                                           unsigned long long* key) {
  __shared__ long long w_sum[kBlock / 64u];
  __shared__ unsigned long long w_key[kBlock / 64u];
  const MutantItem it = items[blockIdx.y];
  const float* __restrict__ mut = bpp + it.bpp_off;
  const uint64_t c0 = static_cast<uint64_t>(blockIdx.x) * strip;
  const uint64_t c1 = c0 + strip < len ? c0 + strip : len;
  long long acc = 0;
  unsigned long long best = 0ull;  // (a cell that moved has t > 0: its key is above 2^32)
  // consecutive lanes read consecutive cells of both triangles; the wild type's strip is the same
  // for every mutant of the launch and comes from the caches
  for (uint64_t c = c0 + threadIdx.x; c < c1; c += kBlock) {
    if (c < n) continue;  // (the main diagonal comes first: d = 0 is no pair)
    const float pw = wt[c], pm = mut[c];
    const float fa = pw > -0.5f ? pw : 0.f, fb = pm > -0.5f ? pm : 0.f;
    const double e = static_cast<double>(fa) - static_cast<double>(fb);
    const double e2 = e * e;  // one rounded multiply (-ffp-contract=off: fused with nothing)
    const double q = fmin(rint(e2 * kQuantum), kQuantumCap);  // exact scaling; to nearest, ties to even
    acc += static_cast<long long>(q);
    const float t = fabsf(fa - fb);
    if (t > 0.f) {
      const unsigned long long k = (static_cast<unsigned long long>(__float_as_uint(t)) << 32) |
                                   static_cast<unsigned long long>(0xffffffffu - static_cast<uint32_t>(c));
      best = k > best ? k : best;
    }
  }
  for (uint32_t s = 32u; s >= 1u; s >>= 1) {
    acc += __shfl_down(acc, s, 64);
    const unsigned long long o = __shfl_down(best, s, 64);
    best = o > best ? o : best;
  }
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) {
    w_sum[wave] = acc;
    w_key[wave] = best;
  }
  __syncthreads();
  if (threadIdx.x != 0u) return;
  for (uint32_t w = 1u; w < kBlock / 64u; w++) {
    acc += w_sum[w];
    best = w_key[w] > best ? w_key[w] : best;
  }
  if (acc != 0) atomicAdd(sum + it.slot, static_cast<unsigned long long>(acc));
  if (best != 0ull) atomicMax(key + it.slot, best);
}

}  // namespace

// (grid.y carries the mutants: at most 65535 of them a launch; all of one length n)
void launch_mutant_compare(const MutantItem* items, uint32_t n_items, const float* wt, const float* bpp, uint32_t n,
                           int64_t* sum, uint64_t* key, hipStream_t st) {
  const uint64_t len = static_cast<uint64_t>(n) * (n + 1ull) / 2ull;
  const uint32_t strip = mutant_strip_of(len);
  hipLaunchKernelGGL(k_mutant_compare, dim3(static_cast<uint32_t>((len + strip - 1u) / strip), n_items, 1),
                     dim3(kBlock), 0, st, items, wt, bpp, n, len, strip, reinterpret_cast<unsigned long long*>(sum),
                     reinterpret_cast<unsigned long long*>(key));
}

}  // namespace rnamc
