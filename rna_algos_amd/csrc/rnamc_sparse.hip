// rnamc_sparse.hip — thresholded sparse pair probabilities of a lock-step group, compacted on the
// GPU off the group's device-resident packed triangles: count, scan, fill,
// and the per-base paired probabilities.
//
// A record's packed triangle is cut into blocks of 256 consecutive cells (packed order: span
// ascending, then i ascending).  A cell is LISTED when it is present (p > -0.5) and p >= min_prob.
//   k_sparse_count  listed cells of every block (ballot popcounts joined through LDS)
//   k_sparse_scan   per record: exclusive scan of its block counts in place, and the record's total
//   k_sparse_fill   the same predicate; rank = listed lanes below in the wave + listed cells of the
//                   workgroup's earlier waves + block base + record base: the list is in packed order
//   k_sparse_paired per base x: sum over d ascending of p(x, x+d), then p(x-d, x), one rounded f32
//                   add each (the order include/rnamc.h defines)
// No atomics and no order that depends on scheduling: the lists are a pure function of the triangle.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rnamc_device.h"

namespace rnamc {

namespace {

constexpr uint32_t kBlock = 256u;  // cells of a block = threads of a workgroup (four waves)

// first cell of diagonal d in a packed triangle of n rows (64-bit: exact for every n <= 65535)
__device__ __forceinline__ uint64_t tri_off(uint64_t n, uint64_t d) { return d * n - ((d * (d - 1ull)) >> 1); }

__device__ __forceinline__ bool listed(float p, float min_prob) { return p > -0.5f && p >= min_prob; }

// the lane's flag over the wave: listed lanes below this one, and all of them
__device__ __forceinline__ uint32_t wave_rank(bool flag, uint32_t* wave_total) {
  const uint64_t mask = __ballot(flag);
  *wave_total = static_cast<uint32_t>(__popcll(mask));
  return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32),
                                   __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
}

__global__ void __launch_bounds__(kBlock) k_sparse_count(const SparseItem* items, const float* bpp,
                                                         uint32_t* blocks, float min_prob) {
  __shared__ uint32_t wsum[kBlock / 64u];
  const SparseItem it = items[blockIdx.y];
  if (blockIdx.x >= it.n_blocks) return;  // (the whole workgroup: no barrier is left waiting)
  const uint64_t len = tri_off(it.n, it.n);  // n(n+1)/2
  const uint64_t x = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const bool flag = x < len && listed(bpp[it.bpp_off + x], min_prob);
  uint32_t total;
  (void)wave_rank(flag, &total);
  if ((threadIdx.x & 63u) == 0u) wsum[threadIdx.x >> 6] = total;
  __syncthreads();
  if (threadIdx.x == 0u) blocks[it.blk_off + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// One workgroup per record: its block counts become exclusive block bases, 256 blocks a step with
// the running sum carried along (a record's total is below 2^31: it fits the u32).
__global__ void __launch_bounds__(kBlock) k_sparse_scan(const SparseItem* items, uint32_t* blocks,
                                                        uint32_t* totals) {
  __shared__ uint32_t buf[kBlock];
  const SparseItem it = items[blockIdx.x];
  uint32_t* b = blocks + it.blk_off;
  uint32_t carry = 0u;
  for (uint32_t base = 0u; base < it.n_blocks; base += kBlock) {
    const uint32_t k = base + threadIdx.x;
    const uint32_t v = k < it.n_blocks ? b[k] : 0u;
    buf[threadIdx.x] = v;
    __syncthreads();
    // inclusive scan (Hillis-Steele), two barriers a step
    for (uint32_t s = 1u; s < kBlock; s <<= 1) {
      const uint32_t add = threadIdx.x >= s ? buf[threadIdx.x - s] : 0u;
      __syncthreads();
      buf[threadIdx.x] += add;
      __syncthreads();
    }
    if (k < it.n_blocks) b[k] = carry + buf[threadIdx.x] - v;
    carry += buf[kBlock - 1u];
    __syncthreads();  // (buf is rewritten by the next step)
  }
  if (threadIdx.x == 0u) totals[blockIdx.x] = carry;
}

__global__ void __launch_bounds__(kBlock) k_sparse_fill(const SparseItem* items, const float* bpp,
                                                        const uint32_t* blocks, float min_prob, uint32_t* out_i,
                                                        uint32_t* out_j, float* out_p) {
  __shared__ uint32_t wsum[kBlock / 64u];
  const SparseItem it = items[blockIdx.y];
  if (blockIdx.x >= it.n_blocks) return;
  const uint64_t n = it.n;
  const uint64_t len = tri_off(n, n);
  const uint64_t x = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const float p = x < len ? bpp[it.bpp_off + x] : -1.f;
  const bool flag = listed(p, min_prob);
  uint32_t total;
  const uint32_t below = wave_rank(flag, &total);
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) wsum[wave] = total;
  __syncthreads();
  if (!flag) return;
  uint32_t rank = below;
  for (uint32_t w = 0u; w < wave; w++) rank += wsum[w];
  // the diagonal of cell x: the largest d in [0, n-1] with tri_off(d) <= x, by bisection in
  // integers (at most 16 steps for n <= 65535); every lane finds its own
  uint32_t lo = 0u, hi = it.n - 1u;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (tri_off(n, mid) <= x) lo = mid; else hi = mid - 1u;
  }
  const uint32_t i = static_cast<uint32_t>(x - tri_off(n, lo));
  const uint64_t at = it.out_off + blocks[it.blk_off + blockIdx.x] + rank;
  out_i[at] = i;
  out_j[at] = i + lo;
  out_p[at] = p;
}

// One lane per base; its two reads of a step, off(d) + x and off(d) + x - d, are consecutive
// floats across the wave.
__global__ void __launch_bounds__(kBlock) k_sparse_paired(const SparseItem* items, const float* bpp,
                                                          float* paired) {
  const SparseItem it = items[blockIdx.y];
  const uint32_t x = blockIdx.x * kBlock + threadIdx.x;
  if (x >= it.n) return;
  const float* __restrict__ P = bpp + it.bpp_off;
  const uint32_t n = it.n;
  float acc = 0.f;
  uint64_t off = n;  // tri_off(n, 1)
  for (uint32_t d = 1u; d < n; d++) {
    if (x + d < n) {
      const float p = P[off + x];
      if (p > -0.5f) acc += p;
    }
    if (x >= d) {
      const float p = P[off + x - d];
      if (p > -0.5f) acc += p;
    }
    off += n - d;
  }
  paired[it.pp_off + x] = acc;
}

}  // namespace

// (grid.y carries the records: at most 65535 of them a launch)
void launch_sparse_count(const SparseItem* items, uint32_t n_items, uint32_t max_blocks, const float* bpp,
                         uint32_t* blocks, float min_prob, hipStream_t st) {
  hipLaunchKernelGGL(k_sparse_count, dim3(max_blocks, n_items, 1), dim3(kBlock), 0, st, items, bpp, blocks,
                     min_prob);
}

void launch_sparse_scan(const SparseItem* items, uint32_t n_items, uint32_t* blocks, uint32_t* totals,
                        hipStream_t st) {
  hipLaunchKernelGGL(k_sparse_scan, dim3(n_items), dim3(kBlock), 0, st, items, blocks, totals);
}

void launch_sparse_fill(const SparseItem* items, uint32_t n_items, uint32_t max_blocks, const float* bpp,
                        const uint32_t* blocks, float min_prob, uint32_t* out_i, uint32_t* out_j, float* out_p,
                        hipStream_t st) {
  hipLaunchKernelGGL(k_sparse_fill, dim3(max_blocks, n_items, 1), dim3(kBlock), 0, st, items, bpp, blocks,
                     min_prob, out_i, out_j, out_p);
}

void launch_sparse_paired(const SparseItem* items, uint32_t n_items, uint32_t max_n, const float* bpp,
                          float* paired, hipStream_t st) {
  hipLaunchKernelGGL(k_sparse_paired, dim3((max_n + kBlock - 1u) / kBlock, n_items, 1), dim3(kBlock), 0, st,
                     items, bpp, paired);
}

}  // namespace rnamc
