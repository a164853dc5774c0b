// rnamc_align.hip — alignment folding (rnamc_bpp_alignment): the pair
// probabilities of the rows of a multiple alignment, each row folded without its gaps, averaged per
// COLUMN pair over all rows, off the device-resident packed triangles of a lock-step group of rows.
//   k_align_accumulate  per present cell (d >= 1) of a row's triangle: the integer
//                       q = min(rint(p * 2^44), 2^45) added into the 64-bit sum of column-pair cell
//                       (map[i], map[i + d]), and 1 into the cell's 32-bit row counter.  The rows of
//                       a launch differ in length: a lane finds its diagonal with its item's own n
//   k_align_finalize    avg = (float)(sum / (n_rows * 2^44)), -1 where no row had the pair and on
//                       the main diagonal.  Accumulators and result are both packed diagonal-major
//                       triangles over the columns: a lane per cell, nothing to transpose
//   k_align_paired      per column c: sum over d ascending of avg(c, c + d), then avg(c - d, c), one
//                       rounded f32 add each (the order of rnamc_bpp_batch_sparse's paired_prob);
//                       the cells are re-derived from the accumulators, which a wave reads
//                       consecutively, by the function the finalize kernel uses: the same bits
// Integer adds commute: the sums, and with them every output bit, do not depend on the order in
// which rows, groups or devices contribute.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rnamc_device.h"

namespace rnamc {

namespace {

constexpr uint32_t kBlock = 256u;  // cells of a block = threads of a workgroup (four waves)
constexpr double kQuantum = 17592186044416.0;      // 2^44
constexpr double kQuantumCap = 35184372088832.0;   // 2^45

// first cell of diagonal d in a packed triangle of n rows (64-bit: exact for every n <= 65535)
__device__ __forceinline__ uint64_t tri_off(uint64_t n, uint64_t d) { return d * n - ((d * (d - 1ull)) >> 1); }

__global__ void __launch_bounds__(kBlock) k_align_accumulate(const AlignItem* items, const float* bpp,
                                                             const uint32_t* maps, uint32_t n_cols,
                                                             unsigned long long* sum, uint32_t* cnt) {
  const AlignItem it = items[blockIdx.y];
  const uint64_t len = tri_off(it.n, it.n);  // n(n+1)/2
  const uint64_t x = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  // (the main diagonal comes first: d = 0 is no pair; the grid is cut for the launch's longest row)
  if (x < static_cast<uint64_t>(it.n) || x >= len) return;
  const float p = bpp[it.bpp_off + x];
  if (!(p > -0.5f)) return;
  // the diagonal of cell x: the largest d in [1, n-1] with tri_off(d) <= x, by bisection in integers
  uint32_t lo = 1u, hi = it.n - 1u;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (tri_off(it.n, mid) <= x) lo = mid; else hi = mid - 1u;
  }
  const uint32_t i = static_cast<uint32_t>(x - tri_off(it.n, lo));
  const uint32_t ci = maps[it.map_off + i], cj = maps[it.map_off + i + lo];
  if (ci >= cj || cj >= n_cols) return;  // (never: a row's map ascends inside the alignment)
  const double q = fmin(rint(static_cast<double>(p) * kQuantum), kQuantumCap);  // to nearest, ties to even
  const uint64_t at = tri_off(n_cols, cj - ci) + ci;
  atomicAdd(sum + at, static_cast<unsigned long long>(static_cast<long long>(q)));
  atomicAdd(cnt + at, 1u);
}

// column-pair cell from its accumulators (not on the main diagonal)
__device__ __forceinline__ float align_value(long long sum, uint32_t cnt, double denom) {
  if (cnt == 0u) return -1.f;
  return static_cast<float>(static_cast<double>(sum) / denom);
}

__global__ void __launch_bounds__(kBlock) k_align_finalize(uint32_t n_cols, uint32_t n_rows, const long long* sum,
                                                           const uint32_t* cnt, float* out) {
  const uint64_t x = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (x >= tri_off(n_cols, n_cols)) return;
  const double denom = static_cast<double>(n_rows) * kQuantum;
  out[x] = x < n_cols ? -1.f : align_value(sum[x], cnt[x], denom);
}

__global__ void __launch_bounds__(kBlock) k_align_paired(uint32_t n_cols, uint32_t n_rows, const long long* sum,
                                                         const uint32_t* cnt, float* paired) {
  const uint32_t c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= n_cols) return;
  const double denom = static_cast<double>(n_rows) * kQuantum;
  float acc = 0.f;
  uint64_t row = n_cols;  // tri_off(n_cols, 1)
  for (uint32_t d = 1u; d < n_cols; d++) {
    if (c + d < n_cols) {
      const float p = align_value(sum[row + c], cnt[row + c], denom);
      if (p > -0.5f) acc += p;
    }
    if (c >= d) {
      const float p = align_value(sum[row + c - d], cnt[row + c - d], denom);
      if (p > -0.5f) acc += p;
    }
    row += n_cols - d;  // diagonal d holds n_cols - d cells
  }
  paired[c] = acc;
}

}  // namespace

// (grid.y carries the rows: at most 65535 of them a launch, the longest first)
void launch_align_accumulate(const AlignItem* items, uint32_t n_items, uint32_t max_n, const float* bpp,
                             const uint32_t* maps, uint32_t n_cols, int64_t* sum, uint32_t* cnt, hipStream_t st) {
  const uint64_t len = static_cast<uint64_t>(max_n) * (max_n + 1ull) / 2ull;
  hipLaunchKernelGGL(k_align_accumulate, dim3(static_cast<uint32_t>((len + kBlock - 1u) / kBlock), n_items, 1),
                     dim3(kBlock), 0, st, items, bpp, maps, n_cols, reinterpret_cast<unsigned long long*>(sum), cnt);
}

void launch_align_finalize(uint32_t n_cols, uint32_t n_rows, const int64_t* sum, const uint32_t* cnt, float* out,
                           hipStream_t st) {
  const uint64_t len = static_cast<uint64_t>(n_cols) * (n_cols + 1ull) / 2ull;
  hipLaunchKernelGGL(k_align_finalize, dim3(static_cast<uint32_t>((len + kBlock - 1u) / kBlock), 1, 1), dim3(kBlock),
                     0, st, n_cols, n_rows, reinterpret_cast<const long long*>(sum), cnt, out);
}

void launch_align_paired(uint32_t n_cols, uint32_t n_rows, const int64_t* sum, const uint32_t* cnt, float* paired,
                         hipStream_t st) {
  hipLaunchKernelGGL(k_align_paired, dim3((n_cols + kBlock - 1u) / kBlock, 1, 1), dim3(kBlock), 0, st, n_cols,
                     n_rows, reinterpret_cast<const long long*>(sum), cnt, paired);
}

}  // namespace rnamc
