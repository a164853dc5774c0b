// rnamc_window.hip — windowed local folding (rnamc_bpp_windowed): the pair
// probabilities of the windows of one long sequence, averaged per pair over the windows that
// contain it, off the device-resident packed triangles of a lock-step group of windows.
//   k_window_accumulate  per present cell (d >= 1, d < band) of a window's triangle: the integer
//                        q = min(rint(p * 2^44), 2^45) added into the 64-bit sum of band cell
//                        (start + i, d), and 1 into the cell's 32-bit window counter
//   k_window_finalize    band(i, d) = (float)(sum / (denom * 2^44)), denom = the windows that
//                        contain (i, i + d) in closed form; -1 where no window had the pair.  The
//                        accumulators are diagonal-major ([d * N + i]: a wave of consecutive i of
//                        one diagonal hits consecutive words), the band row-major ([i * B + d]):
//                        a 64 x 64 tile goes through LDS so that both sides stay coalesced
//   k_window_paired      per base x: sum over d ascending of band(x, d), then band(x - d, d), one
//                        rounded f32 add each (the order of rnamc_bpp_batch_sparse's paired_prob);
//                        the cells are re-derived from the accumulators, which a wave reads
//                        consecutively, by the function the finalize kernel uses: the same bits
// Integer adds commute: the sums, and with them every output bit, do not depend on the order in
// which windows, groups, chunks or devices contribute.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rnamc_device.h"

namespace rnamc {

namespace {

constexpr uint32_t kBlock = 256u;  // cells of a block = threads of a workgroup (four waves)
constexpr uint32_t kTile = 64u;    // finalize: a tile of 64 bases x 64 spans
constexpr double kQuantum = 17592186044416.0;      // 2^44
constexpr double kQuantumCap = 35184372088832.0;   // 2^45

// first cell of diagonal d in a packed triangle of n rows (64-bit: exact for every n <= 65535)
__device__ __forceinline__ uint64_t tri_off(uint64_t n, uint64_t d) { return d * n - ((d * (d - 1ull)) >> 1); }

__global__ void __launch_bounds__(kBlock) k_window_accumulate(const WindowItem* items, const float* bpp, uint32_t w,
                                                              uint32_t band, uint64_t n_total,
                                                              unsigned long long* sum, uint32_t* cnt) {
  const uint64_t len = tri_off(w, w);  // w(w+1)/2
  const uint64_t x = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (x < static_cast<uint64_t>(w) || x >= len) return;  // (the main diagonal comes first: d = 0 is no pair)
  const WindowItem it = items[blockIdx.y];
  const float p = bpp[it.bpp_off + x];
  if (!(p > -0.5f)) return;
  // the diagonal of cell x: the largest d in [0, w-1] with tri_off(d) <= x, by bisection in integers
  uint32_t lo = 1u, hi = w - 1u;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (tri_off(w, mid) <= x) lo = mid; else hi = mid - 1u;
  }
  if (lo >= band) return;
  const uint64_t i = it.start + (x - tri_off(w, lo));
  if (i + lo >= n_total) return;  // (never: a window lies inside the sequence)
  const double q = fmin(rint(static_cast<double>(p) * kQuantum), kQuantumCap);  // to nearest, ties to even
  const uint64_t at = static_cast<uint64_t>(lo) * n_total + i;
  atomicAdd(sum + at, static_cast<unsigned long long>(static_cast<long long>(q)));
  atomicAdd(cnt + at, 1u);
}

// band cell (i, d) from its accumulators; 1 <= d, i + d < N
__device__ __forceinline__ float window_value(const WindowGeom& g, uint64_t i, uint32_t d, long long sum,
                                              uint32_t cnt) {
  if (cnt == 0u) return -1.f;
  // windows x * stride of the grid with x * stride <= i and i + d < x * stride + w
  const uint64_t j = i + d;
  const uint64_t lo = j >= g.w ? (j - g.w + g.stride) / g.stride : 0ull;  // ceil((j - w + 1) / stride)
  const uint64_t last = g.n_grid - 1ull, hi = i / g.stride < last ? i / g.stride : last;
  uint64_t den = hi >= lo ? hi - lo + 1ull : 0ull;
  if (g.has_last != 0u && g.n - g.w <= i) den++;  // the window that ends at N, off the grid
  if (den == 0ull) return -1.f;
  return static_cast<float>(static_cast<double>(sum) / (static_cast<double>(den) * kQuantum));
}

__global__ void __launch_bounds__(kBlock) k_window_finalize(WindowGeom g, const long long* sum,
                                                            const uint32_t* cnt, float* out) {
  __shared__ float tile[kTile][kTile + 1u];
  const uint32_t tx = threadIdx.x & (kTile - 1u), ty = threadIdx.x / kTile;  // ty 0 .. 3
  const uint64_t i0 = static_cast<uint64_t>(blockIdx.x) * kTile;
  const uint32_t d0 = blockIdx.y * kTile;
  for (uint32_t r = ty; r < kTile; r += kBlock / kTile) {  // r: span within the tile, tx: base
    const uint64_t i = i0 + tx;
    const uint32_t d = d0 + r;
    float v = -1.f;
    if (d >= 1u && d < g.band && i < g.n && i + d < g.n) {
      const uint64_t at = static_cast<uint64_t>(d) * g.n + i;
      v = window_value(g, i, d, sum[at], cnt[at]);
    }
    tile[r][tx] = v;
  }
  __syncthreads();
  for (uint32_t r = ty; r < kTile; r += kBlock / kTile) {  // r: base within the tile, tx: span
    const uint64_t i = i0 + r;
    const uint32_t d = d0 + tx;
    if (i < g.n && d < g.band) out[i * g.band + d] = tile[tx][r];
  }
}

__global__ void __launch_bounds__(kBlock) k_window_paired(WindowGeom g, const long long* sum, const uint32_t* cnt,
                                                          float* paired) {
  const uint64_t x = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (x >= g.n) return;
  float acc = 0.f;
  for (uint32_t d = 1u; d < g.band; d++) {
    const uint64_t row = static_cast<uint64_t>(d) * g.n;
    if (x + d < g.n) {
      const float p = window_value(g, x, d, sum[row + x], cnt[row + x]);
      if (p > -0.5f) acc += p;
    }
    if (x >= d) {
      const float p = window_value(g, x - d, d, sum[row + x - d], cnt[row + x - d]);
      if (p > -0.5f) acc += p;
    }
  }
  paired[x] = acc;
}

}  // namespace

// (grid.y carries the windows: at most 65535 of them a launch; all of one length w)
void launch_window_accumulate(const WindowItem* items, uint32_t n_items, const float* bpp, uint32_t w, uint32_t band,
                              uint64_t n_total, int64_t* sum, uint32_t* cnt, hipStream_t st) {
  const uint64_t len = static_cast<uint64_t>(w) * (w + 1ull) / 2ull;
  hipLaunchKernelGGL(k_window_accumulate, dim3(static_cast<uint32_t>((len + kBlock - 1u) / kBlock), n_items, 1),
                     dim3(kBlock), 0, st, items, bpp, w, band, n_total, reinterpret_cast<unsigned long long*>(sum),
                     cnt);
}

void launch_window_finalize(const WindowGeom& g, const int64_t* sum, const uint32_t* cnt, float* band_out,
                            hipStream_t st) {
  const uint32_t gx = static_cast<uint32_t>((g.n + kTile - 1u) / kTile);
  hipLaunchKernelGGL(k_window_finalize, dim3(gx, (g.band + kTile - 1u) / kTile, 1), dim3(kBlock), 0, st, g,
                     reinterpret_cast<const long long*>(sum), cnt, band_out);
}

void launch_window_paired(const WindowGeom& g, const int64_t* sum, const uint32_t* cnt, float* paired,
                          hipStream_t st) {
  const uint32_t gx = static_cast<uint32_t>((g.n + kBlock - 1u) / kBlock);
  hipLaunchKernelGGL(k_window_paired, dim3(gx, 1, 1), dim3(kBlock), 0, st, g,
                     reinterpret_cast<const long long*>(sum), cnt, paired);
}

}  // namespace rnamc
