// rnamc_centroid_batch.hip — gamma-centroid folds of a whole batch on the GPU: the Theta(n^3) fill
// of every (sequence, threshold) item of a chunk, one launch per anti-diagonal, and the traceback,
// one wave per item (reference: src/centroid_fold.rs:25-105, run for 18 gammas per record by
// src/bin/centroid_fold.rs:119-161).  DESIGN.md section 12.
//
//   M[i][j] = max( M[i+1][j], M[i][j-1], (M[i+1][j-1] + gamma * p(i,j)) - 1   (if (i,j) has a bpp),
//                  max_{i<k<j} M[i][k] + M[k+1][j] ),     M = 0 below and on the main diagonal.
//
// The arithmetic is k_centroid's (rnamc_centroid.hip): every candidate is ONE rounded addition, the
// pair term one multiply, one add, one subtract, never fused (-ffp-contract=off), and the maximum
// of a set does not depend on the order it is taken in — so the matrices carry the reference's
// bits and the traceback's exact float comparisons find what the host traceback finds.
//
// Layout: one packed diagonal-major triangle per item, indexed like the bpp triangle.  With a lane
// per cell and lanes on consecutive rows i of diagonal d, step a (k = i + a) reads
//   M[i][i+a]      at off(a)       + i            and
//   M[i+a+1][i+d]  at off(d-a-1)   + i + a + 1,
// both consecutive floats across the wave (as k_mfe's QM loop).  Short sums
// take one lane per cell; long sums are cut over the KS waves of a workgroup (wave w takes the
// steps a = 1 + w mod KS, the same coalesced reads) and joined through LDS.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rnamc_device.h"

namespace rnamc {

namespace {

// first float of diagonal x in a packed triangle of n rows (x <= 65535: no 32-bit overflow)
__device__ __forceinline__ uint32_t diag_off(uint32_t n, uint32_t x) { return x * n - ((x * (x - 1u)) >> 1); }

__global__ void __launch_bounds__(256) k_centroid_batch_init(CentroidChunk a) {
  const CentroidItem it = a.items[blockIdx.y];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i < it.n) a.m[it.m_off + i] = 0.f;
}

// largest entry of every sequence's bpp triangle (absent pairs are negative): one workgroup per
// sequence; seqs[x] carries bpp_off and n
__global__ void __launch_bounds__(256) k_centroid_pmax(const CentroidItem* seqs, const float* bpp, float* out) {
  __shared__ float red[256];
  const CentroidItem it = seqs[blockIdx.x];
  const float* __restrict__ P = bpp + it.bpp_off;
  const uint32_t len = diag_off(it.n, it.n);  // n(n+1)/2
  float best = -1.f;
  for (uint32_t x = threadIdx.x; x < len; x += 256u) best = fmaxf(best, P[x]);
  red[threadIdx.x] = best;
  __syncthreads();
  for (uint32_t w = 128u; w > 0u; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + w]);
    __syncthreads();
  }
  if (threadIdx.x == 0u) out[blockIdx.x] = red[0];
}

template <int KS>
__global__ void __launch_bounds__(64 * KS) k_centroid_batch(CentroidChunk a, uint32_t d) {
  __shared__ float red[KS > 1 ? KS - 1 : 1][64];
  const CentroidItem it = a.items[blockIdx.y];
  const uint32_t n = it.n;
  if (blockIdx.x * 64u + d >= n) return;  // (the whole workgroup: no barrier is left waiting)
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t slice = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const uint32_t i = blockIdx.x * 64u + lane;
  const bool live = i + d < n;
  float* __restrict__ M = a.m + it.m_off;
  float best = 0.f;  // (every M is >= 0: the empty structure)
  if (live) {
    // bifurcations k = i + a, a = 1 .. d-1: M[i][k] + M[k+1][j]
    uint32_t s = 1u + slice;
    for (; s + 3u * KS < d; s += 4u * KS) {
      const uint32_t s1 = s + KS, s2 = s + 2u * KS, s3 = s + 3u * KS;
      const float c0 = M[diag_off(n, s) + i] + M[diag_off(n, d - 1u - s) + i + s + 1u];
      const float c1 = M[diag_off(n, s1) + i] + M[diag_off(n, d - 1u - s1) + i + s1 + 1u];
      const float c2 = M[diag_off(n, s2) + i] + M[diag_off(n, d - 1u - s2) + i + s2 + 1u];
      const float c3 = M[diag_off(n, s3) + i] + M[diag_off(n, d - 1u - s3) + i + s3 + 1u];
      best = fmaxf(fmaxf(best, fmaxf(c0, c1)), fmaxf(c2, c3));
    }
    for (; s < d; s += KS) best = fmaxf(best, M[diag_off(n, s) + i] + M[diag_off(n, d - 1u - s) + i + s + 1u]);
  }
  if (KS > 1) {
    if (slice != 0u) red[slice - 1u][lane] = best;
    __syncthreads();
    if (slice != 0u) return;
    for (int w = 0; w < KS - 1; w++) best = fmaxf(best, red[w][lane]);
  }
  if (!live) return;
  const uint32_t below = diag_off(n, d - 1u) + i;
  best = fmaxf(best, M[below + 1u]);  // M[i+1][j]
  best = fmaxf(best, M[below]);       // M[i][j-1]
  const uint32_t cell = diag_off(n, d) + i;
  const float pr = a.bpp[it.bpp_off + cell];
  if (pr >= -0.5f) {  // present in the SparseProbMat
    const float inner = d >= 2u ? M[diag_off(n, d - 2u) + i + 1u] : 0.f;  // M[i+1][j-1]
    const float cand = inner + it.gamma * pr - 1.f;  // ((M + g*p) - 1), as the reference parses it
    best = fmaxf(best, cand);
  }
  M[cell] = best;
}

// The reference's traceback (rnamc_internal.h, centroid_traceback): exact float equality tests in
// the order left skip, right skip, pair, first bifurcation k.  Every lane of the wave holds the
// same interval and reads the same values; the k scan tries 64 candidates a step and a ballot takes
// the lowest.  A skip or a pair continues in place; a bifurcation parks (i, k) on the wave's stack
// and continues with (k+1, j) — the order the host's LIFO stack visits them in.  Parked intervals
// are disjoint and non-empty: at most n of them.
__global__ void __launch_bounds__(256) k_centroid_trace(CentroidChunk a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u;
  const uint32_t n_waves = gridDim.x * (blockDim.x / 64u);
  uint64_t* stack = a.stack + static_cast<uint64_t>(wave) * a.stack_cap;
  for (uint32_t item = wave; item < a.n_items; item += n_waves) {
    const CentroidItem it = a.items[item];
    const uint32_t n = it.n;
    const float* __restrict__ M = a.m + it.m_off;
    const float* __restrict__ P = a.bpp + it.bpp_off;
    uint8_t* row = a.rows + it.row_off;
    // position x is written by lane x % 64 alone, first '.', then its bracket: program order
    for (uint32_t x = lane; x < n; x += 64u) row[x] = '.';
    uint32_t sp = 0, np = 0, i = 0, j = n - 1u;
    bool have = true, overflow = false;
    for (;;) {
      if (!have) {
        if (sp == 0u) break;
        const uint64_t e = stack[--sp];
        i = static_cast<uint32_t>(e >> 32);
        j = static_cast<uint32_t>(e);
      }
      have = false;
      if (j <= i) continue;
      const uint32_t d = j - i;
      const float best = M[diag_off(n, d) + i];
      if (best == 0.f) continue;
      const uint32_t below = diag_off(n, d - 1u) + i;
      if (best == M[below + 1u]) {  // M[i+1][j]
        i++;
        have = true;
        continue;
      }
      if (best == M[below]) {  // M[i][j-1]
        j--;
        have = true;
        continue;
      }
      const float pr = P[diag_off(n, d) + i];
      const float inner = d >= 2u ? M[diag_off(n, d - 2u) + i + 1u] : 0.f;
      if (pr >= -0.5f && best == inner + it.gamma * pr - 1.f) {
        if ((i & 63u) == lane) row[i] = '(';
        if ((j & 63u) == lane) row[j] = ')';
        np++;
        i++;
        j--;
        have = true;
        continue;
      }
      for (uint32_t k0 = i + 1u; k0 < j; k0 += 64u) {
        const uint32_t k = k0 + lane;
        bool hit = false;
        if (k < j) hit = best == M[diag_off(n, k - i) + i] + M[diag_off(n, j - k - 1u) + k + 1u];
        const uint64_t mask = __ballot(hit);
        if (mask != 0ull) {
          const uint32_t kk = k0 + static_cast<uint32_t>(__builtin_ctzll(mask));
          if (sp >= a.stack_cap) {
            overflow = true;
          } else {
            stack[sp++] = (static_cast<uint64_t>(i) << 32) | kk;  // every lane, the same value
            i = kk + 1u;
            have = true;
          }
          break;
        }
      }
      if (overflow) break;
    }
    if (lane == 0u) {
      a.n_pairs[item] = overflow ? 0xffffffffu : np;
      a.expect_accuracy[item] = M[diag_off(n, n - 1u)];
    }
  }
}

}  // namespace

void launch_centroid_pmax(const CentroidItem* seqs, const float* bpp, float* out, uint32_t nseq, hipStream_t st) {
  hipLaunchKernelGGL(k_centroid_pmax, dim3(nseq), dim3(256), 0, st, seqs, bpp, out);
}

void launch_centroid_batch_init(const CentroidChunk& a, uint32_t max_n, hipStream_t st) {
  hipLaunchKernelGGL(k_centroid_batch_init, dim3((max_n + 255u) / 256u, a.n_items, 1), dim3(256), 0, st, a);
}

void launch_centroid_batch(const CentroidChunk& a, uint32_t d, uint32_t n_active, uint32_t max_n,
                           hipStream_t st) {
  const dim3 grid((max_n - d + 63u) / 64u, n_active, 1);
  // a lane per cell while the sums are short; beyond, the sum is cut over 4 or 16 waves
  if (d <= 64u)
    hipLaunchKernelGGL(k_centroid_batch<1>, grid, dim3(64), 0, st, a, d);
  else if (d <= 1024u)
    hipLaunchKernelGGL(k_centroid_batch<4>, grid, dim3(256), 0, st, a, d);
  else
    hipLaunchKernelGGL(k_centroid_batch<16>, grid, dim3(1024), 0, st, a, d);
}

void launch_centroid_trace(const CentroidChunk& a, uint32_t n_waves, hipStream_t st) {
  hipLaunchKernelGGL(k_centroid_trace, dim3((n_waves + 3u) / 4u), dim3(256), 0, st, a);
}

}  // namespace rnamc
