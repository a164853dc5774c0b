// rnamc_match.hip — what is made of a match-probability matrix while it is still on the device
// (DESIGN.md section 20): the thresholded list of its cells (count, scan, fill, the pattern of
// rnamc_sparse.hip), the per-base marginals, and the gamma-centroid alignment of every gamma (the
// (max,+) fill by anti-diagonal and its traceback, include/rnamc.h, rnamc_match_align).
//
// A matrix is a dense row-major n1 x n2 ProbMat; its border rows and columns are the pseudo bases
// and are never listed, summed or aligned.  L1 = n1 - 2, L2 = n2 - 2.
//   k_match_count      listed cells of every block of 256 consecutive cells (row-major order)
//   k_match_scan       per matrix: exclusive scan of its block counts in place, and its total
//   k_match_list       the same predicate; rank = listed lanes below in the wave + listed cells of the
//                      workgroup's earlier waves + block base + matrix base: the list is row-major
//   k_match_marginals  one lane per row and per column: the cells of the line ascending, one rounded
//                      f32 add each
//   k_match_align      one workgroup per (matrix, gamma): the chain of L1 + L2 - 1 anti-diagonals in
//                      one launch, lanes along the diagonal (strided where it is longer than the
//                      workgroup), three live diagonals in LDS (spilled to the workspace where a
//                      diagonal has more than kMatchDiagLds cells), one direction byte per cell to the
//                      workspace, then the traceback by the workgroup's first lane
// No atomics and no order that depends on scheduling: every output is a pure function of the matrix.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rnamc_device.h"

namespace rnamc {

namespace {

constexpr uint32_t kBlock = 256u;  // cells of a block = threads of a workgroup (four waves)

// an interior cell with p > 0 and p >= min_prob (both f32 comparisons)
__device__ __forceinline__ bool listed(const MatchMat& mt, uint64_t x, float p, float min_prob) {
  const uint32_t i = static_cast<uint32_t>(x / mt.n2), j = static_cast<uint32_t>(x - static_cast<uint64_t>(i) * mt.n2);
  return i >= 1u && i + 1u < mt.n1 && j >= 1u && j + 1u < mt.n2 && p > 0.f && p >= min_prob;
}

// the lane's flag over the wave: listed lanes below this one, and all of them
__device__ __forceinline__ uint32_t wave_rank(bool flag, uint32_t* wave_total) {
  const uint64_t mask = __ballot(flag);
  *wave_total = static_cast<uint32_t>(__popcll(mask));
  return __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32),
                                   __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
}

__global__ void __launch_bounds__(kBlock) k_match_count(const MatchMat* mats, const float* probs,
                                                        uint32_t* blocks, float min_prob) {
  __shared__ uint32_t wsum[kBlock / 64u];
  const MatchMat mt = mats[blockIdx.y];
  if (blockIdx.x >= mt.n_blocks) return;  // (the whole workgroup: no barrier is left waiting)
  const uint64_t cells = static_cast<uint64_t>(mt.n1) * mt.n2;
  const uint64_t x = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const bool flag = x < cells && listed(mt, x, probs[mt.p_off + x], min_prob);
  uint32_t total;
  (void)wave_rank(flag, &total);
  if ((threadIdx.x & 63u) == 0u) wsum[threadIdx.x >> 6] = total;
  __syncthreads();
  if (threadIdx.x == 0u) blocks[mt.blk_off + blockIdx.x] = wsum[0] + wsum[1] + wsum[2] + wsum[3];
}

// One workgroup per matrix: its block counts become exclusive block bases, 256 blocks a step with
// the running sum carried along (a matrix of at most 65537^2 cells: its total fits the u32).
__global__ void __launch_bounds__(kBlock) k_match_scan(const MatchMat* mats, uint32_t* blocks, uint32_t* totals) {
  __shared__ uint32_t buf[kBlock];
  const MatchMat mt = mats[blockIdx.x];
  uint32_t* b = blocks + mt.blk_off;
  uint32_t carry = 0u;
  for (uint32_t base = 0u; base < mt.n_blocks; base += kBlock) {
    const uint32_t k = base + threadIdx.x;
    const uint32_t v = k < mt.n_blocks ? b[k] : 0u;
    buf[threadIdx.x] = v;
    __syncthreads();
    // inclusive scan (Hillis-Steele), two barriers a step
    for (uint32_t s = 1u; s < kBlock; s <<= 1) {
      const uint32_t add = threadIdx.x >= s ? buf[threadIdx.x - s] : 0u;
      __syncthreads();
      buf[threadIdx.x] += add;
      __syncthreads();
    }
    if (k < mt.n_blocks) b[k] = carry + buf[threadIdx.x] - v;
    carry += buf[kBlock - 1u];
    __syncthreads();  // (buf is rewritten by the next step)
  }
  if (threadIdx.x == 0u) totals[blockIdx.x] = carry;
}

__global__ void __launch_bounds__(kBlock) k_match_list(const MatchMat* mats, const float* probs,
                                                       const uint32_t* blocks, float min_prob, uint32_t* out_i,
                                                       uint32_t* out_j, float* out_p) {
  __shared__ uint32_t wsum[kBlock / 64u];
  const MatchMat mt = mats[blockIdx.y];
  if (blockIdx.x >= mt.n_blocks) return;
  const uint64_t cells = static_cast<uint64_t>(mt.n1) * mt.n2;
  const uint64_t x = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const float p = x < cells ? probs[mt.p_off + x] : 0.f;
  const bool flag = x < cells && listed(mt, x, p, min_prob);
  uint32_t total;
  const uint32_t below = wave_rank(flag, &total);
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 0u) wsum[wave] = total;
  __syncthreads();
  if (!flag) return;
  uint32_t rank = below;
  for (uint32_t w = 0u; w < wave; w++) rank += wsum[w];
  const uint32_t i = static_cast<uint32_t>(x / mt.n2);
  const uint64_t at = mt.out_off + blocks[mt.blk_off + blockIdx.x] + rank;
  out_i[at] = i;
  out_j[at] = static_cast<uint32_t>(x - static_cast<uint64_t>(i) * mt.n2);
  out_p[at] = p;
}

// Lane x < n1 sums row x, lane n1 + y column y: the lanes of the columns read consecutive floats, the
// lanes of the rows walk n2 floats apart (each through its own cache lines: a row is contiguous).
__global__ void __launch_bounds__(kBlock) k_match_marginals(const MatchMat* mats, const float* probs,
                                                            float* matched) {
  const MatchMat mt = mats[blockIdx.y];
  const uint32_t x = blockIdx.x * kBlock + threadIdx.x;
  if (x >= mt.n1 + mt.n2) return;
  const float* __restrict__ P = probs + mt.p_off;
  const uint32_t n1 = mt.n1, n2 = mt.n2;
  float acc = 0.f;
  if (x < n1) {
    if (x >= 1u && x + 1u < n1)
      for (uint32_t j = 1u; j + 1u < n2; j++) acc += P[static_cast<uint64_t>(x) * n2 + j];
  } else {
    const uint32_t y = x - n1;
    if (y >= 1u && y + 1u < n2)
      for (uint32_t i = 1u; i + 1u < n1; i++) acc += P[static_cast<uint64_t>(i) * n2 + y];
  }
  matched[mt.marg_off + x] = acc;
}

// The chain of anti-diagonals s = 2 .. L1 + L2 of one item.  The three live diagonals are indexed by
// the row i of a cell, L1 + 1 floats each: cell (i, j) of diagonal s reads (i-1, j) and (i, j-1) of
// diagonal s-1 at [i-1] and [i], (i-1, j-1) of diagonal s-2 at [i-1]; row 0 and column 0 are +0 and
// never stored.  One barrier a diagonal: the buffer written is the one read two diagonals ago.
// Returns M[L1][L2] (valid on every lane after the last barrier).
__device__ __forceinline__ float match_chain(float* b0, float* b1, float* b2, const float* __restrict__ P,
                                             uint32_t l1, uint32_t l2, uint32_t n2, float gamma,
                                             uint8_t* __restrict__ dir) {
  float* cur = b0;
  float* p1 = b1;  // diagonal s-1
  float* p2 = b2;  // diagonal s-2
  const uint32_t w = l1 + 1u;
  for (uint32_t s = 2u; s <= l1 + l2; s++) {
    const uint32_t ilo = s > l2 ? s - l2 : 1u, ihi = min(l1, s - 1u);
    uint8_t* __restrict__ drow = dir + static_cast<uint64_t>(s) * w;
    for (uint32_t i = ilo + threadIdx.x; i <= ihi; i += blockDim.x) {
      const uint32_t j = s - i;
      const float up = i > 1u ? p1[i - 1u] : 0.f;
      const float left = j > 1u ? p1[i] : 0.f;
      const float dg = (i > 1u && j > 1u) ? p2[i - 1u] : 0.f;
      // one rounded multiply, one rounded add, one rounded subtract (-ffp-contract=off)
      const float gp = gamma * P[static_cast<uint64_t>(i) * n2 + j];
      const float sum = dg + gp;
      const float cand = sum - 1.f;
      const float m = fmaxf(fmaxf(up, left), cand);
      cur[i] = m;
      // what the traceback's equality tests decide at this cell, in their order
      drow[i] = m == up ? 0u : (m == left ? 1u : 2u);
    }
    __syncthreads();
    float* t = p2;
    p2 = p1;
    p1 = cur;
    cur = t;
  }
  return p1[l1];
}

__global__ void __launch_bounds__(kBlock) k_match_align(const MatchMat* mats, const float* probs,
                                                        const float* gammas, uint32_t ng, float* ws,
                                                        int32_t* mate, uint32_t* n_matched, float* accuracy) {
  __shared__ float lds[3u * kMatchDiagLds];
  const uint32_t item = blockIdx.x;
  const uint32_t which = item / ng, g = item - which * ng;
  const MatchMat mt = mats[which];
  const uint32_t n1 = mt.n1, n2 = mt.n2, l1 = n1 - 2u, l2 = n2 - 2u;
  int32_t* __restrict__ row = mate + mt.mate_off + static_cast<uint64_t>(g) * n1;
  for (uint32_t i = threadIdx.x; i < n1; i += blockDim.x) row[i] = -1;
  if (l1 == 0u || l2 == 0u) {  // an empty sequence: the empty alignment (the whole workgroup leaves)
    if (threadIdx.x == 0u) {
      n_matched[item] = 0u;
      accuracy[item] = 0.f;
    }
    return;
  }
  const uint32_t w = l1 + 1u;
  uint8_t* dir = reinterpret_cast<uint8_t*>(ws) + mt.dir_off + g * match_dir_bytes(n1, n2);
  const float* __restrict__ P = probs + mt.p_off;
  const float gamma = gammas[g];
  float acc;
  if (w <= kMatchDiagLds) {
    acc = match_chain(lds, lds + kMatchDiagLds, lds + 2u * kMatchDiagLds, P, l1, l2, n2, gamma, dir);
  } else {
    float* sp = ws + mt.spill_off + static_cast<uint64_t>(g) * 3u * w;
    acc = match_chain(sp, sp + w, sp + 2ull * w, P, l1, l2, n2, gamma, dir);
  }
  // (the chain ends on a barrier: the workgroup's direction bytes and the -1 of every row are
  // visible to its first lane)
  if (threadIdx.x != 0u) return;
  uint32_t i = l1, j = l2, count = 0u;
  while (i > 0u && j > 0u) {
    const uint32_t d = dir[static_cast<uint64_t>(i + j) * w + i];
    if (d == 0u) {
      i--;
    } else if (d == 1u) {
      j--;
    } else {
      row[i] = static_cast<int32_t>(j);
      count++;
      i--;
      j--;
    }
  }
  n_matched[item] = count;
  accuracy[item] = acc;
}

}  // namespace

// (grid.y carries the matrices: at most 65535 of them a launch)
void launch_match_count(const MatchMat* mats, uint32_t n_mats, uint32_t max_blocks, const float* probs,
                        uint32_t* blocks, float min_prob, hipStream_t st) {
  hipLaunchKernelGGL(k_match_count, dim3(max_blocks, n_mats, 1), dim3(kBlock), 0, st, mats, probs, blocks,
                     min_prob);
}

void launch_match_scan(const MatchMat* mats, uint32_t n_mats, uint32_t* blocks, uint32_t* totals, hipStream_t st) {
  hipLaunchKernelGGL(k_match_scan, dim3(n_mats), dim3(kBlock), 0, st, mats, blocks, totals);
}

void launch_match_list(const MatchMat* mats, uint32_t n_mats, uint32_t max_blocks, const float* probs,
                       const uint32_t* blocks, float min_prob, uint32_t* out_i, uint32_t* out_j, float* out_p,
                       hipStream_t st) {
  hipLaunchKernelGGL(k_match_list, dim3(max_blocks, n_mats, 1), dim3(kBlock), 0, st, mats, probs, blocks,
                     min_prob, out_i, out_j, out_p);
}

void launch_match_marginals(const MatchMat* mats, uint32_t n_mats, uint32_t max_side, const float* probs,
                            float* matched, hipStream_t st) {
  hipLaunchKernelGGL(k_match_marginals, dim3((max_side + kBlock - 1u) / kBlock, n_mats, 1), dim3(kBlock), 0, st,
                     mats, probs, matched);
}

void launch_match_align(const MatchMat* mats, uint32_t n_mats, const float* probs, const float* gammas,
                        uint32_t n_gammas, float* ws, int32_t* mate, uint32_t* n_matched, float* accuracy,
                        hipStream_t st) {
  hipLaunchKernelGGL(k_match_align, dim3(n_mats * n_gammas), dim3(kBlock), 0, st, mats, probs, gammas, n_gammas,
                     ws, mate, n_matched, accuracy);
}

}  // namespace rnamc
