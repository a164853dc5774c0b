// rnamc_context.hip — structural context profiles (rnamc_context_profile_batch):
// for every base the probability of being unpaired in a bulge, the exterior loop, a hairpin, an
// internal loop or a multibranch loop, off the matrices the reference-order sweep of a lock-step
// group leaves in its workspace.  Records of different lengths share every launch (grid.y).
//   k_ctx_save_qm  between the inside and the outside sweep: sums_multibranch (M_QM, whose slot the
//                  outside sweep reuses) into the entry's own buffer, column-major like M_Q1C:
//                  M2(r, c), r >= 1, at col_off(c) + r - 1
// and behind k_finalize:
//   k_ctx_wcol     lw(i, k) = (log p + mbclose) - Qb of every pair of the finished triangle (p its
//                  value there, like everywhere in this file; the W of the outside sweep up to the
//                  reference's approximate exp), in f64 into the dead M_W and M_P slots, column-major:
//                  (i, k) at col_off(k) + i; -inf where there is no pair or p = 0
//   k_ctx_loops    hairpins and 2-loops.  A workgroup takes 256 consecutive cells of the packed
//                  triangle and compacts the closing pairs with p >= 2^-45 (half a quantum; p is the
//                  finished triangle's value, so a pair's loops add up to what row 5 holds of it)
//                  before any scoring; a wave then owns one closing pair: lane 0 its hairpin
//                  p exp(hairpin - Qb), all lanes its <= 495 enclosed pairs, p exp(Qb(k,l) + twoloop -
//                  Qb) (Turner::twoloop / Contra::twoloop of rnamc_scoring.h).
//                  Every loop's probability is rounded ONCE to an integer of 2^-44 (rint, capped at
//                  2^45, the quantum of rnamc_align.hip) and summed in LDS per class {bulge, internal}
//                  by left length a and right length b; the wave then issues at most 2 x 2 x 31
//                  64-bit integer atomics into the record's DIFFERENCE rows (+ at the first base of a
//                  range, - one past its last), never one per loop.  A stack reaches no base.
//   k_ctx_ext      exterior[u] = exp(Z(0,u-1) + Z(u+1,n-1) + c_e - ln Z), a lane per base
//   k_ctx_mb13     multibranch, branches on both sides of u and all on the left: a wave per base u,
//                  lanes over i along column u - 1 of M1 / M2 and column u of {PM, PM2}
//   k_ctx_mb2      multibranch, all branches right of u: a lane per column k walks u upwards with
//                  V(u+1,k) = e^{c_m} V(u,k) + w(u,k) (f64 logarithms), the wave's terms of a step
//                  summed as integers across lanes and added by one lane
//   k_ctx_finish   integer prefix sums of the three difference rows, the multibranch row as it is,
//                  value = (float)(sum / 2^44)
// Integer adds commute: every output bit is independent of grouping, batch order, device count and
// run.  No floating-point atomics.  Every exponential is expf of a sum of the sweep's f32
// logarithms, the sum formed in f64 and rounded once; quantisation adds at most (number of loops
// over a base) * 2^-45 per base, about 6e-5 for a base under every loop a record of 65 535 bases
// can hold.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rnamc_device.h"
#include "rnamc_scoring.h"

namespace rnamc {

namespace {

constexpr uint32_t kBlock = 256u;
constexpr double kQuantum = 17592186044416.0;     // 2^44
constexpr double kQuantumCap = 35184372088832.0;  // 2^45
constexpr float kHalfQuantum = 2.8421709e-14f;    // 2^-45
constexpr uint32_t kSlots = RNAMC_MAX_2LOOP_LEN + 1u;                // 31 lengths 0 .. 30
constexpr uint32_t kProbes = kSlots * (kSlots + 1u) / 2u;            // 496 (a, b), a + b <= 30
using u64 = unsigned long long;

__device__ __forceinline__ uint64_t tri_off(uint64_t n, uint64_t d) { return d * n - ((d * (d - 1ull)) >> 1); }

// column-major packed triangle of the sweep (rnamc_kernels.hip): column j starts here
__device__ __forceinline__ uint32_t col_off(uint32_t j) {
  const uint32_t m = j >> 4, r = j & 15u;
  return 16u * (m + 1u) * (8u * m + r);
}

// a probability as an integer of 2^-44: to nearest, ties to even, capped; 0 for anything not positive
__device__ __forceinline__ u64 quant(double q) {
  if (!(q > 0.0)) return 0ull;
  return static_cast<u64>(static_cast<long long>(fmin(rint(q * kQuantum), kQuantumCap)));
}

// the diagonal of packed cell x: the largest d in [0, n-1] with tri_off(d) <= x
__device__ __forceinline__ uint32_t diag_of(uint32_t n, uint64_t x) {
  uint32_t lo = 0u, hi = n - 1u;
  while (lo < hi) {
    const uint32_t mid = (lo + hi + 1u) >> 1;
    if (tri_off(n, mid) <= x) lo = mid; else hi = mid - 1u;
  }
  return lo;
}

__device__ __forceinline__ const float* mat(const ContextBatch& b, const SeqDesc& sd, int which) {
  return b.workspace + sd.ws_off + static_cast<size_t>(which) * sd.tri_pad;
}

// lw, column-major, as f64 over the two dead slots M_W and M_P (adjacent; finalize has read M_P)
static_assert(M_P == M_W + 1, "lw takes two adjacent slots");
__device__ __forceinline__ double* wcol_of(const ContextBatch& b, const SeqDesc& sd) {
  return reinterpret_cast<double*>(b.workspace + sd.ws_off + static_cast<size_t>(M_W) * sd.tri_pad);
}

// expf of a sum of logarithms formed in f64 (the terms are hundreds of nats and cancel: the f32 sum
// would carry an ulp of its largest term, 6e-5 at 512 nats, into the probability)
__device__ __forceinline__ float exp_of(double x) { return expf(static_cast<float>(x)); }

template <bool CONTRA>
__device__ __forceinline__ auto model_of(const ContextBatch& b) {
  if constexpr (CONTRA) {
    return Contra{b.params->contra};
  } else {
    return Turner{b.params->turner, b.hp_init};
  }
}

__device__ __forceinline__ u64 wave_sum(u64 v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += static_cast<u64>(__shfl_xor(static_cast<long long>(v), s));
  return v;
}

__global__ void __launch_bounds__(kBlock) k_ctx_save_qm(ContextBatch b) {
  const SeqDesc sd = b.seqs[blockIdx.y];
  const uint32_t n = sd.n;
  const uint64_t x = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (x >= tri_off(n, n)) return;
  const uint32_t d = diag_of(n, x);
  const uint32_t r = static_cast<uint32_t>(x - tri_off(n, d));
  if (r == 0u) return;
  b.qm[b.items[blockIdx.y].qm_off + col_off(r + d) + r - 1u] = mat(b, sd, M_QM)[x];
}

__global__ void __launch_bounds__(kBlock) k_ctx_wcol(ContextBatch b) {
  const SeqDesc sd = b.seqs[blockIdx.y];
  const uint32_t n = sd.n;
  const uint64_t x = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (x >= tri_off(n, n)) return;
  const uint32_t d = diag_of(n, x);
  const uint32_t i = static_cast<uint32_t>(x - tri_off(n, d));
  const float p = d >= 1u ? b.bpp[sd.out_off + x] : -1.f;
  const double lw = p > 0.f ? log(static_cast<double>(p)) + static_cast<double>(mat(b, sd, M_MBC)[x]) -
                                  static_cast<double>(mat(b, sd, M_QB)[x])
                            : -__builtin_inf();
  wcol_of(b, sd)[col_off(i + d) + i] = lw;
}

template <bool CONTRA>
__global__ void __launch_bounds__(kBlock) k_ctx_loops(ContextBatch b) {
  __shared__ uint32_t act_i[kBlock], act_j[kBlock];
  __shared__ float act_p[kBlock], act_qb[kBlock];
  __shared__ uint32_t wsum[kBlock / 64u];
  __shared__ u64 S[kBlock / 64u][2][2][32];  // wave, class, side (0 left, 1 right), length
  __shared__ uint16_t ab[kProbes];
  const SeqDesc sd = b.seqs[blockIdx.y];
  const uint32_t n = sd.n;
  const uint64_t len = tri_off(n, n);
  if (static_cast<uint64_t>(blockIdx.x) * kBlock >= len) return;  // (the whole workgroup)
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  for (uint32_t t = threadIdx.x; t < kProbes; t += kBlock) {
    uint32_t a = 0u, rem = t;
    while (rem >= kSlots - a) {
      rem -= kSlots - a;
      a++;
    }
    ab[t] = static_cast<uint16_t>(a | (rem << 8));
  }
  for (uint32_t t = lane; t < 128u; t += 64u) (&S[wave][0][0][0])[t] = 0ull;
  // this lane's cell: a pair of the finished triangle (absent: -1) with p >= half a quantum?
  const uint64_t x = static_cast<uint64_t>(blockIdx.x) * kBlock + threadIdx.x;
  const float p = (x >= n && x < len) ? b.bpp[sd.out_off + x] : -1.f;
  const bool flag = p >= kHalfQuantum;
  const uint64_t mask = __ballot(flag);
  if (lane == 0u) wsum[wave] = static_cast<uint32_t>(__popcll(mask));
  __syncthreads();
  uint32_t n_act = 0u, rank = __builtin_amdgcn_mbcnt_hi(static_cast<uint32_t>(mask >> 32),
                                                         __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(mask), 0u));
  for (uint32_t w = 0u; w < kBlock / 64u; w++) {
    if (w < wave) rank += wsum[w];
    n_act += wsum[w];
  }
  if (flag) {
    const uint32_t d = diag_of(n, x);
    const uint32_t i = static_cast<uint32_t>(x - tri_off(n, d));
    act_i[rank] = i;
    act_j[rank] = i + d;
    act_p[rank] = p;
    act_qb[rank] = mat(b, sd, M_QB)[x];
  }
  __syncthreads();
  const uint8_t* s = b.bases + sd.seq_off;
  const float* qbm = mat(b, sd, M_QB);
  u64* acc = b.acc + b.items[blockIdx.y].acc_off;
  const uint64_t row = static_cast<uint64_t>(n) + 1ull;  // entries of an accumulator row
  const auto model = model_of<CONTRA>(b);
  // every wave runs every round (the barriers order a wave's LDS sums and their readers)
  for (uint32_t c0 = 0u; c0 < n_act; c0 += kBlock / 64u) {
    const uint32_t c = c0 + wave;
    const bool live = c < n_act;
    const uint32_t i = live ? act_i[c] : 0u, j = live ? act_j[c] : 0u;
    const double p_ij = live ? static_cast<double>(act_p[c]) : 0.0;
    const double qb_ij = live ? static_cast<double>(act_qb[c]) : 0.0;
    if (live) {
      if (lane == 0u && j - i >= 2u && (!CONTRA || j - i - 1u <= RNAMC_MAX_LOOP_LEN)) {
        const u64 q = quant(p_ij * exp_of(static_cast<double>(model.hairpin(s, n, i, j)) - qb_ij));
        if (q) {
          atomicAdd(acc + CTX_ACC_HAIRPIN * row + i + 1u, q);
          atomicAdd(acc + CTX_ACC_HAIRPIN * row + j, 0ull - q);
        }
      }
      for (uint32_t t = 1u + lane; t < kProbes; t += 64u) {  // (t = 0 is the stack)
        const uint32_t a = ab[t] & 255u, bb = ab[t] >> 8;
        const uint32_t k = i + 1u + a;
        if (k + 1u + bb >= j) continue;  // l = j - 1 - bb must lie right of k
        const uint32_t l = j - 1u - bb;
        const float qb_kl = qbm[tri_off(n, l - k) + k];
        if (!(qb_kl > kNegInf)) continue;
        const double sc = static_cast<double>(model.twoloop(s, i, j, k, l));
        const u64 q = quant(p_ij * exp_of(static_cast<double>(qb_kl) + sc - qb_ij));
        if (!q) continue;
        const uint32_t cls = (a == 0u || bb == 0u) ? 0u : 1u;
        if (a) atomicAdd(&S[wave][cls][0][a], q);
        if (bb) atomicAdd(&S[wave][cls][1][bb], q);
      }
    }
    __syncthreads();
    if (live && lane < 2u * kSlots) {
      const uint32_t cls = lane / kSlots, sl = lane - cls * kSlots;
      u64* r = acc + (cls == 0u ? CTX_ACC_BULGE : CTX_ACC_INTERNAL) * row;
      if (sl == 0u) {
        // a loop with a >= 1 starts its left range at i + 1; one with b >= 1 ends its right range at j - 1
        u64 tl = 0ull, tr = 0ull;
        for (uint32_t y = 1u; y < kSlots; y++) {
          tl += S[wave][cls][0][y];
          tr += S[wave][cls][1][y];
        }
        if (tl) atomicAdd(r + i + 1u, tl);
        if (tr) atomicAdd(r + j, 0ull - tr);
      } else {
        const u64 vl = S[wave][cls][0][sl], vr = S[wave][cls][1][sl];
        if (vl) atomicAdd(r + i + 1u + sl, 0ull - vl);  // left range i + 1 .. i + a
        if (vr) atomicAdd(r + j - sl, vr);              // right range j - b .. j - 1
      }
    }
    __syncthreads();
    for (uint32_t t = lane; t < 128u; t += 64u) (&S[wave][0][0][0])[t] = 0ull;
    __syncthreads();
  }
}

template <bool CONTRA>
__global__ void __launch_bounds__(kBlock) k_ctx_ext(ContextBatch b) {
  const SeqDesc sd = b.seqs[blockIdx.y];
  const uint32_t n = sd.n;
  const uint32_t u = blockIdx.x * kBlock + threadIdx.x;
  if (u >= n) return;
  const float* z = mat(b, sd, M_Z);
  const float zl = u < 1u ? 0.f : z[tri_off(n, u - 1u)];                       // Z(0, u-1)
  const float zr = u + 2u > n ? 0.f : z[tri_off(n, n - 2u - u) + u + 1u];  // Z(u+1, n-1)
  const float ce = CONTRA ? b.params->contra.external_score_unpair : 0.f;
  b.out[b.items[blockIdx.y].out_off + static_cast<uint64_t>(CTX_ROW_EXTERIOR) * n + u] =
      exp_of(static_cast<double>(zl) + static_cast<double>(zr) + static_cast<double>(ce) -
             static_cast<double>(z[tri_off(n, n - 1u)]));
}

template <bool CONTRA>
__global__ void __launch_bounds__(kBlock) k_ctx_mb13(ContextBatch b) {
  const SeqDesc sd = b.seqs[blockIdx.y];
  const uint32_t n = sd.n;
  const uint32_t u = blockIdx.x * (kBlock / 64u) + (threadIdx.x >> 6);
  if (u >= n || u < 2u) return;  // (a whole wave)
  const uint32_t lane = threadIdx.x & 63u;
  const ContextItem it = b.items[blockIdx.y];
  const double cm = CONTRA ? static_cast<double>(b.params->contra.multibranch_score_unpair) : 0.0;
  const float* __restrict__ q1 = mat(b, sd, M_Q1C) + col_off(u - 1u);       // M1(i+1, u-1) at [i]
  const float* __restrict__ q2 = b.qm + it.qm_off + col_off(u - 1u);        // M2(i+1, u-1) at [i]
  const float2* __restrict__ pm = reinterpret_cast<const float2*>(mat(b, sd, M_PM)) + col_off(u);  // {PM, PM2}(i, u)
  u64 sum = 0ull;
  for (uint32_t i = lane; i + 2u <= u; i += 64u) {
    const float2 y = pm[i];
    sum += quant(exp_of(static_cast<double>(q1[i]) + static_cast<double>(y.x) + cm));
    sum += quant(exp_of(static_cast<double>(q2[i]) + static_cast<double>(y.y) + cm));
  }
  sum = wave_sum(sum);
  if (lane == 0u && sum) atomicAdd(b.acc + it.acc_off + CTX_ACC_MULTI * (static_cast<uint64_t>(n) + 1ull) + u, sum);
}

template <bool CONTRA>
__global__ void __launch_bounds__(kBlock) k_ctx_mb2(ContextBatch b) {
  const SeqDesc sd = b.seqs[blockIdx.y];
  const uint32_t n = sd.n;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t k0 = blockIdx.x * kBlock + threadIdx.x - lane;  // the wave's first column
  if (k0 >= n) return;
  const uint32_t k = k0 + lane;
  const bool valid = k < n && k >= 2u;
  const uint32_t kmax = min(k0 + 63u, n - 1u);  // the wave walks to its last column's end
  const ContextItem it = b.items[blockIdx.y];
  const double cm = CONTRA ? static_cast<double>(b.params->contra.multibranch_score_unpair) : 0.0;
  const double* __restrict__ wc = wcol_of(b, sd) + col_off(valid ? k : 0u);            // lw(u, k) at [u]
  const float* __restrict__ q2 = b.qm + it.qm_off + col_off(valid ? k - 1u : 0u);      // M2(u+1, k-1) at [u]
  u64* acc = b.acc + it.acc_off + CTX_ACC_MULTI * (static_cast<uint64_t>(n) + 1ull);
  double lv = -__builtin_inf();  // ln V(u, k), V(0, k) = 0
  for (uint32_t u = 0u; u + 2u <= kmax; u++) {
    u64 q = 0ull;
    if (valid && u + 2u <= k) {
      if (lv > -__builtin_inf()) q = quant(exp_of(static_cast<double>(q2[u]) + lv + cm));
      const double w = wc[u];
      const double a = lv + cm;
      if (w > -__builtin_inf()) {
        const double hi = fmax(a, w), lo = fmin(a, w);
        lv = lo > -__builtin_inf() ? hi + log1p(exp(lo - hi)) : hi;
      } else {
        lv = a;
      }
    }
    if (__ballot(q != 0ull) == 0ull) continue;  // wave-uniform
    q = wave_sum(q);
    if (lane == 0u) atomicAdd(acc + u, q);
  }
}

__global__ void __launch_bounds__(kBlock) k_ctx_finish(ContextBatch b) {
  __shared__ long long buf[kBlock];
  const SeqDesc sd = b.seqs[blockIdx.x];
  const uint32_t n = sd.n;
  const ContextItem it = b.items[blockIdx.x];
  const uint64_t row = static_cast<uint64_t>(n) + 1ull;
  const long long* acc = reinterpret_cast<const long long*>(b.acc + it.acc_off);
  float* out = b.out + it.out_off;
  const int acc_rows[3] = {CTX_ACC_BULGE, CTX_ACC_HAIRPIN, CTX_ACC_INTERNAL};
  const int out_rows[3] = {CTX_ROW_BULGE, CTX_ROW_HAIRPIN, CTX_ROW_INTERNAL};
  for (int r = 0; r < 3; r++) {
    const long long* a = acc + acc_rows[r] * row;
    long long carry = 0;
    for (uint32_t x0 = 0u; x0 < n; x0 += kBlock) {
      const uint32_t x = x0 + threadIdx.x;
      buf[threadIdx.x] = x < n ? a[x] : 0ll;
      __syncthreads();
      for (uint32_t s = 1u; s < kBlock; s <<= 1) {  // inclusive scan (Hillis-Steele), two barriers a step
        const long long add = threadIdx.x >= s ? buf[threadIdx.x - s] : 0ll;
        __syncthreads();
        buf[threadIdx.x] += add;
        __syncthreads();
      }
      if (x < n)
        out[static_cast<uint64_t>(out_rows[r]) * n + x] =
            static_cast<float>(static_cast<double>(carry + buf[threadIdx.x]) / kQuantum);
      carry += buf[kBlock - 1u];
      __syncthreads();  // (buf is rewritten by the next step)
    }
  }
  const long long* m = acc + CTX_ACC_MULTI * row;
  for (uint32_t x = threadIdx.x; x < n; x += kBlock)
    out[static_cast<uint64_t>(CTX_ROW_MULTI) * n + x] = static_cast<float>(static_cast<double>(m[x]) / kQuantum);
}

dim3 cells_grid(uint32_t max_n, uint32_t n_items) {
  const uint64_t len = static_cast<uint64_t>(max_n) * (max_n + 1ull) / 2ull;
  return dim3(static_cast<uint32_t>((len + kBlock - 1u) / kBlock), n_items, 1);
}

}  // namespace

// (grid.y carries the records: at most 65535 of them a launch, the longest first; b.seqs and
// b.items point at the launch's first record)
void launch_context_save(const ContextBatch& b, uint32_t n_items, uint32_t max_n, hipStream_t st) {
  hipLaunchKernelGGL(k_ctx_save_qm, cells_grid(max_n, n_items), dim3(kBlock), 0, st, b);
}

uint32_t launch_context_profile(const ContextBatch& b, bool contra, uint32_t n_items, uint32_t max_n,
                                hipStream_t st) {
  const dim3 cells = cells_grid(max_n, n_items), blk(kBlock);
  const dim3 bases((max_n + kBlock - 1u) / kBlock, n_items, 1);
  const dim3 waves((max_n + kBlock / 64u - 1u) / (kBlock / 64u), n_items, 1);
  hipLaunchKernelGGL(k_ctx_wcol, cells, blk, 0, st, b);
  if (contra) {
    hipLaunchKernelGGL(k_ctx_loops<true>, cells, blk, 0, st, b);
    hipLaunchKernelGGL(k_ctx_ext<true>, bases, blk, 0, st, b);
    hipLaunchKernelGGL(k_ctx_mb13<true>, waves, blk, 0, st, b);
    hipLaunchKernelGGL(k_ctx_mb2<true>, bases, blk, 0, st, b);
  } else {
    hipLaunchKernelGGL(k_ctx_loops<false>, cells, blk, 0, st, b);
    hipLaunchKernelGGL(k_ctx_ext<false>, bases, blk, 0, st, b);
    hipLaunchKernelGGL(k_ctx_mb13<false>, waves, blk, 0, st, b);
    hipLaunchKernelGGL(k_ctx_mb2<false>, bases, blk, 0, st, b);
  }
  hipLaunchKernelGGL(k_ctx_finish, dim3(n_items), blk, 0, st, b);
  return 6u;
}

}  // namespace rnamc
