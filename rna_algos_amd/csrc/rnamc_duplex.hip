// rnamc_duplex.hip — RNA-RNA duplex folding (include/rnamc.h): inside, outside
// and max-plus sweeps of a chunk of strand pairs, one lane per cell and one launch per line; the
// reductions behind them (ln Z, best score and its cell), the probabilities and the traceback.
//
// A cell (i, j) pairs A[i] with B[j].  Inside, F(i, j) reads F(k, l) with k = i + 1 + a, l = j - 1 - b,
// a + b <= 30; outside, G(k, l) reads G(i, j) with i = k - 1 - a, j = l + 1 + b.  A sweep steps along
// one strand (the "line" coordinate u) and runs a lane per position of the other (the "lane"
// coordinate v); a workgroup owns 128 consecutive lanes and stages the 31 lines x (128 + 30) lanes
// of the matrix it reads in LDS.  Which strand is stepped along is the host's choice per chunk; the
// terms of a cell are the same values added in the same order, (a, b) ascending, either way.
//
// Arithmetic.  A loop score is f32.  The log-domain values F, G and ln Z are f64: a long helix reaches
// hundreds of nats, where one f32 ulp per cell (1.5e-5 at 160) would add up to 1e-4 in the
// probabilities.  A sum keeps its running maximum in f64 and adds, per term, one hardware exp2 of the
// term's f32 distance to that maximum; the closing logarithm is one hardware log2.  The max-plus
// matrix M is f32 throughout (its value and its ties are f32 by contract).
#include <type_traits>

#include "rnamc_device.h"
#include "rnamc_scoring.h"

namespace rnamc {
namespace {

constexpr uint32_t kBlock = 128u;  // lanes of a sweep workgroup
constexpr uint32_t kRed = 256u;    // threads of a reduction workgroup
constexpr int kMaxLoop = RNAMC_MAX_2LOOP_LEN;         // a + b <= 30
constexpr uint32_t kWin = RNAMC_MAX_2LOOP_LEN + 1u;   // lines a cell reads
constexpr uint32_t kTileW = kBlock + RNAMC_MAX_2LOOP_LEN;
constexpr int kHalo = 36;  // bases staged either side of the workgroup's lines and lanes (31 + 2 needed)
constexpr float kL2E = 1.44269504088896340736f, kLn2 = 0.693147180559945309417f;
constexpr uint32_t kNone = 0xffffffffu;

__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }
__device__ __forceinline__ float lg2(float x) { return __builtin_amdgcn_logf(x); }

constexpr double kNegInfD = -__builtin_inf();
// exp(d) for d <= 0 (or -inf): one hardware exp2 of the f32 distance
__device__ __forceinline__ double exp_of(double d) { return static_cast<double>(ex2(static_cast<float>(d) * kL2E)); }
// Sum of exp(x_t) held as s * exp(m), m >= every x_t seen; only finite terms are added.
struct Acc {
  double m, s;
};
__device__ __forceinline__ void acc_add(Acc& a, double x) {
  const double mn = fmax(a.m, x);
  a.s = __builtin_fma(a.s, exp_of(a.m - mn), exp_of(x - mn));
  a.m = mn;
}
__device__ __forceinline__ double acc_value(const Acc& a) {
  return a.s > 0.0 ? a.m + static_cast<double>(lg2(static_cast<float>(a.s)) * kLn2) : kNegInfD;
}

// base x of a strand, 0 outside it (a flat 2-loop form reads every index it might need)
struct GlobalBases {
  const uint8_t* p;
  int n;
  __device__ __forceinline__ int operator()(int x) const { return (x >= 0 && x < n) ? p[x] : 0; }
};
// the same out of a staged window [org, org + len): the caller stays inside it
struct LdsBases {
  const uint8_t* s;
  int org;
  __device__ __forceinline__ int operator()(int x) const { return s[x - org]; }
};

// accessible(S, nA + nB, i, nA + j)
template <class BA, class BB>
__device__ __forceinline__ float outer_end(const rnamc_params* P, bool contra, const BA& A, const BB& B, int na,
                                           int nb, int i, int j) {
  const int ai = A(i), bj = B(j);
  const bool hp = i > 0, hn = j < nb - 1;
  const int prev = A(i - 1), next = B(j + 1);
  if (contra) return Contra{P->contra}.junction_codes(bj, ai, hn, next, hp, prev) + P->contra.basepair_scores[ai][bj];
  return Turner{P->turner, nullptr}.accessible_codes(ai, bj, hp, prev, hn, next);
}
// Turner accessible(R, nA + nB, j, nB + i); CONTRAfold junction(R, nA + nB, nB + i, j)
template <class BA, class BB>
__device__ __forceinline__ float inner_end(const rnamc_params* P, bool contra, const BA& A, const BB& B, int na,
                                           int nb, int i, int j) {
  const int ai = A(i), bj = B(j);
  const bool hp = j > 0, hn = i < na - 1;
  const int prev = B(j - 1), next = A(i + 1);
  if (contra) return Contra{P->contra}.junction_codes(ai, bj, hn, next, hp, prev);
  return Turner{P->turner, nullptr}.accessible_codes(bj, ai, hp, prev, hn, next);
}
// twoloop(S, i, nA + j, k, nA + l): (A[i], B[j]) closes, (A[k], B[l]) is enclosed
template <class BA, class BB>
__device__ __forceinline__ float duplex_twoloop(const rnamc_params* P, bool contra, const BA& A, const BB& B, int i,
                                                int j, int k, int l) {
  const uint32_t a = static_cast<uint32_t>(k - i - 1), b = static_cast<uint32_t>(j - l - 1);
  const int ci = A(i), cj = B(j), ak = A(k), al = B(l);
  const int x1 = A(i + 1), x2 = A(i + 2), y1 = B(j - 1), y2 = B(j - 2), m2 = B(l + 1), m3 = A(k - 1);
  return contra ? contra_twoloop_flat(P->contra, a, b, ci, cj, x1, y1, ak, al, m2, m3)
                : turner_twoloop_flat(P->turner, a, b, ci, cj, x1, x2, y1, y2, ak, al, m2, m3);
}

// F and G are f64 (their float offsets are even), M is f32
__device__ __forceinline__ double* sum_matrix_of(const DuplexChunk& c, const DuplexPair& p, int what) {
  return reinterpret_cast<double*>(c.ws + (what == 0 ? p.f_off : p.g_off));
}
__device__ __forceinline__ float* max_matrix_of(const DuplexChunk& c, const DuplexPair& p) { return c.ws + p.m_off; }
// storage index of cell (i, j)
__device__ __forceinline__ uint64_t cell_at(const DuplexChunk& c, const DuplexPair& p, uint32_t i, uint32_t j) {
  return c.by_col ? static_cast<uint64_t>(j) * p.na + i : static_cast<uint64_t>(i) * p.nb + j;
}

// WHAT: 0 inside (sum), 1 outside (sum), 2 inside (max).  COL: lines are positions of B.
// FWD: the cell reads lines AHEAD of its own (u + 1 + x) at lanes BELOW its own (v - 1 - y): the
// inside sweep along A and the outside sweep along B; the other two read lines behind, lanes above.
template <int WHAT, bool COL>
__global__ __launch_bounds__(128) void k_duplex_step(DuplexChunk c, uint32_t step) {
  using T = typename std::conditional<WHAT == 2, float, double>::type;
  constexpr bool OUT = WHAT == 1;
  constexpr bool FWD = OUT == COL;
  const DuplexPair p = c.pairs[blockIdx.y];
  const uint32_t nU = COL ? p.nb : p.na, nV = COL ? p.na : p.nb;
  const uint32_t v0 = blockIdx.x * kBlock;
  if (step >= nU || v0 >= nV) return;
  const uint32_t u = FWD ? nU - 1u - step : step;
  const uint32_t tid = threadIdx.x;
  T* M;
  if constexpr (WHAT == 2) M = max_matrix_of(c, p);
  else M = sum_matrix_of(c, p, WHAT);
  const T ninf = static_cast<T>(kNegInf);

  __shared__ T tile[kWin][kTileW];
  __shared__ uint8_t sU[2 * kHalo + 1];
  __shared__ uint8_t sV[kBlock + 2 * kHalo];
  const int64_t vorg = FWD ? static_cast<int64_t>(v0) - kMaxLoop - 1 : static_cast<int64_t>(v0) + 1;
  for (uint32_t x = 0; x < kWin; x++) {
    const int64_t line = FWD ? static_cast<int64_t>(u) + 1 + x : static_cast<int64_t>(u) - 1 - x;
    const bool line_ok = line >= 0 && line < static_cast<int64_t>(nU);
    for (uint32_t cc = tid; cc < kTileW; cc += kBlock) {
      const int64_t v = vorg + cc;
      T val = ninf;
      if (line_ok && v >= 0 && v < static_cast<int64_t>(nV)) val = M[static_cast<uint64_t>(line) * nV + static_cast<uint64_t>(v)];
      tile[x][cc] = val;
    }
  }
  const uint8_t* gU = c.bases + (COL ? p.b_off : p.a_off);
  const uint8_t* gV = c.bases + (COL ? p.a_off : p.b_off);
  const int uorg = static_cast<int>(u) - kHalo, vbase = static_cast<int>(v0) - kHalo;
  for (uint32_t x = tid; x < 2u * kHalo + 1u; x += kBlock) {
    const int q = uorg + static_cast<int>(x);
    sU[x] = (q >= 0 && q < static_cast<int>(nU)) ? gU[q] : 0;
  }
  for (uint32_t x = tid; x < kBlock + 2u * kHalo; x += kBlock) {
    const int q = vbase + static_cast<int>(x);
    sV[x] = (q >= 0 && q < static_cast<int>(nV)) ? gV[q] : 0;
  }
  __syncthreads();

  const uint32_t v = v0 + tid;
  if (v >= nV) return;
  const LdsBases A{COL ? sV : sU, COL ? vbase : uorg}, B{COL ? sU : sV, COL ? uorg : vbase};
  const int na = static_cast<int>(p.na), nb = static_cast<int>(p.nb);
  const int i = static_cast<int>(COL ? v : u), j = static_cast<int>(COL ? u : v);
  const bool contra = c.contra != 0;
  const rnamc_params* P = c.params;
  T out = ninf;
  if (canonical(A(i), B(j))) {
    // the end term first, then the 2-loops in (a, b) ascending order
    const float first = OUT ? outer_end(P, contra, A, B, na, nb, i, j) : inner_end(P, contra, A, B, na, nb, i, j);
    Acc acc{kNegInfD, 0.0};
    float best = first;
    if (WHAT != 2 && first > kNegInf) acc_add(acc, static_cast<double>(first));
    for (int a = 0; a <= kMaxLoop; a++) {
      // the other pair of the 2-loop: enclosed (k, l) inside, closing (k, l) outside
      const int k = OUT ? i - 1 - a : i + 1 + a;
      if (k < 0 || k >= na) break;
      for (int b = 0; a + b <= kMaxLoop; b++) {
        const int l = OUT ? j + 1 + b : j - 1 - b;
        if (l < 0 || l >= nb) break;
        const int x = COL ? b : a, y = COL ? a : b;
        const T other = tile[x][FWD ? tid + kMaxLoop - y : tid + y];
        if (!(other > ninf)) continue;
        const float sc = OUT ? duplex_twoloop(P, contra, A, B, k, l, i, j) : duplex_twoloop(P, contra, A, B, i, j, k, l);
        const T term = static_cast<T>(sc) + other;  // (f32 + f32 under max-plus, f64 in the sums)
        if constexpr (WHAT == 2) {
          best = fmaxf(best, term);
        } else {
          if (term > ninf) acc_add(acc, term);
        }
      }
    }
    if constexpr (WHAT == 2) out = best;
    else out = acc_value(acc);
  }
  M[static_cast<uint64_t>(u) * nV + v] = out;
}

// x(cell) = outer_end + matrix over the cells in ROW-major order i * nB + j, whatever the storage:
// thread t takes cells t, t + 256, ... in order, then a fixed tree over the 256 partial results.
// WHAT 0: ln Z = lse of x over F; WHAT 2: max of x over M and its first cell.
template <int WHAT>
__global__ __launch_bounds__(256) void k_duplex_reduce(DuplexChunk c) {
  const DuplexPair p = c.pairs[blockIdx.x];
  const uint32_t tid = threadIdx.x;
  const uint64_t cells = static_cast<uint64_t>(p.na) * p.nb;
  const double* F = sum_matrix_of(c, p, 0);
  const float* M = max_matrix_of(c, p);
  const GlobalBases A{c.bases + p.a_off, static_cast<int>(p.na)}, B{c.bases + p.b_off, static_cast<int>(p.nb)};
  const bool contra = c.contra != 0;
  __shared__ double red[kRed];
  __shared__ uint64_t red_at[kRed];
  // f32 + f32 under max-plus (exact in the f64 it is carried in), f32 + f64 for ln Z
  auto value = [&](uint64_t cell) -> double {
    const uint32_t i = static_cast<uint32_t>(cell / p.nb), j = static_cast<uint32_t>(cell % p.nb);
    const uint64_t at = cell_at(c, p, i, j);
    const bool live = WHAT == 2 ? M[at] > kNegInf : F[at] > kNegInfD;
    if (!live) return kNegInfD;
    const float oe = outer_end(c.params, contra, A, B, static_cast<int>(p.na), static_cast<int>(p.nb),
                               static_cast<int>(i), static_cast<int>(j));
    return WHAT == 2 ? static_cast<double>(oe + M[at]) : static_cast<double>(oe) + F[at];
  };
  double mx = kNegInfD;
  uint64_t at = ~0ull;
  for (uint64_t cell = tid; cell < cells; cell += kRed) {
    const double x = value(cell);
    if (x > mx) {
      mx = x;
      at = cell;
    }
  }
  red[tid] = mx;
  red_at[tid] = at;
  __syncthreads();
  for (uint32_t h = kRed / 2u; h > 0u; h >>= 1) {
    if (tid < h) {
      const double o = red[tid + h];
      const uint64_t oa = red_at[tid + h];
      if (o > red[tid] || (o == red[tid] && oa < red_at[tid])) {
        red[tid] = o;
        red_at[tid] = oa;
      }
    }
    __syncthreads();
  }
  mx = red[0];
  at = red_at[0];
  __syncthreads();
  if (WHAT == 2) {
    if (tid == 0) {
      DuplexRes& r = c.res[blockIdx.x];
      r.best = static_cast<float>(mx);
      r.start_i = mx > kNegInfD ? static_cast<uint32_t>(at / p.nb) : kNone;
      r.start_j = mx > kNegInfD ? static_cast<uint32_t>(at % p.nb) : kNone;
    }
    return;
  }
  double s = 0.0;
  if (mx > kNegInfD)
    for (uint64_t cell = tid; cell < cells; cell += kRed) {
      const double x = value(cell);
      if (x > kNegInfD) s += exp_of(x - mx);
    }
  red[tid] = s;
  __syncthreads();
  for (uint32_t h = kRed / 2u; h > 0u; h >>= 1) {
    if (tid < h) red[tid] += red[tid + h];
    __syncthreads();
  }
  if (tid == 0)
    c.res[blockIdx.x].log_z = mx > kNegInfD ? mx + static_cast<double>(lg2(static_cast<float>(red[0])) * kLn2) : kNegInfD;
}

// P(i, j) = exp(F + G - ln Z), 0 where either is -inf
__device__ __forceinline__ float duplex_prob(double f, double g, double log_z) {
  if (!(f > kNegInfD) || !(g > kNegInfD)) return 0.f;
  return ex2(static_cast<float>((f + g) - log_z) * kL2E);
}

__global__ __launch_bounds__(256) void k_duplex_probs(DuplexChunk c) {
  const DuplexPair p = c.pairs[blockIdx.y];
  const uint64_t cell = static_cast<uint64_t>(blockIdx.x) * kRed + threadIdx.x;
  if (cell >= static_cast<uint64_t>(p.na) * p.nb) return;
  const uint32_t i = static_cast<uint32_t>(cell / p.nb), j = static_cast<uint32_t>(cell % p.nb);
  const uint64_t at = cell_at(c, p, i, j);
  c.probs[p.prob_off + cell] =
      duplex_prob(sum_matrix_of(c, p, 0)[at], sum_matrix_of(c, p, 1)[at], c.res[blockIdx.y].log_z);
}

// pa[i] = sum_j P(i, j), pb[j] = sum_i P(i, j): a lane per base, its cells in ascending order in f64,
// rounded once
__global__ __launch_bounds__(256) void k_duplex_bound(DuplexChunk c) {
  const DuplexPair p = c.pairs[blockIdx.y];
  const uint32_t t = blockIdx.x * kRed + threadIdx.x;
  if (t >= p.na + p.nb) return;
  const double log_z = c.res[blockIdx.y].log_z;
  const double* F = sum_matrix_of(c, p, 0);
  const double* G = sum_matrix_of(c, p, 1);
  const bool is_a = t < p.na;
  const uint32_t fixed = is_a ? t : t - p.na, count = is_a ? p.nb : p.na;
  double sum = 0.0;
  for (uint32_t x = 0; x < count; x++) {
    const uint64_t at = is_a ? cell_at(c, p, fixed, x) : cell_at(c, p, x, fixed);
    sum += static_cast<double>(duplex_prob(F[at], G[at], log_z));
  }
  c.bound[p.bound_off + t] = static_cast<float>(sum);
}

// One workgroup of 64 per pair: dots, then lane 0 walks the chain from the start cell.  At a cell the
// inner end is the first candidate, then the enclosed pairs in (a, b) ascending order; a later
// candidate wins only when strictly larger.
__global__ __launch_bounds__(64) void k_duplex_trace(DuplexChunk c) {
  const DuplexPair p = c.pairs[blockIdx.x];
  uint8_t* row = c.structs + p.struct_off;
  for (uint32_t x = threadIdx.x; x < p.na + p.nb; x += 64u) row[x] = '.';
  __syncthreads();
  if (threadIdx.x != 0) return;
  const DuplexRes r = c.res[blockIdx.x];
  if (r.start_i == kNone) return;
  const GlobalBases A{c.bases + p.a_off, static_cast<int>(p.na)}, B{c.bases + p.b_off, static_cast<int>(p.nb)};
  const int na = static_cast<int>(p.na), nb = static_cast<int>(p.nb);
  const bool contra = c.contra != 0;
  const float* M = c.ws + p.m_off;
  int i = static_cast<int>(r.start_i), j = static_cast<int>(r.start_j);
  for (;;) {
    row[i] = '(';
    row[na + j] = ')';
    float best = inner_end(c.params, contra, A, B, na, nb, i, j);
    int bk = -1, bl = -1;
    for (int a = 0; a <= kMaxLoop; a++) {
      const int k = i + 1 + a;
      if (k >= na) break;
      for (int b = 0; a + b <= kMaxLoop; b++) {
        const int l = j - 1 - b;
        if (l < 0) break;
        const float m = M[cell_at(c, p, static_cast<uint32_t>(k), static_cast<uint32_t>(l))];
        if (!(m > kNegInf)) continue;
        const float term = duplex_twoloop(c.params, contra, A, B, i, j, k, l) + m;
        if (term > best) {
          best = term;
          bk = k;
          bl = l;
        }
      }
    }
    if (bk < 0) break;
    i = bk;
    j = bl;
  }
}

}  // namespace

void launch_duplex_step(const DuplexChunk& c, int what, uint32_t step, uint32_t max_lane, hipStream_t st) {
  const dim3 grid((max_lane + kBlock - 1u) / kBlock, c.n_pairs), block(kBlock);
  if (c.by_col) {
    if (what == 0) hipLaunchKernelGGL((k_duplex_step<0, true>), grid, block, 0, st, c, step);
    else if (what == 1) hipLaunchKernelGGL((k_duplex_step<1, true>), grid, block, 0, st, c, step);
    else hipLaunchKernelGGL((k_duplex_step<2, true>), grid, block, 0, st, c, step);
  } else {
    if (what == 0) hipLaunchKernelGGL((k_duplex_step<0, false>), grid, block, 0, st, c, step);
    else if (what == 1) hipLaunchKernelGGL((k_duplex_step<1, false>), grid, block, 0, st, c, step);
    else hipLaunchKernelGGL((k_duplex_step<2, false>), grid, block, 0, st, c, step);
  }
}

void launch_duplex_reduce(const DuplexChunk& c, int what, hipStream_t st) {
  if (what == 2) hipLaunchKernelGGL(k_duplex_reduce<2>, dim3(c.n_pairs), dim3(kRed), 0, st, c);
  else hipLaunchKernelGGL(k_duplex_reduce<0>, dim3(c.n_pairs), dim3(kRed), 0, st, c);
}

void launch_duplex_probs(const DuplexChunk& c, uint64_t max_cells, uint32_t max_bases, hipStream_t st) {
  if (c.probs)
    hipLaunchKernelGGL(k_duplex_probs, dim3(static_cast<uint32_t>((max_cells + kRed - 1u) / kRed), c.n_pairs),
                       dim3(kRed), 0, st, c);
  if (c.bound)
    hipLaunchKernelGGL(k_duplex_bound, dim3((max_bases + kRed - 1u) / kRed, c.n_pairs), dim3(kRed), 0, st, c);
}

void launch_duplex_trace(const DuplexChunk& c, hipStream_t st) {
  hipLaunchKernelGGL(k_duplex_trace, dim3(c.n_pairs), dim3(64), 0, st, c);
}

}  // namespace rnamc
