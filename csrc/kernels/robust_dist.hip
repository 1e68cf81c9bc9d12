// Distance-based Byzantine-robust aggregation of M clients' fp32 arenas (gfx950): multi-Krum
// (Blanchard et al., "Machine Learning with Adversaries: Byzantine Tolerant Gradient Descent",
// NeurIPS 2017) and the geometric median by smoothed Weiszfeld iterations (RFA: Pillutla, Kakade,
// Harchaoui, "Robust Aggregation for Federated Learning", IEEE TSP 2022).  Two streaming kernels
// that read the M arenas once per pass, and two one-block finalizers that turn their per-block
// partial sums into the next pass's weights on the device, so nothing goes back to the host between
// the passes.  The specification is parallel/robust_dist.py; every operation is rounded on its own
// (no FMA contraction).
//
//   fd_robust_pairdist        partial[block][p] = the block's sum of (x_i - x_j)^2 for the pair
//                             p = i (2M - i - 1) / 2 + (j - i - 1), i < j: the difference first, then
//                             the square (never G_ii + G_jj - 2 G_ij: client masters differ by ~1e-3
//                             of their norm and fp32 partial sums would cancel that away).  Per lane
//                             one fp32 accumulator per pair (the four components of a float4 in order,
//                             iterations in order), converted to double, reduced wave -> block in a
//                             fixed order, one double per block and pair.
//   fd_robust_krum_finalize   one block: D = the partials added over the blocks in a fixed two-level
//                             order (reduce_columns below: up to 16 threads per column);
//                             parallel/robust_dist.py krum_select(D, f, m), bit for bit:
//                               non-finite D[i][j] count as +inf;  c = max(1, M - f - 2);
//                               score_i = the c smallest D[i][j], j != i, added ascending in fp64;
//                               the m slots with the smallest (score, slot) and a finite score are
//                               selected: weight float(1 / m), every other slot +0;
//                               fewer than m finite scores: flag = 1 and every weight 0.
//   fd_robust_wmean           out = the weighted sum of the sources, weights and flag read from ctl
//                             on the device (launch-uniform):
//                               acc = w_a * x_a for the first slot with w != 0, then
//                               acc = acc + w_b * x_b for each later slot with w != 0, in slot order;
//                               a slot with weight 0 is skipped, not multiplied (its NaN never
//                               reaches out); no non-zero weight: +0.
//                             shadow (nullable) = bf16(out).  out == nullptr: neither is stored (pass
//                             0 of Weiszfeld, and its inner passes: only the distances are wanted).
//                             partial (nullable): [block][M + 1], per slot -- zero-weight slots
//                             included -- the block's sum of (x_s - out)^2 (fp32 difference against the
//                             rounded out, fp32 square, lane fp32 sums as above), then the block's
//                             count of non-finite outputs.  flag != 0: returns at once, nothing is
//                             written.
//   fd_robust_geomed_finalize one block: Dz = the partials added over the blocks in the same order;
//                             parallel/robust_dist.py geomed_weights(Dz, nu):
//                               w_i = 1 / max(nu, sqrt(Dz_i)) in fp64, 0 for a non-finite Dz_i;
//                               beta_i = w_i / sum(w) (the sum in slot order), ctl weight float(beta_i);
//                               objective = the sum of sqrt(Dz_i) over the finite slots;
//                               sum(w) == 0: flag = 1, every weight 0.
//
// Buffers.
//   ctl    float[20]:  [0..15] the slots' weights (slots >= M: 0), [16] the flag, [17..19] 0.
//   krum stats   double[288]:  [0..255] D as 16 x 16 (row i, column j; symmetric, diagonal 0, rows
//                and columns >= M: 0), [256..271] the scores, [272..287] 1.0 for a selected slot.
//   geomed stats double[rows][34], row `iter`:  [0] the objective, [1] the non-finite outputs of
//                the pass, [2..17] Dz, [18..33] beta in fp64 (before the rounding to ctl).
//
// No atomics: every output entry is written by exactly one plain store on every launch.
#include "common.h"

#include <cmath>
#include <utility>

namespace {

constexpr int RD_MAX_M = 16;
constexpr int RD_CTL = 20;
constexpr int RD_KRUM_STATS = 288;
constexpr int RD_GEOMED_ROW = 34;

struct PairArgs {
  const float* src[RD_MAX_M];
  double* partial;  // [grid][M (M - 1) / 2]
  long long n4;
};

struct WmeanArgs {
  const float* src[RD_MAX_M];
  const float* ctl;
  float* out;       // nullable
  bf16_t* shadow;   // nullable
  double* partial;  // nullable: [grid][M + 1]
  long long n4;
};

DEV float4 ld_nt(const float4* p) {
  const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
  return make_float4(v[0], v[1], v[2], v[3]);
}

DEV double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

DEV bool finite_f64(double v) { return fabs(v) <= 1.7976931348623157e308; }

template <int M>
__global__ __launch_bounds__(256) void robust_pairdist_kernel(PairArgs a) {
#pragma clang fp contract(off)
  constexpr int P = M * (M - 1) / 2;
  float acc[P];
#pragma unroll
  for (int p = 0; p < P; ++p) acc[p] = 0.f;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < a.n4; i += (long long)gridDim.x * 256) {
    float4 v[M];
#pragma unroll
    for (int s = 0; s < M; ++s) v[s] = ld_nt(reinterpret_cast<const float4*>(a.src[s]) + i);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float x[M];
#pragma unroll
      for (int s = 0; s < M; ++s) x[s] = e == 0 ? v[s].x : e == 1 ? v[s].y : e == 2 ? v[s].z : v[s].w;
      int p = 0;
#pragma unroll
      for (int s = 0; s < M; ++s)
#pragma unroll
        for (int t = s + 1; t < M; ++t, ++p) {
          const float d = x[s] - x[t];
          acc[p] = acc[p] + d * d;
        }
    }
  }
  // lanes -> wave (shuffles) -> block (LDS, fixed order) -> one plain store per block and pair
  __shared__ double red[P][4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const double t = wave_sum_f64((double)acc[p]);
    if (lane == 0) red[p][wave] = t;
  }
  __syncthreads();
  if (threadIdx.x < P) {
    const int p = threadIdx.x;
    a.partial[(long long)blockIdx.x * P + p] = ((red[p][0] + red[p][1]) + red[p][2]) + red[p][3];
  }
}

template <int M>
__global__ __launch_bounds__(256) void robust_wmean_kernel(WmeanArgs a) {
#pragma clang fp contract(off)
  if (a.ctl[16] != 0.f) return;  // uniform over the launch: the finalizer refused, nothing is written
  float w[M];
#pragma unroll
  for (int s = 0; s < M; ++s) w[s] = a.ctl[s];
  const bool dist = a.partial != nullptr;  // uniform
  float dz[M];
#pragma unroll
  for (int s = 0; s < M; ++s) dz[s] = 0.f;
  int nonfinite = 0;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < a.n4; i += (long long)gridDim.x * 256) {
    float4 v[M];
#pragma unroll
    for (int s = 0; s < M; ++s)  // (a zero-weight source is read only for its distance)
      if (dist || w[s] != 0.f) v[s] = ld_nt(reinterpret_cast<const float4*>(a.src[s]) + i);
      else v[s] = make_float4(0.f, 0.f, 0.f, 0.f);
    float o[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float x[M];
#pragma unroll
      for (int s = 0; s < M; ++s) x[s] = e == 0 ? v[s].x : e == 1 ? v[s].y : e == 2 ? v[s].z : v[s].w;
      float acc = 0.f;
      bool have = false;  // uniform: the weights are
#pragma unroll
      for (int s = 0; s < M; ++s)
        if (w[s] != 0.f) {
          const float t = w[s] * x[s];
          acc = have ? acc + t : t;
          have = true;
        }
      o[e] = acc;
      if (dist) {
        nonfinite += (__float_as_uint(acc) & 0x7f800000u) == 0x7f800000u ? 1 : 0;
#pragma unroll
        for (int s = 0; s < M; ++s) {
          const float d = x[s] - acc;
          dz[s] = dz[s] + d * d;
        }
      }
    }
    if (a.out) {
      reinterpret_cast<float4*>(a.out)[i] = make_float4(o[0], o[1], o[2], o[3]);
      if (a.shadow) reinterpret_cast<uint2*>(a.shadow)[i] = make_uint2(pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]));
    }
  }
  if (!dist) return;
  __shared__ double red[M + 1][4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int s = 0; s < M; ++s) {
    const double t = wave_sum_f64((double)dz[s]);
    if (lane == 0) red[s][wave] = t;
  }
  {
    const double t = wave_sum_f64((double)nonfinite);  // (exact: a block counts at most 2^22 per sweep)
    if (lane == 0) red[M][wave] = t;
  }
  __syncthreads();
  if (threadIdx.x < M + 1) {
    const int c = threadIdx.x;
    a.partial[(long long)blockIdx.x * (M + 1) + c] = ((red[c][0] + red[c][1]) + red[c][2]) + red[c][3];
  }
}

constexpr int RD_COLS = 128;   // columns a finalizer reduces at most (120 pairs at M = 16)
constexpr int RD_RANKS = 16;   // threads that share one column at most

// cols[c] = the block partials of column c, c < ncols <= 128, added in a fixed two-level order: with
// R = min(16, 256 / ncols), rank r < R adds the blocks r, r + R, r + 2R, ... in that order from 0.0, then
// the R rank sums are added in rank order from 0.0 (a rank with no block contributes 0.0).  The order
// depends on (grid, ncols) alone.
DEV void reduce_columns(const double* __restrict__ partial, int grid, int ncols, double* cols, double* tmp) {
#pragma clang fp contract(off)
  int R = 256 / ncols;
  if (R > RD_RANKS) R = RD_RANKS;
  const int r = (int)threadIdx.x / ncols, c = (int)threadIdx.x % ncols;
  if (r < R) {
    double acc = 0.0;
    for (int b = r; b < grid; b += R) acc = acc + partial[(long long)b * ncols + c];
    tmp[r * RD_COLS + c] = acc;
  }
  __syncthreads();
  if ((int)threadIdx.x < ncols) {
    double acc = 0.0;
    for (int k = 0; k < R; ++k) acc = acc + tmp[k * RD_COLS + threadIdx.x];
    cols[threadIdx.x] = acc;
  }
  __syncthreads();
}

__global__ __launch_bounds__(256) void robust_krum_finalize_kernel(const double* __restrict__ partial, int grid, int M,
                                                                    int f, int m, float* __restrict__ ctl,
                                                                    double* __restrict__ stats) {
#pragma clang fp contract(off)
  __shared__ double cols[RD_COLS];
  __shared__ double tmp[RD_RANKS * RD_COLS];
  __shared__ double D[RD_MAX_M][RD_MAX_M];
  __shared__ double row[RD_MAX_M][RD_MAX_M];
  __shared__ double score[RD_MAX_M];
  __shared__ int picked[RD_MAX_M];
  const int P = M * (M - 1) / 2;
  reduce_columns(partial, grid, P, cols, tmp);
  {
    const int i = threadIdx.x >> 4, j = threadIdx.x & 15;  // 256 threads: one entry of D each
    double d = 0.0;
    if (i < M && j < M && i != j) {
      const int lo = i < j ? i : j, hi = i < j ? j : i;
      d = cols[lo * (2 * M - lo - 1) / 2 + (hi - lo - 1)];
    }
    D[i][j] = d;
    stats[threadIdx.x] = d;
  }
  __syncthreads();
  const double inf = __builtin_huge_val();
  if ((int)threadIdx.x < M) {
    const int i = threadIdx.x;
    double* r = row[i];
    int cnt = 0;
    for (int j = 0; j < M; ++j) {  // insertion sort of the M - 1 distances, ascending
      if (j == i) continue;
      double d = D[i][j];
      if (!finite_f64(d)) d = inf;
      int k = cnt++;
      while (k > 0 && r[k - 1] > d) {
        r[k] = r[k - 1];
        --k;
      }
      r[k] = d;
    }
    int c = M - f - 2;
    if (c < 1) c = 1;
    if (c > M - 1) c = M - 1;
    double acc = 0.0;
    for (int k = 0; k < c; ++k) acc = acc + r[k];
    score[i] = acc;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  int finite = 0;
  for (int i = 0; i < RD_MAX_M; ++i) {
    picked[i] = 0;
    if (i < M && finite_f64(score[i])) ++finite;
  }
  const bool ok = finite >= m;
  if (ok)
    for (int t = 0; t < m; ++t) {  // the smallest (score, slot) not yet picked
      int best = -1;
      for (int i = 0; i < M; ++i)
        if (!picked[i] && finite_f64(score[i]) && (best < 0 || score[i] < score[best])) best = i;
      picked[best] = 1;
    }
  const float wsel = (float)(1.0 / (double)m);
  for (int i = 0; i < RD_MAX_M; ++i) {
    ctl[i] = picked[i] ? wsel : 0.f;
    stats[256 + i] = i < M ? score[i] : 0.0;
    stats[272 + i] = picked[i] ? 1.0 : 0.0;
  }
  ctl[16] = ok ? 0.f : 1.f;
  ctl[17] = ctl[18] = ctl[19] = 0.f;
}

__global__ __launch_bounds__(256) void robust_geomed_finalize_kernel(const double* __restrict__ partial, int grid,
                                                                      int M, double nu, int iter,
                                                                      float* __restrict__ ctl,
                                                                      double* __restrict__ stats) {
#pragma clang fp contract(off)
  __shared__ double cols[RD_COLS];
  __shared__ double tmp[RD_RANKS * RD_COLS];
  reduce_columns(partial, grid, M + 1, cols, tmp);
  if (threadIdx.x != 0) return;
  double* rowp = stats + (long long)iter * RD_GEOMED_ROW;
  double w[RD_MAX_M];
  double sum = 0.0, objective = 0.0;
#pragma unroll
  for (int i = 0; i < RD_MAX_M; ++i) {
    double wi = 0.0;
    if (i < M && finite_f64(cols[i])) {
      const double r = sqrt(cols[i]);
      objective = objective + r;
      wi = 1.0 / (r > nu ? r : nu);
    }
    if (i < M) sum = sum + wi;
    w[i] = wi;
  }
  const bool ok = sum != 0.0;
  rowp[0] = objective;
  rowp[1] = cols[M];
#pragma unroll
  for (int i = 0; i < RD_MAX_M; ++i) {
    const double beta = ok && i < M ? w[i] / sum : 0.0;
    rowp[2 + i] = i < M ? cols[i] : 0.0;
    rowp[18 + i] = beta;
    ctl[i] = (float)beta;
  }
  ctl[16] = ok ? 0.f : 1.f;
  ctl[17] = ctl[18] = ctl[19] = 0.f;
}

int rd_grid_for(long long n4) { return (int)std::min<long long>((n4 + 255) / 256, 4096); }

bool rd_overlap(const void* a, long long ab, const void* b, long long bb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + (uintptr_t)bb && b0 < a0 + (uintptr_t)ab;
}

template <int M>
bool rd_launch_pair(const PairArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((robust_pairdist_kernel<M>), dim3(rd_grid_for(a.n4)), dim3(256), 0, st, a);
  return true;
}

template <int M>
bool rd_launch_wmean(const WmeanArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((robust_wmean_kernel<M>), dim3(rd_grid_for(a.n4)), dim3(256), 0, st, a);
  return true;
}

template <int... Ms>  // Ms = M - 2
bool rd_pair_m(int M, const PairArgs& a, hipStream_t st, std::integer_sequence<int, Ms...>) {
  return ((M == Ms + 2 ? rd_launch_pair<Ms + 2>(a, st) : false) || ...);
}

template <int... Ms>  // Ms = M - 2
bool rd_wmean_m(int M, const WmeanArgs& a, hipStream_t st, std::integer_sequence<int, Ms...>) {
  return ((M == Ms + 2 ? rd_launch_wmean<Ms + 2>(a, st) : false) || ...);
}

}  // namespace

extern "C" {

// Blocks of an fd_robust_pairdist / fd_robust_wmean launch over n floats (their partial buffers hold
// M (M - 1) / 2 and M + 1 doubles per block): the grid of fd_robust_agg and fd_server_opt.
int fd_robust_dist_grid(long long n) { return n > 0 ? rd_grid_for(n / 4) : 0; }

// partial[grid][M (M - 1) / 2] = per block the sums of (src[i] - src[j])^2, i < j, over n floats.
// 2 <= M <= 16, n % 4 == 0; every entry of partial is overwritten.
int fd_robust_pairdist(const float* const* src, int M, double* partial, long long n, hipStream_t st) {
  if (n <= 0 || n % 4 != 0) return 1;
  if (M < 2 || M > RD_MAX_M) return 2;
  if (!src || !partial) return 4;
  PairArgs a{};
  for (int s = 0; s < M; ++s) {
    if (!src[s]) return 4;
    a.src[s] = src[s];
  }
  a.partial = partial;
  a.n4 = n / 4;
  return rd_pair_m(M, a, st, std::make_integer_sequence<int, RD_MAX_M - 1>{}) ? 0 : 5;
}

// ctl[20] / stats[288] = krum_select of the grid x M (M - 1) / 2 partials of fd_robust_pairdist.
int fd_robust_krum_finalize(const double* partial, int grid, int M, int f, int m, float* ctl, double* stats,
                            hipStream_t st) {
  if (M < 2 || M > RD_MAX_M) return 2;
  if (grid < 1 || grid > 4096) return 3;
  if (!partial || !ctl || !stats) return 4;
  if (f < 0 || m < 1 || m > M) return 6;
  hipLaunchKernelGGL(robust_krum_finalize_kernel, dim3(1), dim3(256), 0, st, partial, grid, M, f, m, ctl, stats);
  return 0;
}

// out (nullable) = the ctl-weighted sum of src[0..M) over n floats, shadow (nullable, needs out) =
// bf16(out), partial (nullable) = [grid][M + 1] squared distances to out and non-finite outputs.
// out / shadow must not overlap a source.
int fd_robust_wmean(const float* const* src, int M, const float* ctl, float* out, void* shadow, double* partial,
                    long long n, hipStream_t st) {
  if (n <= 0 || n % 4 != 0) return 1;
  if (M < 2 || M > RD_MAX_M) return 2;
  if (!src || !ctl) return 4;
  if (shadow && !out) return 4;
  WmeanArgs a{};
  for (int s = 0; s < M; ++s) {
    if (!src[s]) return 4;
    if (out && rd_overlap(src[s], n * 4, out, n * 4)) return 5;
    if (shadow && rd_overlap(src[s], n * 4, shadow, n * 2)) return 5;
    a.src[s] = src[s];
  }
  a.ctl = ctl;
  a.out = out;
  a.shadow = (bf16_t*)shadow;
  a.partial = partial;
  a.n4 = n / 4;
  return rd_wmean_m(M, a, st, std::make_integer_sequence<int, RD_MAX_M - 1>{}) ? 0 : 5;
}

// ctl[20] / row iter of stats[rows][34] = geomed_weights of the grid x (M + 1) partials of fd_robust_wmean.
int fd_robust_geomed_finalize(const double* partial, int grid, int M, double nu, int iter, float* ctl, double* stats,
                              hipStream_t st) {
  if (M < 2 || M > RD_MAX_M) return 2;
  if (grid < 1 || grid > 4096) return 3;
  if (!partial || !ctl || !stats) return 4;
  if (!std::isfinite(nu) || !(nu > 0.0) || iter < 0) return 6;
  hipLaunchKernelGGL(robust_geomed_finalize_kernel, dim3(1), dim3(256), 0, st, partial, grid, M, nu, iter, ctl, stats);
  return 0;
}

}  // extern "C"
