// Byzantine-robust aggregation: coordinate-wise trimmed mean / median of M clients' fp32 arenas
// (Yin et al., "Byzantine-Robust Distributed Learning: Towards Optimal Statistical Rates", ICML
// 2018) in ONE pass that also writes the bf16 shadow and counts how often each client's value was
// the one trimmed (gfx950).
//
// Per coordinate, with v_0 .. v_{M-1} the clients' values and 0 <= 2k < M:
//   key(v) = b ^ ((b >> 31) & 0x7fffffff), b the float's bits as int32, compared signed:
//            -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN; ties broken by the slot index
//   sort the (key, slot) pairs ascending, drop the k lowest and the k highest,
//   acc = s[k]; acc = acc + s[k+1]; ...        (fp32, every addition rounded on its own)
//   out = acc * float(1 / (M - 2k))
// This is parallel/robust.py's torch_robust_, bit for bit.  k = 0 is the mean summed in sorted
// order, k = (M - 1) / 2 the median.  An alignment pad (every client +0) stays +0.
//
// The kernel is templated on M and k (a run-time k kept M launch-uniform predicates live in scalar
// registers across the sort and spilled some of them at M = 6 and 16): a thread loads one float4 from each of the M sources (nontemporal:
// each is read once), and sorts each of the four coordinates as M 64-bit composites (key in the
// high word, slot in the low one) with a compile-time Batcher odd-even merge network, every index
// a constant, so values and slots stay in registers.  The source pointers travel by value in the
// kernel arguments: virtual clients' masters are separate allocations.
#include "common.h"

#include <utility>

namespace {

constexpr int RA_MAX_M = 16;
constexpr int RA_COLS = RA_MAX_M + 1;  // counts row of a block: [slot 0..15 trimmed, non-finite outputs]

struct RobustArgs {
  const float* src[RA_MAX_M];
  float* out;
  bf16_t* shadow;  // nullable
  int* counts;     // nullable: [grid][RA_COLS]
  long long n4;
  float inv;
};

// Batcher's odd-even merge sort as a list of compare-exchanges; valid for every M (not only powers
// of two).  63 exchanges at M = 16.
template <int M>
struct SortNet {
  int a[96];
  int b[96];
  int n;
};

template <int M>
constexpr SortNet<M> make_sort_net() {
  SortNet<M> net{};
  int c = 0;
  for (int p = 1; p < M; p *= 2)
    for (int k = p; k >= 1; k /= 2)
      for (int j = k % p; j + k < M; j += 2 * k)
        for (int i = 0; i < k && i + j + k < M; ++i)
          if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
            net.a[c] = i + j;
            net.b[c] = i + j + k;
            ++c;
          }
  net.n = c;
  return net;
}

DEV void cmp_exchange(long long& a, long long& b) {
  const bool sw = b < a;
  const long long lo = sw ? b : a, hi = sw ? a : b;
  a = lo;
  b = hi;
}

template <int M, size_t... I>
DEV void sort_apply(long long (&c)[M], std::index_sequence<I...>) {
  constexpr SortNet<M> net = make_sort_net<M>();
  (cmp_exchange(c[net.a[I]], c[net.b[I]]), ...);
}

template <int M>
DEV void sort_composites(long long (&c)[M]) {
  sort_apply<M>(c, std::make_index_sequence<make_sort_net<M>().n>{});
}

DEV float4 ld_nt(const float4* p) {
  const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
  return make_float4(v[0], v[1], v[2], v[3]);
}

DEV int wave_sum_int(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One coordinate: the robust aggregate of vals[0..M), and the 16-bit mask of the trimmed slots.
template <int M, int K>
DEV float robust_coord(const float (&vals)[M], float inv, uint32_t& trimmed_mask) {
#pragma clang fp contract(off)
  long long c[M];
#pragma unroll
  for (int s = 0; s < M; ++s) {
    const int b = __float_as_int(vals[s]);
    const int key = b ^ ((b >> 31) & 0x7fffffff);
    c[s] = (long long)(((unsigned long long)(uint32_t)key << 32) | (uint32_t)s);
  }
  sort_composites<M>(c);
  float acc = 0.f;
  uint32_t mask = 0u;
#pragma unroll
  for (int j = 0; j < M; ++j) {
    const int key = (int)(c[j] >> 32);
    const float v = __int_as_float(key ^ ((key >> 31) & 0x7fffffff));
    const uint32_t bit = 1u << ((uint32_t)c[j] & 31u);
    if (j < K || j >= M - K) mask |= bit;
    else acc = j == K ? v : acc + v;
  }
  trimmed_mask = mask;
  return acc * inv;
}

template <int M, int K>
__global__ __launch_bounds__(256) void robust_agg_kernel(RobustArgs a) {
  int cnt[M];
#pragma unroll
  for (int s = 0; s < M; ++s) cnt[s] = 0;
  int nonfinite = 0;
  for (long long i = blockIdx.x * 256ll + threadIdx.x; i < a.n4; i += (long long)gridDim.x * 256) {
    float4 v4[M];
#pragma unroll
    for (int s = 0; s < M; ++s) v4[s] = ld_nt(reinterpret_cast<const float4*>(a.src[s]) + i);
    float o[4];
    uint32_t mk[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float vals[M];
#pragma unroll
      for (int s = 0; s < M; ++s) vals[s] = e == 0 ? v4[s].x : e == 1 ? v4[s].y : e == 2 ? v4[s].z : v4[s].w;
      o[e] = robust_coord<M, K>(vals, a.inv, mk[e]);
      nonfinite += (__float_as_uint(o[e]) & 0x7f800000u) == 0x7f800000u ? 1 : 0;
      // one coordinate's sort at a time: interleaving the four costs ~60 more VGPRs and spills
      // compare masks out of the scalar registers
      __builtin_amdgcn_sched_barrier(0);
    }
    // the four coordinates' masks side by side: one popcount pair per slot
    const uint32_t w01 = mk[0] | (mk[1] << 16), w23 = mk[2] | (mk[3] << 16);
#pragma unroll
    for (int s = 0; s < M; ++s) cnt[s] += __popc(w01 & (0x00010001u << s)) + __popc(w23 & (0x00010001u << s));
    reinterpret_cast<float4*>(a.out)[i] = make_float4(o[0], o[1], o[2], o[3]);
    if (a.shadow) reinterpret_cast<uint2*>(a.shadow)[i] = make_uint2(pack_bf2(o[0], o[1]), pack_bf2(o[2], o[3]));
  }
  if (!a.counts) return;  // uniform over the launch
  // lanes -> wave (shuffles) -> block (LDS, fixed order) -> one plain store per block and column:
  // no atomics, so every entry of every block row is written on every launch
  __shared__ int red[RA_COLS][4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int s = 0; s < M; ++s) {
    const int t = wave_sum_int(cnt[s]);
    if (lane == 0) red[s][wave] = t;
  }
  {
    const int t = wave_sum_int(nonfinite);
    if (lane == 0) red[RA_MAX_M][wave] = t;
  }
  __syncthreads();
  if (threadIdx.x < RA_COLS) {
    const int col = threadIdx.x;
    int t = 0;
    if (col < M || col == RA_MAX_M) t = ((red[col][0] + red[col][1]) + red[col][2]) + red[col][3];
    a.counts[(long long)blockIdx.x * RA_COLS + col] = t;
  }
}

int ra_grid_for(long long n4) { return (int)std::min<long long>((n4 + 255) / 256, 4096); }

// One instantiation per valid (M, k), k = 0 .. (M - 1) / 2: 71 kernels for M = 2 .. 16.
template <int M, int K>
bool ra_launch(const RobustArgs& a, hipStream_t st) {
  hipLaunchKernelGGL((robust_agg_kernel<M, K>), dim3(ra_grid_for(a.n4)), dim3(256), 0, st, a);
  return true;
}

template <int M, int... Ks>
bool ra_launch_k(int k, const RobustArgs& a, hipStream_t st, std::integer_sequence<int, Ks...>) {
  return ((k == Ks ? ra_launch<M, Ks>(a, st) : false) || ...);
}

template <int... Ms>  // Ms = M - 2
bool ra_launch_m(int M, int k, const RobustArgs& a, hipStream_t st, std::integer_sequence<int, Ms...>) {
  return ((M == Ms + 2 ? ra_launch_k<Ms + 2>(k, a, st, std::make_integer_sequence<int, (Ms + 3) / 2>{}) : false) || ...);
}

}  // namespace

extern "C" {

// Blocks of an fd_robust_agg launch over n floats (its counts buffer holds 17 ints per block): the
// grid of fd_server_opt.
int fd_robust_agg_grid(long long n) { return n > 0 ? ra_grid_for(n / 4) : 0; }

// out = the trimmed mean (k dropped at each end) of src[0..M) over n floats, shadow (nullable) =
// bf16(out), counts (nullable) = [grid][17] per-block trimmed counts per slot and non-finite
// outputs.  2 <= M <= 16, 0 <= 2k < M, n % 4 == 0; out / shadow must not overlap a source.
int fd_robust_agg(const float* const* src, int M, int k, float* out, void* shadow, int* counts, long long n,
                  hipStream_t st) {
  if (n <= 0 || n % 4 != 0) return 1;
  if (M < 2 || M > RA_MAX_M) return 2;
  if (k < 0 || 2 * k >= M) return 3;
  if (!src || !out) return 4;
  RobustArgs a{};
  for (int s = 0; s < M; ++s) {
    if (!src[s]) return 4;
    a.src[s] = src[s];
  }
  a.out = out;
  a.shadow = (bf16_t*)shadow;
  a.counts = counts;
  a.n4 = n / 4;
  a.inv = (float)(1.0 / (double)(M - 2 * k));
  return ra_launch_m(M, k, a, st, std::make_integer_sequence<int, RA_MAX_M - 1>{}) ? 0 : 5;
}

}  // extern "C"
